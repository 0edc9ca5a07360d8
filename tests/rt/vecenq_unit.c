/* vecenq_unit -- the host side of the vector fill, without a device and through
 * the public API only: odp_amd_cls_vec_geom against the runtime's vectors,
 * odp_amd_cls_pool_move_geom unchanged by a vector pool, the argument checks of
 * mi_cls_vec_fill that need no context, odp_amd_cls_vec_take (a pool that runs
 * short, every refusal) and odp_amd_cls_vec_enq over a batch filled here by the
 * literal loop of _odp_cos_vector_enq: the queues' events, the vectors' sizes
 * and packets, the queue stats and the pools' free counts.
 *
 * A stand-alone program: it is also the one to build with -fsanitize=address,
 * undefined together with the runtime's C sources.  Prints "ok" and returns 0,
 * or the line of the first failed check. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "odp_api.h"
#include "odp_cls_api.h"
#include "mi_cls.h"

#define CHECK(x)                                                        \
	do {                                                            \
		if (!(x)) {                                             \
			printf("FAIL %d: %s\n", __LINE__, #x);          \
			return 1;                                       \
		}                                                       \
	} while (0)

static odp_pool_t vec_pool(const char *name, uint32_t num, uint32_t max_size)
{
	odp_pool_param_t p;

	odp_pool_param_init(&p);
	p.type = ODP_POOL_VECTOR;
	p.vector.num = num;
	p.vector.max_size = max_size;
	return odp_pool_create(name, &p);
}

static odp_cos_t mkcos(const char *name, odp_queue_t *q, odp_pool_t vpool, uint32_t vmax)
{
	odp_cls_cos_param_t cp;
	odp_queue_param_t qp;

	odp_cls_cos_param_init(&cp);
	odp_queue_param_init(&qp);
	qp.type = ODP_QUEUE_TYPE_PLAIN;
	cp.action = ODP_COS_ACTION_ENQUEUE;
	cp.num_queue = 1;
	if (vpool != ODP_POOL_INVALID) {
		cp.vector.enable = true;
		cp.vector.pool = vpool;
		cp.vector.max_size = vmax;
	}
	*q = cp.queue = odp_queue_create(name, &qp);
	return odp_cls_cos_create(name, &cp);
}

/* the vectors a pool can still give (taken and put back) */
static int vec_free_count(odp_pool_t pool)
{
	odp_packet_vector_t v[64];
	int n = 0;

	while (n < 64 && (v[n] = odp_packet_vector_alloc(pool)) != ODP_PACKET_VECTOR_INVALID)
		n++;
	for (int i = 0; i < n; i++)
		odp_packet_vector_free(v[i]);
	return n;
}

static int pkt_free_count(odp_pool_t pool)
{
	odp_packet_t p[128];
	const int n = odp_packet_alloc_multi(pool, 64, p, 128);

	if (n > 0)
		odp_packet_free_multi(p, n);
	return n < 0 ? 0 : n;
}

#define NPK 20
#define NRUN 5

int main(void)
{
	odp_instance_t inst;

	if (odp_init_global(&inst, NULL, NULL) || odp_init_local(inst, ODP_THREAD_CONTROL))
		return 3;
	odp_schedule_config(NULL);

	/* ---- geometry ---------------------------------------------------- */
	odp_pool_param_t pp;

	odp_pool_param_init(&pp);
	pp.type = ODP_POOL_PACKET;
	pp.pkt.num = 64;
	pp.pkt.len = 256;
	const odp_pool_t pkpool = odp_pool_create("pk", &pp);

	CHECK(pkpool != ODP_POOL_INVALID);
	uint32_t mo[2], dfm[2];
	uint64_t lo[2], nb[2];
	const int g0 = odp_amd_cls_pool_move_geom(&mo[0], &dfm[0], &lo[0], &nb[0]);
	const odp_pool_t pa = vec_pool("vpoolA", 4, 4), pb = vec_pool("vpoolB", 16, 8);

	CHECK(pa != ODP_POOL_INVALID && pb != ODP_POOL_INVALID);
	/* a vector pool changes nothing in the packets' arena */
	CHECK(odp_amd_cls_pool_move_geom(&mo[1], &dfm[1], &lo[1], &nb[1]) == g0);
	CHECK(mo[0] == mo[1] && dfm[0] == dfm[1] && lo[0] == lo[1] && nb[0] == nb[1]);

	uint32_t size_off = 0, tbl_off = 0;
	uint64_t vlo = 1, vnb = 1;
	const int vg = odp_amd_cls_vec_geom(&size_off, &tbl_off, &vlo, &vnb);

	CHECK(vg == 0 || vg == -ENOENT);
	CHECK((vg == 0) == (vnb != 0) && (vg == 0) == (vlo != 0));
	CHECK(odp_amd_cls_vec_geom(NULL, &tbl_off, &vlo, &vnb) == -EINVAL);
	CHECK(odp_amd_cls_vec_geom(&size_off, &tbl_off, &vlo, NULL) == -EINVAL);
	{
		odp_packet_vector_t v = odp_packet_vector_alloc(pb);
		odp_packet_t *tbl;

		CHECK(v != ODP_PACKET_VECTOR_INVALID);
		odp_packet_vector_tbl(v, &tbl);
		CHECK((uintptr_t)tbl - (uintptr_t)v == tbl_off);
		CHECK(size_off % 4 == 0 && tbl_off % 8 == 0 && size_off + 4 <= tbl_off);
		odp_packet_vector_size_set(v, 5);
		CHECK(*(const uint32_t *)((const uint8_t *)v + size_off) == 5);
		if (vg == 0)
			CHECK((uint64_t)(uintptr_t)v >= vlo && (uint64_t)(uintptr_t)v + tbl_off + 8 * 8 <= vlo + vnb);
		odp_packet_vector_free(v);
	}

	/* ---- the control plane -------------------------------------------- */
	odp_queue_t qa, qb, qp;
	const odp_cos_t ca = mkcos("cosA", &qa, pa, 4), cb = mkcos("cosB", &qb, pb, 8);
	const odp_cos_t cp = mkcos("cosP", &qp, ODP_POOL_INVALID, 0);

	CHECK(ca != ODP_COS_INVALID && cb != ODP_COS_INVALID && cp != ODP_COS_INVALID);
	const uint32_t ia = (uint32_t)odp_cos_to_u64(ca) - 1u, ib = (uint32_t)odp_cos_to_u64(cb) - 1u;
	const uint32_t ip = (uint32_t)odp_cos_to_u64(cp) - 1u;
	static mi_cls_run_tab_t rtab;
	odp_pool_t vp[MI_CLS_RUN_VSLOTS];
	uint32_t ns = 0;
	uint64_t gen = 0;

	CHECK(odp_amd_cls_runtab_fill(&rtab, vp, &ns, &gen) == 0 && ns == 2);
	const uint32_t sa = rtab.vslot[ia], sb = rtab.vslot[ib];

	CHECK(vp[sa] == pa && vp[sb] == pb && rtab.vmax[ia] == 4 && rtab.vmax[ib] == 8);

	/* ---- mi_cls_vec_fill: what is checked before the context ---------- */
	{
		static uint64_t out[24];
		mi_cls_vec_args_t a;
		const int no_ctx = mi_cls_device_count() > 0 ? -EINVAL : -ENODEV;
		uint64_t t = 9;

		memset(&a, 0, sizeof(a));
		a.rtab = &rtab;
		a.size_off = size_off;
		a.tbl_off = tbl_off;
		a.vcap[sa] = 4;
		a.vcap[sb] = 8;
		a.varena_lo = 4096;
		a.varena_bytes = 4096;
		a.out = (mi_cls_vec_out_t *)out;
		CHECK(mi_cls_vec_fill(NULL, &a, NULL) == no_ctx);
		CHECK(mi_cls_vec_fill_host(NULL, &a) == no_ctx);
		CHECK(mi_cls_vec_fill_host_submit(NULL, &a, &t) == no_ctx && t == 0);
		CHECK(mi_cls_vec_fill_host_submit(NULL, &a, NULL) == -EINVAL);
		CHECK(mi_cls_vec_fill(NULL, NULL, NULL) == -EINVAL);
		mi_cls_vec_args_t b = a;

		b.rtab = NULL;
		CHECK(mi_cls_vec_fill(NULL, &b, NULL) == -EINVAL);
		b = a;
		b.size_off = size_off + 2;
		CHECK(mi_cls_vec_fill(NULL, &b, NULL) == -EINVAL);
		b = a;
		b.size_off = tbl_off;            /* the size word is not wholly before the table */
		CHECK(mi_cls_vec_fill(NULL, &b, NULL) == -EINVAL);
		b = a;
		b.tbl_off = tbl_off + 4;
		CHECK(mi_cls_vec_fill(NULL, &b, NULL) == -EINVAL);
		b = a;
		b.vcap[sa] = 3;                  /* the CoS's vmax exceeds its pool's max_size */
		CHECK(mi_cls_vec_fill_host(NULL, &b) == -EINVAL);
		b = a;
		b.vbase[3] = 2;                  /* vbase + vhave past nvgot */
		b.vhave[3] = 1;
		b.nvgot = 2;
		b.vgot = out;
		CHECK(mi_cls_vec_fill(NULL, &b, NULL) == -EINVAL);
		b.nvgot = 3;
		CHECK(mi_cls_vec_fill(NULL, &b, NULL) == no_ctx);
		b.vgot = NULL;                   /* vectors and no array */
		CHECK(mi_cls_vec_fill(NULL, &b, NULL) == -EINVAL);
		b = a;
		b.varena_lo = ~0ull - 63;        /* the arena wraps */
		b.varena_bytes = 128;
		CHECK(mi_cls_vec_fill(NULL, &b, NULL) == -EINVAL);
		b = a;
		b.n = (1u << 28);
		t = 9;
		CHECK(mi_cls_vec_fill_host_submit(NULL, &b, &t) == -EINVAL && t == 0);
		CHECK(mi_cls_vec_fill_host_wait(NULL, 1) == no_ctx);
		for (int i = 0; i < 24; i++)
			CHECK(out[i] == 0);
	}

	/* ---- odp_amd_cls_vec_take ------------------------------------------ */
	uint64_t need[MI_CLS_RUN_VSLOTS] = { 0 }, vgot[32];
	uint32_t vbase[MI_CLS_RUN_VSLOTS], vhave[MI_CLS_RUN_VSLOTS], vcap[MI_CLS_RUN_VSLOTS];

	need[sa] = 6;   /* the pool has 4 */
	need[sb] = 2;
	CHECK(odp_amd_cls_vec_take(vp, 17, need, vgot, 32, vbase, vhave, vcap) == -EINVAL);
	CHECK(odp_amd_cls_vec_take(NULL, 2, need, vgot, 32, vbase, vhave, vcap) == -EINVAL);
	CHECK(odp_amd_cls_vec_take(vp, 2, NULL, vgot, 32, vbase, vhave, vcap) == -EINVAL);
	CHECK(odp_amd_cls_vec_take(vp, 2, need, vgot, 32, NULL, vhave, vcap) == -EINVAL);
	{
		odp_pool_t bad[2] = { pa, pkpool };

		CHECK(odp_amd_cls_vec_take(bad, 2, need, vgot, 32, vbase, vhave, vcap) == -EINVAL);
	}
	CHECK(odp_amd_cls_vec_take(vp, 2, need, vgot, 5, vbase, vhave, vcap) == -ENOSPC);
	CHECK(odp_amd_cls_vec_take(vp, 2, need, NULL, 32, vbase, vhave, vcap) == -ENOSPC);
	CHECK(vec_free_count(pa) == 4 && vec_free_count(pb) == 16);   /* nothing was kept */
	CHECK(odp_amd_cls_vec_take(vp, 2, need, vgot, 32, vbase, vhave, vcap) == 6);
	CHECK(vhave[sa] == 4 && vhave[sb] == 2 && vcap[sa] == 4 && vcap[sb] == 8);
	CHECK(vbase[0] == 0 && vbase[1] == vhave[0] && vbase[2] == 6 && vhave[2] == 0 && vcap[15] == 0);
	CHECK(vec_free_count(pa) == 0 && vec_free_count(pb) == 14);
	for (uint32_t i = 0; i < 6; i++)
		CHECK(odp_packet_vector_pool((odp_packet_vector_t)(uintptr_t)vgot[i]) == (i - vbase[sa] < 4 ? pa : pb));

	/* ---- a batch, filled as the reference does it ----------------------- */
	odp_packet_t pk[NPK];

	CHECK(odp_packet_alloc_multi(pkpool, 64, pk, NPK) == NPK);
	const odp_queue_t dstq[3] = { qa, qb, qp };
	/* first, count, dst, cos, flags, nvec */
	const mi_cls_run_t runs[NRUN] = {
		{ 0, 9, 0, (uint8_t)ia, MI_CLS_RUN_VEC, 3 },   /* vectors of 4, 4, 1           */
		{ 9, 2, 2, (uint8_t)ip, 0, 0 },                 /* plain                        */
		{ 11, 6, 0, (uint8_t)ia, MI_CLS_RUN_VEC, 2 },  /* the stock ends: 4 in, 2 lost */
		{ 17, 1, 1, (uint8_t)ib, 0, 0 },                /* one packet: plain            */
		{ 18, 2, 0, (uint8_t)ia, MI_CLS_RUN_VEC, 1 },  /* no vector left: 2 lost       */
	};
	mi_cls_evrun_t evr[NRUN];
	uint64_t ev[NPK], lost[NPK];
	static mi_cls_vec_out_t out;
	uint32_t evn = 0, nlost = 0, next[MI_CLS_RUN_VSLOTS] = { 0 };

	for (int r = 0; r < NRUN; r++) {
		const mi_cls_run_t *u = &runs[r];
		const uint32_t s = rtab.vslot[u->cos], vm = rtab.vmax[u->cos];
		uint32_t done = 0, g = 0;

		evr[r].ev_first = evn;
		evr[r].vfirst = 0xFFFFFFFFu;
		if (!(u->flags & MI_CLS_RUN_VEC)) {
			for (uint32_t o = 0; o < u->count; o++)
				ev[evn++] = (uint64_t)(uintptr_t)pk[u->first + o];
			evr[r].ev_count = evr[r].pk_enq = u->count;
			continue;
		}
		for (uint32_t k = 0; k < u->nvec; k++) {
			if (next[s] >= vhave[s]) {
				ev[evn++] = 0;
				continue;
			}
			const uint32_t vi = vbase[s] + next[s]++, sz = u->count - done < vm ? u->count - done : vm;
			odp_packet_vector_t v = (odp_packet_vector_t)(uintptr_t)vgot[vi];
			odp_packet_t *tbl;

			if (g++ == 0)
				evr[r].vfirst = vi;
			odp_packet_vector_tbl(v, &tbl);
			memcpy(tbl, &pk[u->first + done], sz * sizeof(odp_packet_t));
			odp_packet_vector_size_set(v, sz);
			ev[evn++] = vgot[vi];
			done += sz;
			out.vectors++;
			out.in_vectors += sz;
		}
		for (uint32_t o = done; o < u->count; o++)
			lost[nlost++] = (uint64_t)(uintptr_t)pk[u->first + o];
		evr[r].ev_count = g;
		evr[r].pk_enq = done;
		out.events += g;
		out.vec_used[s] += u->nvec;
	}
	for (uint32_t s = 0; s < MI_CLS_RUN_VSLOTS; s++)
		if (out.vec_used[s] > vhave[s])
			out.vec_used[s] = vhave[s];
	out.ev_span = evn;
	out.lost = nlost;
	CHECK(evn == 9 && nlost == 4 && out.vectors == 4 && out.events == 4);

	/* ---- odp_amd_cls_vec_enq --------------------------------------------- */
	CHECK(odp_amd_cls_vec_enq(runs, evr, NRUN, ev, lost, nlost, dstq, 3, NULL, vp, ns, vgot, vbase, vhave,
				  &out, NULL, NULL, 0) == -EINVAL);
	CHECK(odp_amd_cls_vec_enq(runs, NULL, NRUN, ev, lost, nlost, dstq, 3, &rtab, vp, ns, vgot, vbase, vhave,
				  &out, NULL, NULL, 0) == -EINVAL);
	CHECK(odp_amd_cls_vec_enq(runs, evr, NRUN, ev, lost, nlost, dstq, 2, &rtab, vp, ns, vgot, vbase, vhave,
				  &out, NULL, NULL, 0) == -EINVAL);                     /* a destination id past ndst */
	CHECK(pkt_free_count(pkpool) == 64 - NPK);                       /* nothing was done */
	CHECK(odp_amd_cls_vec_enq(runs, evr, NRUN, ev, lost, nlost, dstq, 3, &rtab, vp, ns, vgot, vbase, vhave,
				  &out, NULL, NULL, 0) == 4 + 2 + 1);
	/* the lost packets are freed, the vectors not used are back */
	CHECK(pkt_free_count(pkpool) == 64 - NPK + 4);
	CHECK(vec_free_count(pa) == 0 && vec_free_count(pb) == 16);
	{
		odp_event_t e[8];
		const uint32_t want_size[4] = { 4, 4, 1, 4 }, want_first[4] = { 0, 4, 8, 11 };

		CHECK(odp_queue_deq_multi(qa, e, 8) == 4);
		for (int i = 0; i < 4; i++) {
			odp_packet_vector_t v = odp_packet_vector_from_event(e[i]);
			odp_packet_t *tbl;

			CHECK(odp_event_type(e[i]) == ODP_EVENT_PACKET_VECTOR && odp_packet_vector_valid(v));
			CHECK(odp_packet_vector_tbl(v, &tbl) == want_size[i]);
			for (uint32_t j = 0; j < want_size[i]; j++)
				CHECK(tbl[j] == pk[want_first[i] + j]);
			odp_packet_free_multi(tbl, (int)want_size[i]);
			odp_packet_vector_free(v);
		}
		CHECK(odp_queue_deq_multi(qp, e, 8) == 2 && e[0] == odp_packet_to_event(pk[9]) &&
		      e[1] == odp_packet_to_event(pk[10]));
		odp_event_free_multi(e, 2);
		CHECK(odp_queue_deq_multi(qb, e, 8) == 1 && e[0] == odp_packet_to_event(pk[17]));
		odp_event_free(e[0]);
	}
	CHECK(pkt_free_count(pkpool) == 64 && vec_free_count(pa) == 4);
	{
		odp_cls_queue_stats_t st;

		CHECK(odp_cls_queue_stats(ca, qa, &st) == 0 && st.packets == 13 && st.discards == 4);
		CHECK(odp_cls_queue_stats(cp, qp, &st) == 0 && st.packets == 2 && st.discards == 0);
		CHECK(odp_cls_queue_stats(cb, qb, &st) == 0 && st.packets == 1 && st.discards == 0);
	}
	/* ---- holes, a refused vector, a queue that takes nothing -------------- */
	{
		odp_packet_t p2[12];
		uint32_t seq2[12];
		uint64_t ent2[12], ev2[12], vg2[8];
		const odp_queue_t dq2[4] = { qa, qb, qp, ODP_QUEUE_INVALID };
		const mi_cls_run_t r2[3] = {
			{ 0, 3, 2, (uint8_t)ip, 0, 0 },                 /* plain, its second packet a hole    */
			{ 3, 6, 0, (uint8_t)ia, MI_CLS_RUN_VEC, 2 },   /* 4 + 2 packets, the second refused  */
			{ 9, 3, 3, (uint8_t)ia, MI_CLS_RUN_VEC, 1 },   /* to a queue that is not there       */
		};
		mi_cls_evrun_t x2[3] = { { 0, 3, 3, 0xFFFFFFFFu }, { 3, 2, 6, 0 }, { 5, 1, 3, 2 } };
		odp_packet_t *tbl;

		CHECK(odp_packet_alloc_multi(pkpool, 64, p2, 12) == 12);
		need[sa] = 3;
		need[sb] = 0;
		CHECK(odp_amd_cls_vec_take(vp, 2, need, vg2, 8, vbase, vhave, vcap) == 3 && vbase[sa] == 0);
		for (int i = 0; i < 12; i++) {
			seq2[i] = (uint32_t)i;
			ent2[i] = (uint64_t)(uintptr_t)p2[i] + 64;
		}
		ent2[1] = 0;   /* the move refused it: the packet stays the caller's */
		ev2[0] = ent2[0] - 64;
		ev2[1] = 0;
		ev2[2] = ent2[2] - 64;
		odp_packet_vector_tbl((odp_packet_vector_t)(uintptr_t)vg2[0], &tbl);
		memcpy(tbl, &p2[3], 4 * sizeof(odp_packet_t));
		odp_packet_vector_size_set((odp_packet_vector_t)(uintptr_t)vg2[0], 4);
		ev2[3] = vg2[0];
		ev2[4] = 0;    /* vector 1 was refused: packets 7 and 8 are in no vector */
		odp_packet_vector_tbl((odp_packet_vector_t)(uintptr_t)vg2[2], &tbl);
		memcpy(tbl, &p2[9], 3 * sizeof(odp_packet_t));
		odp_packet_vector_size_set((odp_packet_vector_t)(uintptr_t)vg2[2], 3);
		ev2[5] = vg2[2];
		memset(&out, 0, sizeof(out));
		out.holes = 1;
		out.refused = 1;
		out.vec_used[sa] = 3;
		CHECK(odp_amd_cls_vec_enq(r2, x2, 3, ev2, NULL, 0, dq2, 4, &rtab, vp, ns, vg2, vbase, vhave, &out, seq2,
					  ent2, 64) == 2 + 1);
		/* packets 7, 8 (refused vector) and 9 - 11 (no queue) are freed, and vector 2 */
		CHECK(pkt_free_count(pkpool) == 64 - 12 + 5 && vec_free_count(pa) == 2);
		odp_event_t e[4];

		CHECK(odp_queue_deq_multi(qp, e, 4) == 2 && e[0] == odp_packet_to_event(p2[0]) &&
		      e[1] == odp_packet_to_event(p2[2]));
		odp_event_free_multi(e, 2);
		CHECK(odp_queue_deq_multi(qa, e, 4) == 1);
		CHECK(odp_packet_vector_tbl(odp_packet_vector_from_event(e[0]), &tbl) == 4 && tbl[0] == p2[3] &&
		      tbl[3] == p2[6]);
		odp_packet_free_multi(tbl, 4);
		odp_packet_vector_free(odp_packet_vector_from_event(e[0]));
		odp_packet_free(p2[1]);
		odp_packet_vector_free((odp_packet_vector_t)(uintptr_t)vg2[1]);   /* the "refused" one */
		CHECK(pkt_free_count(pkpool) == 64 && vec_free_count(pa) == 4);
		odp_cls_queue_stats_t st;

		CHECK(odp_cls_queue_stats(cp, qp, &st) == 0 && st.packets == 2 + 2 && st.discards == 1);
		CHECK(odp_cls_queue_stats(ca, qa, &st) == 0 && st.packets == 13 + 4 && st.discards == 4 + 2 + 3);
	}
	/* an empty batch: nothing to do, the vectors taken go back */
	need[sa] = 3;
	need[sb] = 0;
	CHECK(odp_amd_cls_vec_take(vp, 2, need, vgot, 32, vbase, vhave, vcap) == 3 && vec_free_count(pa) == 1);
	memset(&out, 0, sizeof(out));
	CHECK(odp_amd_cls_vec_enq(NULL, NULL, 0, NULL, NULL, 0, dstq, 3, &rtab, vp, ns, vgot, vbase, vhave, &out, NULL,
				  NULL, 0) == 0);
	CHECK(vec_free_count(pa) == 4);
	printf("ok\n");
	return 0;
}
