/*
 * odp_pktin.c -- the receive path of the "loop" and "pcap" pktios, whole:
 * staging, the host delivery, the GPU delivery, the one-submission receive
 * chain and the pipelined pktio_recv.  Every function a burst runs through
 * is in this unit.
 *
 * Reference behaviour:
 *   platform/linux-generic/pktio/loop.c:253-384   loopback_recv
 *   platform/linux-generic/pktio/pcap.c:299-352   pcapif_recv_pkt
 *   include/odp_classification_internal.h:142-236 _odp_cls_enq run batching
 *
 * The receive path replaces the reference's per-packet
 *   _odp_packet_parse_common() + _odp_cls_classify_packet()
 * with ONE batched GPU launch per burst: the burst's frames are packed into a
 * pinned staging buffer at 64-byte aligned offsets, parsed and classified by
 * mi_cls_kernel (odp_amd_cls_classify_host -> mi_cls_classify_host), and the
 * 16-byte result records drive the host side exactly as the reference's
 * return codes do:
 *   parse != 0            -> in_errors++        (loop.c:311-312)
 *   parse  < 0            -> drop               (loop.c:314-317)
 *   classify < 0          -> in_discards++, drop (loop.c:324-330)
 *   classify > 0 (DROP)   -> drop
 *   pool switch           -> copy into the CoS pool (loop.c:332-337)
 *   no error flags        -> in_packets / in_octets (loop.c:352-355)
 *   enqueue               -> runs of equal (dst_queue, cos) in arrival order
 *                            (_odp_cls_enq / _odp_cos_enq + queue stats)
 */
#define _GNU_SOURCE
#include <errno.h>
#include <x86intrin.h>
#include <string.h>

#include "odp_pktio_internal.h"

int rx_prof = -1;

uint32_t rx_burst(void)
{
	static uint32_t b;

	if (!b) {
		const char *e = getenv("ODP_AMD_RX_BURST");

		b = e && atoi(e) > 0 ? (uint32_t)atoi(e) : RX_BURST_DEFAULT;
	}
	return b;
}

/* ODP_AMD_RX_PIPELINE=0: classify each burst synchronously */
static int rx_pipeline(void)
{
	static int on = -1;

	return env_switch("ODP_AMD_RX_PIPELINE", &on);
}

/* ODP_AMD_RX_GPU_DELIVER=0: host delivery only */
static int gpu_deliver_on(void)
{
	static int on = -1;

	return env_switch("ODP_AMD_RX_GPU_DELIVER", &on);
}

/* ODP_AMD_RX_CHAIN=0: no receive chain (below) */
static int rx_chain_on(void)
{
	static int on = -1;

	return env_switch("ODP_AMD_RX_CHAIN", &on);
}

/* ============================================================ burst sets */
static void rx_set_arrays_free(rx_set_t *s)
{
	hmem_free(s->soff, s->arr_pinned);
	hmem_free(s->slen, s->arr_pinned);
	hmem_free(s->res, s->arr_pinned);
	hmem_free(s->dlv, s->dlv_pinned);
	hmem_free(s->perm, s->dlv_pinned);
	hmem_free(s->gcnt, s->dlv_pinned);
	free(s->ent);
	free(s->old);
	hmem_free(s->ppool, s->pk_pinned);
	free(s->pdoff);
	free(s->pup);
	s->pup = NULL;
	s->dlv = NULL;
	s->perm = NULL;
	s->gcnt = NULL;
	s->ent = NULL;
	s->old = NULL;
	s->ppool = NULL;
	s->pdoff = NULL;
	s->dlv_pinned = 0;
	hmem_free(s->pk, s->pk_pinned);
	hmem_free(s->dec, s->rxc_pinned);
	hmem_free(s->cent, s->rxc_pinned);
	hmem_free(s->got, s->rxc_pinned);
	hmem_free(s->rxo, s->rxc_pinned);
	s->dec = NULL;
	s->cent = NULL;
	s->got = NULL;
	s->rxo = NULL;
	s->got_cap = 0;
	s->rxc_pinned = 0;
	free(s->tmp);
	s->tmp = NULL;
	s->tmp_cap = 0;
	s->soff = NULL;
	s->slen = NULL;
	s->res = NULL;
	s->pk = NULL;
	s->n_cap = 0;
}

void rx_sets_free(rt_pktio_t *e)
{
	hmem_free(e->rxtab, e->rxtab_pinned);
	e->rxtab = NULL;
	e->rxtab_pinned = 0;
	e->rxtab_ok = 0;
	e->rxtab_gen = 0;
	e->rx_np = 0;
	for (int k = 0; k < RX_SETS; k++) {
		rx_set_t *s = &e->rs[k];

		hmem_free(s->stage, s->stage_pinned);
		rx_set_arrays_free(s);
		memset(s, 0, sizeof(*s));
	}
}

/* descriptor arrays for n frames; stage bytes grow keeping the contents */
int stage_reserve(rx_set_t *s, uint32_t n, size_t bytes)
{
	if (n > s->n_cap) {
		uint32_t c = n < 256 ? 256 : n;
		int p1, p2, p3;

		rx_set_arrays_free(s);
		s->soff = hmem_alloc(c * sizeof(uint32_t), &p1);
		s->slen = hmem_alloc(c * sizeof(uint16_t), &p2);
		s->res = hmem_alloc(c * sizeof(mi_cls_result_t), &p3);
		s->arr_pinned = p1;
		int k1, k2;

		s->pk = hmem_alloc(c * sizeof(odp_packet_t), &k1);
		s->ppool = hmem_alloc(c, &k2);
		s->pk_pinned = k1 && k2;
		if (k1 != k2 && s->pk && s->ppool) {   /* mixed: ordinary copies */
			hmem_free(s->pk, k1);
			hmem_free(s->ppool, k2);
			s->pk = malloc(c * sizeof(odp_packet_t));
			s->ppool = malloc(c);
		}
		if (p1 != p2 || p1 != p3) {   /* mixed: keep the pageable copies */
			hmem_free(s->soff, p1);
			hmem_free(s->slen, p2);
			hmem_free(s->res, p3);
			s->soff = malloc(c * sizeof(uint32_t));
			s->slen = malloc(c * sizeof(uint16_t));
			s->res = malloc(c * sizeof(mi_cls_result_t));
			s->arr_pinned = 0;
		}
		if (!s->soff || !s->slen || !s->res || !s->pk) {
			rx_set_arrays_free(s);
			return -1;
		}
		/* GPU delivery arrays: only when all three are page-locked */
		int q1, q2, q3;

		s->dlv = hmem_alloc(c * sizeof(mi_cls_dlv_t), &q1);
		s->perm = hmem_alloc(c * sizeof(uint32_t), &q2);
		s->gcnt = hmem_alloc(RX_SLICES * MI_CLS_DLV_GROUPS * sizeof(uint32_t), &q3);
		s->ent = malloc(c * sizeof(odp_packet_t));
		s->old = malloc(c * sizeof(odp_packet_t));
		s->pdoff = malloc(c * sizeof(uint16_t));
		s->pup = malloc(c * sizeof(void *));
		if (!s->ppool || !s->pdoff || !s->pup) {
			rx_set_arrays_free(s);
			return -1;
		}
		/* receive chain arrays (page-locked or none) */
		{
			int r1, r2, r3, r4;

			s->dec = hmem_alloc(c * sizeof(uint32_t), &r1);
			s->cent = hmem_alloc(c * sizeof(uint64_t), &r2);
			s->got = hmem_alloc((size_t)4 * c * sizeof(uint64_t), &r3);
			s->rxo = hmem_alloc(RX_SLICES * sizeof(mi_cls_rx_out_t), &r4);
			s->rxc_pinned = r1 && r2 && r3 && r4;
			s->got_cap = 4u * c;
			if (!s->rxc_pinned) {
				hmem_free(s->dec, r1);
				hmem_free(s->cent, r2);
				hmem_free(s->got, r3);
				hmem_free(s->rxo, r4);
				s->dec = NULL;
				s->cent = NULL;
				s->got = NULL;
				s->rxo = NULL;
				s->got_cap = 0;
			}
		}
		s->dlv_pinned = q1 && q2 && q3 && s->dlv && s->perm && s->gcnt && s->ent && s->old;
		if (!s->dlv_pinned) {
			hmem_free(s->dlv, q1);
			hmem_free(s->perm, q2);
			hmem_free(s->gcnt, q3);
			free(s->ent);
			free(s->old);
			s->dlv = NULL;
			s->perm = NULL;
			s->gcnt = NULL;
			s->ent = NULL;
			s->old = NULL;
		}
		s->n_cap = c;
	}
	if (bytes > s->stage_cap) {
		size_t c = s->stage_cap ? s->stage_cap : (4u << 20);
		int pinned;

		while (c < bytes)
			c *= 2;
		uint8_t *ns = hmem_alloc(c, &pinned);

		if (!ns)
			return -1;
		if (s->stage) {
			memcpy(ns, s->stage, s->stage_cap);
			hmem_free(s->stage, s->stage_pinned);
		}
		s->stage = ns;
		s->stage_pinned = pinned;
		s->stage_cap = c;
	}
	return 0;
}

/* Host-side masking for parser layers below L4 (odp_parse.c:372-414): the
 * L2 / L3 parts of the full parse are identical at any layer; the layer only
 * cuts what is recorded and whether an L4 truncation drops. */
static void apply_layer(mi_cls_result_t *r, odp_proto_layer_t layer)
{
	/* l2 l3 eth eth_bcast eth_mcast jumbo vlan vlan_qinq */
	const uint32_t L2F = (1u << 3) | (0x3fu << 6);
	/* + l3 arp ipv4 ipv6 ip_bcast ip_mcast ipfrag ipopt */
	const uint32_t L3F = L2F | (1u << 4) | (0x7fu << 12);

	if (layer >= ODP_PROTO_LAYER_L4)
		return;
	/* an L4 truncation does not drop below L4; a drop_ipv4/6_err drop
	 * (ip_err set, L3 options) does */
	if (r->outcome == MI_CLS_OUT_PARSE_DROP && !(layer == ODP_PROTO_LAYER_L3 && (r->err & 0x02)))
		r->outcome = MI_CLS_OUT_DISCARD;
	if (layer == ODP_PROTO_LAYER_L2) {
		r->in_flags &= L2F;
		r->err &= 0x01;     /* snap_len_err */
		r->l4_offset = ODP_PACKET_OFFSET_INVALID;
	} else {
		r->in_flags &= L3F | (1u << 30);   /* + l3_chksum_done */
		r->err &= 0x07;     /* snap_len_err, ip_err, l3_chksum_err */
	}
}

/* Queue slot of dst inside the CoS (_odp_cos_queue_idx,
 * odp_classification_internal.h:49-65): 0 for a single-queue CoS. */
static uint32_t cos_slot_of(uint32_t cos_index, odp_queue_t dst)
{
	odp_cos_t cos = (odp_cos_t)(uintptr_t)(cos_index + 1u);
	uint32_t nq = odp_cls_cos_num_queue(cos), slot = 0;

	if (nq > 1) {
		odp_queue_t qs[32];

		odp_cls_cos_queues(cos, qs, 32);
		for (uint32_t i = 0; i < nq; i++)
			if (qs[i] == dst)
				slot = i;
	}
	return slot;
}

/* _odp_cos_vector_enq (odp_classification_internal.h:83-137): the run goes
 * into ceil(num / max_size) packet vectors, all full but the last; what the
 * vector pool cannot hold is counted as discards.  (The reference leaves the
 * packets it could not place unreferenced; here they are freed.) */
static void cos_vector_enq(odp_queue_t queue, odp_packet_t pk[], int num, uint32_t cos,
			   odp_pool_t vpool, uint32_t max_size)
{
	const uint32_t slot = cos_slot_of(cos, queue);
	int num_pktv = (int)(((uint32_t)num + max_size - 1) / max_size);
	odp_event_t ev[num_pktv];
	odp_packet_vector_t pv[num_pktv];
	int i;

	for (i = 0; i < num_pktv; i++) {
		pv[i] = odp_packet_vector_alloc(vpool);
		if (pv[i] == ODP_PACKET_VECTOR_INVALID)
			break;
		ev[i] = odp_packet_vector_to_event(pv[i]);
	}
	if (i == 0) {
		odp_packet_free_multi(pk, num);
		odp_amd_cls_queue_stats_add(cos, slot, 0, (uint64_t)num);
		return;
	}
	num_pktv = i;
	uint32_t num_enq = 0;

	for (i = 0; i < num_pktv; i++) {
		odp_packet_t *tbl;
		uint32_t sz = max_size;

		if (num_enq + max_size > (uint32_t)num)
			sz = (uint32_t)num - num_enq;
		odp_packet_vector_tbl(pv[i], &tbl);
		memcpy(tbl, &pk[num_enq], sz * sizeof(odp_packet_t));
		odp_packet_vector_size_set(pv[i], sz);
		num_enq += sz;
	}
	if (num_enq < (uint32_t)num)
		odp_packet_free_multi(&pk[num_enq], num - (int)num_enq);
	int ret = odp_queue_enq_multi(queue, ev, num_pktv);

	if (ret == num_pktv) {
		odp_amd_cls_queue_stats_add(cos, slot, num_enq, (uint64_t)num - num_enq);
		return;
	}
	if (ret < 0)
		ret = 0;
	uint32_t enqueued = max_size * (uint32_t)ret;

	odp_amd_cls_queue_stats_add(cos, slot, enqueued, (uint64_t)num - enqueued);
	for (i = ret; i < num_pktv; i++) {
		odp_packet_t *tbl;
		uint32_t sz = odp_packet_vector_tbl(pv[i], &tbl);

		odp_packet_free_multi(tbl, (int)sz);
		odp_packet_vector_free(pv[i]);
	}
}

/* The plain enqueue of pk[0..num) to q: the packets the queue did not take
 * (all of them for an invalid queue) are freed.  Returns how many it took. */
static inline int rx_enq_plain(odp_queue_t q, odp_packet_t pk[], int num)
{
	int r = q == ODP_QUEUE_INVALID ? -1
		: odp_queue_enq_multi(q, (const odp_event_t *)(void *)pk, num);

	if (r < 0)
		r = 0;
	if (r != num)
		odp_packet_free_multi(&pk[r], num - r);
	return r;
}

/* One enqueue run (equal dst_queue and cos): _odp_cos_enq
 * (odp_classification_internal.h:142-167).  Single packets and CoS without
 * packet vectors take the plain enqueue -- to odp_queue_aggr(dst, 0) for a
 * hash-queue CoS with event aggregators -- others go into packet vectors;
 * queue stats are kept on the CoS queue (dst). */
static void cos_enq_run(odp_packet_t pk[], int num)
{
	pkt_hdr_t *h = rt_pkt_hdr(pk[0]);
	const uint32_t cos = h->cos;
	odp_queue_t dst = h->dst_queue;
	odp_pool_t vpool = ODP_POOL_INVALID;
	uint32_t vmax = 0;
	int use_aggr = 0;
	const int std = odp_amd_cls_cos_enq_mode(cos, &vpool, &vmax, &use_aggr);

	if (num < 2 || std != 0) {
		const int r = rx_enq_plain(use_aggr ? odp_queue_aggr(dst, 0) : dst, pk, num);

		odp_amd_cls_queue_stats_add(cos, cos_slot_of(cos, dst), (uint64_t)r,
					    (uint64_t)(num - r));
		return;
	}
	cos_vector_enq(dst, pk, num, cos, vpool, vmax);
}

/* One enqueue per queue group (rx_enqueue, rx_dlv_end, rxc_end): the
 * group's packets pk[0..num), in arrival order, go to q with one call, and
 * the queue statistics are kept as per run of the reference (_odp_cos_enq):
 * per CoS of the queue, cos[k] being the CoS of pk[k] -- the first packets
 * the queue took counted as enqueued, the rest (freed) as discards. */
static inline void rx_enq_group(odp_queue_t q, odp_packet_t pk[], const uint8_t cos[], int num)
{
	const int r = rx_enq_plain(q, pk, num);
	uint64_t ok[256], bad[256];
	uint8_t seen[256], cl[256];
	int ncos = 0;

	/* by stretches of one CoS [k, e): most groups are a single one */
	for (int k = 0, e; k < num; k = e) {
		const uint32_t c = cos[k];

		for (e = k + 1; e < num && cos[e] == c; e++)
			;
		const int took = r <= k ? 0 : (r < e ? r : e) - k;

		if (k == 0) {
			if (e == num) {
				odp_amd_cls_queue_stats_add(c, cos_slot_of(c, q), (uint64_t)took,
							    (uint64_t)(num - took));
				return;
			}
			memset(seen, 0, sizeof(seen));
		}
		if (!seen[c]) {
			seen[c] = 1;
			cl[ncos++] = (uint8_t)c;
			ok[c] = 0;
			bad[c] = 0;
		}
		ok[c] += (uint64_t)took;
		bad[c] += (uint64_t)(e - k - took);
	}
	for (int k = 0; k < ncos; k++)
		odp_amd_cls_queue_stats_add(cl[k], cos_slot_of(cl[k], q), ok[cl[k]], bad[cl[k]]);
}

/* The queue groups of a burst: every queue seen so far, found through an
 * open-addressing table. */
#define RX_GROUP_MAXQ 64
#define RX_GROUP_HASH 256      /* slots: queue -> group */
typedef struct {
	odp_queue_t q[RX_GROUP_MAXQ];
	uint8_t slot[RX_GROUP_HASH];   /* group + 1, 0 empty */
	int n;
} rx_qgroups_t;

/* Group of queue q, added when new; -1 when it would be one more than
 * RX_GROUP_MAXQ. */
static inline int rx_qgroup_of(rx_qgroups_t *g, odp_queue_t q)
{
	/* top 8 bits: RX_GROUP_HASH slots */
	uint32_t sl = (uint32_t)(((uint64_t)(uintptr_t)q * 0x9E3779B97F4A7C15ull) >> 56);

	while (g->slot[sl] && g->q[g->slot[sl] - 1] != q)
		sl = (sl + 1) & (RX_GROUP_HASH - 1);
	if (!g->slot[sl]) {
		if (g->n == RX_GROUP_MAXQ)
			return -1;
		g->q[g->n] = q;
		g->slot[sl] = (uint8_t)++g->n;
	}
	return g->slot[sl] - 1;
}

/* Whether a CoS's runs take the plain enqueue (no packet vectors, no
 * aggregator), looked up once per burst: mode[] is 1 plain, 0 not, -1 not
 * looked up yet. */
static inline int rx_cos_plain(int8_t mode[256], uint32_t cos)
{
	if (mode[cos] < 0) {
		odp_pool_t vp = ODP_POOL_INVALID;
		uint32_t vmax = 0;
		int aggr = 0;
		const int std = odp_amd_cls_cos_enq_mode(cos, &vp, &vmax, &aggr);

		mode[cos] = std > 0 && !aggr;
	}
	return mode[cos];
}

/* ============================================================ staging */
/* The chain's table for the current control-plane generation: refilled when
 * it changed; 0 when the chain can serve this pktio (every pool of the
 * table page-locked). */
static int rxc_table(rt_pktio_t *e)
{
	const uint64_t g = odp_amd_cls_generation();

	if (e->rxtab && e->rxtab_gen == g)
		return e->rxtab_ok ? 0 : -1;
	if (!e->rxtab) {
		e->rxtab = hmem_alloc(sizeof(mi_cls_rxtab_t), &e->rxtab_pinned);
		if (!e->rxtab)
			return -1;
	}
	uint64_t tg = 0;
	uint32_t np = 0;
	int ok = e->rxtab_pinned &&
		 odp_amd_cls_rxtab_fill(e->pool, e->rxtab, e->rx_pools, &np, &tg) == 0;

	for (uint32_t k = 0; ok && k < np; k++) {
		rt_pool_t *rp = rt_pool(e->rx_pools[k]);
		const int idx = odp_pool_index(e->rx_pools[k]);

		ok = rp && rp->pinned && rp->param.type == ODP_POOL_PACKET && idx >= 0 && idx < 64;
		if (ok) {
			e->rxtab->pool_cap[k] = rp->data_cap;
			e->rxtab->rt_slot[idx] = (uint8_t)(k + 1u);
		}
	}
	for (int k = 0; ok && k < RT_MAX_POOLS && k < 64; k++) {
		rt_pool_t *rp = rt_pool((odp_pool_t)(uintptr_t)(k + 1));

		e->rxtab->rt_pinned[k] = rp && rp->pinned;
	}
	if (e->rx_np != np)
		memset(e->rx_want, 0, sizeof(e->rx_want));   /* first bursts: as many as frames */
	e->rx_np = np;
	e->rxtab_gen = tg;
	{
		/* a new stamp per rewrite: the device's copies follow it */
		static uint64_t stamps;

		e->rxtab->stamp = __atomic_add_fetch(&stamps, 1, __ATOMIC_RELAXED);
	}
	e->rxtab_ok = ok && tg == g;
	return e->rxtab_ok ? 0 : -1;
}

/* Whether this pktio's loop bursts can be staged by the GPU (the chain's
 * conditions, and an arena of page-locked pools to address them in). */
static int rxc_loop_stage_ok(rt_pktio_t *e, rx_set_t *s, uint32_t max)
{
	uint8_t *lo = NULL;
	size_t span = 0;

	/* only a burst that will really be submitted to the chain (pktio_recv
	 * submits with the pipeline on only) is left for the GPU to stage */
	return rx_chain_on() && rx_pipeline() && gpu_deliver_on() && e->cls_enabled &&
	       e->parse_layer == ODP_PROTO_LAYER_ALL &&
	       s->rxc_pinned && s->dlv_pinned && s->arr_pinned && s->pk_pinned && max > 0 &&
	       max <= MI_CLS_DLV_GROUP_MAX && rt_pinned_arena(&lo, &span) && span < OOB_SPAN &&
	       rxc_table(e) == 0;
}

/* The host's staging of n loop packets already in s->pk: lengths, pools,
 * headrooms, user pointers and the descriptors.  Packets of page-locked
 * pools are classified in place: the descriptors are their data addresses
 * relative to the lowest pinned pool (one base for the burst; the GPU
 * addresses that memory at the host's addresses).  A burst with a packet
 * outside that range is copied into the stage instead.  0, or -1 when the
 * stage cannot grow. */
static int loop_stage_hdrs(rt_pktio_t *e, rx_set_t *s, uint32_t n)
{
	uint8_t *lo = NULL;
	size_t span = 0, off = 0;
	int in_place = s->arr_pinned && rt_pinned_arena(&lo, &span) && span < OOB_SPAN;
	uint8_t pinned_of[RT_MAX_POOLS];

	(void)e;
	for (int k = 0; k < RT_MAX_POOLS; k++) {
		rt_pool_t *rp = rt_pool((odp_pool_t)(uintptr_t)(k + 1));

		pinned_of[k] = rp && rp->pinned;
	}
	/* header prefetch distance (ODP_AMD_LOOP_PF, A/B; 16 -> 96: loop receive
	 * 17.5 -> 20.0 Mpkt/s, profiles/r04pf_loop_prefetch_ab.txt) */
	static int pf = -1;

	if (pf < 0)
		pf = getenv("ODP_AMD_LOOP_PF") ? atoi(getenv("ODP_AMD_LOOP_PF")) : 96;
	for (uint32_t i = 0; i < n; i++) {
		if (i + pf < n) {   /* both header lines (the sender wrote them) */
			const uint8_t *nh = (const uint8_t *)rt_pkt_hdr(s->pk[i + pf]);

			__builtin_prefetch(nh);
			__builtin_prefetch(nh + 64);
		}
		pkt_hdr_t *h = rt_pkt_hdr(s->pk[i]);
		const uint8_t *d = h->head + h->data_off;
		uint32_t l = h->len > 65535 ? 65535 : h->len;
		const uint32_t pi = h->ev.pool;

		s->slen[i] = (uint16_t)l;
		s->ppool[i] = (uint8_t)(pi + 1u);
		s->pdoff[i] = (uint16_t)h->data_off;
		s->pup[i] = h->user_ptr;
		if (in_place && pinned_of[pi] && d >= lo && (size_t)(d - lo) + l + 16u <= span)
			s->soff[i] = (uint32_t)(d - lo);
		else
			in_place = 0;
	}
	if (in_place) {
		s->base = lo;
		s->bytes = span;
		return 0;
	}
	for (uint32_t i = 0; i < n; i++) {
		pkt_hdr_t *h = rt_pkt_hdr(s->pk[i]);
		const uint32_t l = s->slen[i];

		if (stage_reserve(s, n, off + l + 64))
			return -1;
		memcpy(s->stage + off, h->head + h->data_off, l);
		s->soff[i] = (uint32_t)off;
		off += (l + 63u) & ~63u;
	}
	s->base = s->stage;
	s->bytes = off + 64;
	return 0;
}

/* Pull up to `max` frames from the driver into staging set s.  pcap frames
 * in a page-locked frame store are not copied: the set points at the store
 * (the GPU reads them there) and they are copied once, into their packets,
 * at delivery.  Other pcap frames are copied into the stage (64 B aligned
 * offsets) and allocated later, directly from the final pool; loop frames
 * keep their packets in s->pk.  Returns the frame count. */
static int stage_frames(rt_pktio_t *e, rx_set_t *s, uint32_t max, uint32_t idx)
{
	uint32_t n = 0;
	size_t off = 0;

	if (stage_reserve(s, max, 0))
		return -1;
	s->base = s->stage;
	if (e->drv == DRV_PCAP) {
		/* in place only when the descriptor / record arrays are page-locked
		 * too: otherwise mi_cls stages the whole frame store every burst */
		const int in_place = e->fs_pinned && s->arr_pinned;

		if (in_place)
			s->base = e->fs.buf;
		while (n < max) {
			if (e->next >= e->fs.n) {
				if (e->fs.n == 0 || e->eof)
					break;
				/* _pcapif_reopen (pcap.c:257-278): note loop_cnt starts at 1 */
				if (e->loops != 0 && ++e->loop_cnt >= e->loops) {
					e->eof = 1;
					break;
				}
				e->next = 0;
			}
			const uint32_t fo = e->fs.off[e->next];
			const uint8_t *d = e->fs.buf + fo;
			uint16_t l = e->fs.len[e->next];

			e->next++;
			if (!pcap_filter_pass(e->promisc, d, l))
				continue;
			if (in_place) {
				s->soff[n] = fo;
			} else {
				if (stage_reserve(s, max, off + l + 64))
					return -1;
				s->base = s->stage;
				memcpy(s->stage + off, d, l);
				s->soff[n] = (uint32_t)off;
				off += ((uint32_t)l + 63u) & ~63u;
			}
			s->slen[n] = l;
			n++;
		}
		s->bytes = in_place ? e->fs.bytes : off + 64;
	} else if (e->drv == DRV_LOOP) {
		/* the receive chain stages the burst on the GPU from the packets'
		 * headers (rxc_submit): only the handles are taken here */
		const int gstage = rxc_loop_stage_ok(e, s, max);

		while (n < max) {
			odp_event_t *ev = (odp_event_t *)(void *)(s->pk + n);
			int want = (int)(max - n);
			int got = rt_queue_deq_multi_raw((rt_queue_t *)(void *)e->loopq[idx], ev, want);

			if (got <= 0)
				break;
			n += (uint32_t)got;
			if (got < want)
				break;
		}
		/* the GPU reads the headers: only of packets in page-locked pools
		 * (a packet of a pool in ordinary memory is staged by the host) */
		s->gstage = gstage && n > 0 && rt_pinned_handles(s->pk, (int)n);
		if (s->gstage) {
			uint8_t *lo = NULL;
			size_t span = 0;

			(void)rt_pinned_arena(&lo, &span);
			s->base = lo;
			s->bytes = span;
		} else if (n > 0 && loop_stage_hdrs(e, s, n)) {
			odp_packet_free_multi(s->pk, (int)n);
			return -1;
		}
	}
	return (int)n;
}

/* more frames ready at the driver right now (a burst in flight can wait) */
static int rx_more(rt_pktio_t *e, uint32_t idx)
{
	if (e->drv == DRV_PCAP)
		return e->fs.n && !e->eof &&
		       (e->next < e->fs.n || e->loops == 0 || e->loop_cnt + 1 < e->loops);
	if (e->drv == DRV_LOOP)
		return ((rt_queue_t *)(void *)e->loopq[idx])->count > 0;
	return 0;
}

static void rx_drop(rt_pktio_t *e, rx_set_t *s, int rc)
{
	RT_ERR("pktio %s: GPU classify failed (%s), burst of %d dropped\n", e->name,
	       mi_cls_strerror(rc), s->n);
	if (e->drv == DRV_LOOP)
		odp_packet_free_multi(s->pk, s->n);
	odp_atomic_add_u64(&e->in_discards, (uint64_t)s->n);
	s->pending = 0;
}

/* Classify set s: submitted to the GPU (pipelined) or done on return.  On
 * failure the burst is dropped and counted; returns 0 / -1. */
static int rx_classify(rt_pktio_t *e, rx_set_t *s, int pipe)
{
	int rc = 0;

	s->ticket = 0;
	s->pending = 1;
	if (e->parse_layer == ODP_PROTO_LAYER_NONE)
		return 0;
	s->gen = odp_amd_cls_generation();
	if (pipe)
		rc = odp_amd_cls_classify_host_submit(e->hdl, s->base, s->bytes, s->soff, s->slen,
						      (uint32_t)s->n, s->res, &s->ticket);
	else
		rc = odp_amd_cls_classify_host(e->hdl, s->base, s->bytes, s->soff, s->slen,
					       (uint32_t)s->n, s->res, !e->cls_enabled);
	if (rc) {
		rx_drop(e, s, rc);
		return -1;
	}
	return 0;
}

/* What becomes of one received frame (loop.c:311-337, pcap.c:299-352). */
typedef enum {
	RX_PARSE_DROP,    /* the parser drops it: an error */
	RX_COS_DROP,      /* its CoS drops it: no counter */
	RX_COS_DISCARD,   /* no CoS takes it (classify < 0, or back to the loop): a discard */
	RX_DELIVER        /* delivered, as a packet of *pool */
} rx_verdict_t;

/* A frame's record as the pktio's parse layer leaves it (apply_layer); at
 * layer NONE, where nothing was classified, all zero with no CoS. */
static inline void rx_record(const rt_pktio_t *e, const mi_cls_result_t *rec, mi_cls_result_t *r)
{
	if (e->parse_layer != ODP_PROTO_LAYER_NONE) {
		*r = *rec;
		apply_layer(r, e->parse_layer);
	} else {
		memset(r, 0, sizeof(*r));
		r->cos = 0xff;
	}
}

/* A burst's cache of the CoS lookups: the pool, the queue of slot 0. */
typedef struct {
	odp_pool_t pool[256];
	odp_queue_t q0[256];
	uint8_t seen[256];
} rx_cos_cache_t;

static inline void rx_cos_lookup(rx_cos_cache_t *cc, uint32_t cos)
{
	if (!cc->seen[cos]) {
		cc->seen[cos] = 1;
		cc->pool[cos] = odp_amd_cls_pool_of(cos);
		cc->q0[cos] = odp_amd_cls_queue_of(cos, 0);
	}
}

/* The verdict on a frame from its record, for every delivery path: *r is
 * rx_record's, *pool where a delivered frame's packet comes from, its CoS's
 * pool or else the pktio's (looked up through the burst's cache cc, where
 * the caller keeps one).  With the classifier off only the parser drops.
 * Nothing is counted here (rx_count). */
static inline rx_verdict_t rx_decide(const rt_pktio_t *e, const mi_cls_result_t *rec,
				     mi_cls_result_t *r, odp_pool_t *pool, rx_cos_cache_t *cc)
{
	rx_record(e, rec, r);
	if (r->outcome == MI_CLS_OUT_PARSE_DROP)
		return RX_PARSE_DROP;
	*pool = e->pool;
	if (e->cls_enabled) {
		if (r->outcome == MI_CLS_OUT_DISCARD || r->outcome == MI_CLS_OUT_LOOP)
			return RX_COS_DISCARD;
		if (r->outcome != MI_CLS_OUT_ENQ)
			return RX_COS_DROP;
		odp_pool_t cp;

		if (cc) {
			rx_cos_lookup(cc, r->cos);
			cp = cc->pool[r->cos];
		} else {
			cp = odp_amd_cls_pool_of(r->cos);
		}
		if (cp != ODP_POOL_INVALID)
			*pool = cp;
	}
	return RX_DELIVER;
}

/* The counters of a verdict: in_errors for a parse drop or any error flag of
 * the record (loop.c:311-312), in_discards for a CoS discard (loop.c:324-330;
 * the verdict exists with the classifier on only). */
static inline void rx_count(rx_verdict_t v, int err, rx_cnt_t *c)
{
	if (err || v == RX_PARSE_DROP)
		c->in_errors++;
	if (v == RX_COS_DISCARD)
		c->in_discards++;
}

/* A delivered frame found no packet (too long for its pool, or the pool ran
 * short): a discard with the classifier on (loop.c:332-337; off, the
 * reference's receive stops instead, pcap.c:324-327), and always for a loop
 * packet `had` that failed to switch pools. */
static inline void rx_count_no_packet(const rt_pktio_t *e, odp_packet_t had, rx_cnt_t *c)
{
	if (e->cls_enabled || had != ODP_PACKET_INVALID)
		c->in_discards++;
}

/* Add a delivery's counters to the pktio's. */
static inline void rx_cnt_flush(rt_pktio_t *e, const rx_cnt_t *c)
{
	if (c->in_errors)
		odp_atomic_add_u64(&e->in_errors, c->in_errors);
	if (c->in_discards)
		odp_atomic_add_u64(&e->in_discards, c->in_discards);
	odp_atomic_add_u64(&e->in_octets, c->octets);
	odp_atomic_add_u64(&e->in_packets, c->packets);
	/* and to the input queue the burst was received on (several queues: a
	 * receive call leaves no burst in flight, so it is the call's queue) */
	if (c->in_errors)
		odp_atomic_add_u64(&e->inq_st[e->rx_idx].errors, c->in_errors);
	if (c->in_discards)
		odp_atomic_add_u64(&e->inq_st[e->rx_idx].discards, c->in_discards);
	odp_atomic_add_u64(&e->inq_st[e->rx_idx].octets, c->octets);
	odp_atomic_add_u64(&e->inq_st[e->rx_idx].packets, c->packets);
}

/* Packet metadata of a delivered frame from its record. */
static inline void rx_fill(rt_pktio_t *e, pkt_hdr_t *h, const mi_cls_result_t *r, uint32_t len,
			   rx_cnt_t *c)
{
	if (e->parse_layer != ODP_PROTO_LAYER_NONE) {
		h->in_flags = r->in_flags;
		h->err = r->err;
		h->l2 = 0;
		h->l3 = r->l3_offset;
		h->l4 = r->l4_offset;
	} else {
		h->in_flags = 0;
		h->err = 0;
	}
	h->input = e->hdl;
	if (!h->err) {
		c->octets += len;
		c->packets++;
	}
	if (e->cls_enabled) {
		h->cos = r->cos;
		h->cls_mark = r->mark;
		h->dst_queue = odp_amd_cls_queue_of(r->cos, r->queue);
	}
}

/* The host steps of loopback_recv / pcapif_recv_pkt for frames [lo, hi) of
 * set s (loop.c:253-384, pcap.c:299-352; _odp_packet_parse_common's result
 * applied at the pktio's layer, _odp_cls_classify_packet's outcome, the
 * packet in its final pool, _odp_pktio_packet_to_pool): s->pk[i] becomes the
 * packet to deliver, or ODP_PACKET_INVALID.  (Preparing chunks of a burst on
 * helper threads measured slower -- 14.3 -> 6.4 Mpkt/s with four helpers,
 * profiles/r03g_rx_helpers_ab.txt: each packet's header line then moves between cores
 * on its way to the queue and the consumer -- so one thread does it.) */
static void rx_prepare_each(rt_pktio_t *e, rx_set_t *s, int lo, int hi, rx_cnt_t *c)
{
	for (int i = lo; i < hi; i++) {
		mi_cls_result_t r;
		odp_packet_t pkt = e->drv == DRV_LOOP ? s->pk[i] : ODP_PACKET_INVALID;
		uint32_t len = s->slen[i];

		s->pk[i] = ODP_PACKET_INVALID;
		if (i + 16 < hi)    /* records written by the GPU: not in the CPU caches */
			__builtin_prefetch(&s->res[i + 16]);
		if (i + 8 < hi) {   /* frames read in place are cold in the CPU caches */
			const uint8_t *nf = s->base + s->soff[i + 8];
			const uint32_t nl = s->slen[i + 8];

			for (uint32_t b = 0; b < nl; b += 64)
				__builtin_prefetch(nf + b);
		}
		odp_pool_t pool;
		const rx_verdict_t v = rx_decide(e, &s->res[i], &r, &pool, NULL);

		rx_count(v, r.err, c);
		if (v != RX_DELIVER) {
			odp_packet_free(pkt);
			continue;
		}
		/* packet in the final pool (_odp_pktio_packet_to_pool) */
		if (pkt == ODP_PACKET_INVALID) {
			const uint64_t ta = rx_prof > 0 ? __rdtsc() : 0;

			pkt = odp_packet_alloc(pool, len);
			if (pkt == ODP_PACKET_INVALID) {
				rx_count_no_packet(e, pkt, c);
				continue;
			}
			const uint64_t tb = rx_prof > 0 ? __rdtsc() : 0;

			memcpy(odp_packet_data(pkt), s->base + s->soff[i], len);
			if (rx_prof > 0) {
				e->prof[6] += tb - ta;
				e->prof[7] += __rdtsc() - tb;
			}
		} else if (odp_packet_pool(pkt) != pool) {
			odp_packet_t np = odp_packet_alloc(pool, len);

			if (np == ODP_PACKET_INVALID) {
				rx_count_no_packet(e, pkt, c);
				odp_packet_free(pkt);
				continue;
			}
			pkt_hdr_t *sh = rt_pkt_hdr(pkt);

			memcpy(odp_packet_data(np), sh->head + sh->data_off, len);
			rt_pkt_hdr(np)->user_ptr = sh->user_ptr;
			odp_packet_free(pkt);
			pkt = np;
		} else {
			/* a loop packet delivered in place: packet_parse_reset(.., 1)
			 * (loop.c:308), a received packet carries no pktout checksum
			 * or LSO overrides (a fresh packet has none, pkt_init; the GPU
			 * deliveries write the whole metadata block, these as 0) */
			pkt_hdr_t *h = rt_pkt_hdr(pkt);

			h->tx_ck = 0;
			h->payload_off = 0;
			h->lso_flags = 0;
			h->lso_prof = 0;
			h->lso_max_payload = 0;
		}
		rx_fill(e, rt_pkt_hdr(pkt), &r, len, c);
		s->pk[i] = pkt;
	}
}

/* A set's delivery scratch (s->tmp): n_cap packets -- those taken from the
 * pools in bulk, then a queue group's -- followed by one byte per frame -- its
 * pool bucket or verdict, then its queue group, then a group's CoS values.
 * rx_tmp_bytes is NULL when there is none. */
static void rx_tmp_ensure(rx_set_t *s)
{
	if (!s->tmp || s->tmp_cap < s->n_cap) {
		free(s->tmp);
		s->tmp = malloc(s->n_cap * (sizeof(odp_packet_t) + 1u));
		s->tmp_cap = s->tmp ? s->n_cap : 0;
	}
}

static inline uint8_t *rx_tmp_bytes(const rx_set_t *s)
{
	return s->tmp ? (uint8_t *)(void *)(s->tmp + s->tmp_cap) : NULL;
}

/* The pool buckets of a burst delivered in passes (rx_prepare, rx_dlv_start):
 * pass 1 finds each delivered frame's bucket and counts it in, pass 2 takes
 * every bucket's packets from its pool at once, pass 3 hands them out.
 * Frames of one pool get their packets in arrival order, so when a pool runs
 * short the same frames go without as frame-by-frame allocation would leave
 * (pktio/loop.c:332-337); every frame counted in asks for its packet, so
 * none taken is left over. */
#define RX_MAX_POOLS 16
typedef struct {
	odp_pool_t pool;
	uint32_t cap;   /* longest frame a packet of it holds (0: not a packet pool) */
	int pinned;     /* page-locked */
	int cnt;        /* frames counted in */
	int base, have; /* its packets: got[base .. base + have) */
	int used;       /* asked for so far */
} rx_bucket_t;

typedef struct {
	rx_bucket_t b[RX_MAX_POOLS];
	int n;
} rx_buckets_t;

/* Bucket of a pool, added when new; -1 when all RX_MAX_POOLS are other
 * pools' (the caller falls back). */
static inline int rx_bucket_of(rx_buckets_t *bk, odp_pool_t pool)
{
	int k = 0;

	while (k < bk->n && bk->b[k].pool != pool)
		k++;
	if (k == bk->n) {
		const rt_pool_t *rp = rt_pool(pool);

		if (k == RX_MAX_POOLS)
			return -1;
		bk->b[k].pool = pool;
		bk->b[k].cap = rp && rp->param.type == ODP_POOL_PACKET ? rp->data_cap : 0u;
		bk->b[k].pinned = rp && rp->pinned;
		bk->b[k].cnt = 0;
		bk->n++;
	}
	return k;
}

/* Take every bucket's packets at once, into got[at ...). */
static inline void rx_buckets_take(rx_buckets_t *bk, odp_packet_t got[], int at)
{
	for (int k = 0; k < bk->n; k++) {
		rx_bucket_t *b = &bk->b[k];

		b->base = at;
		b->have = b->cnt ? rt_packet_alloc_raw(b->pool, 0, &got[at], b->cnt) : 0;
		b->used = 0;
		at += b->cnt;
	}
}

/* The next packet of a bucket, ODP_PACKET_INVALID when its pool ran short. */
static inline odp_packet_t rx_bucket_next(rx_bucket_t *b, const odp_packet_t got[])
{
	const int j = b->used++;

	return j < b->have ? got[b->base + j] : ODP_PACKET_INVALID;
}

/* rx_prepare for pcap frames: the same steps in three passes, so packets
 * are taken from each pool in bulk and their headers prefetched before they
 * are written (a per-frame odp_packet_alloc spent most of its time on the
 * cold header line).  Pass 1 decides each frame (rx_decide) and counts it
 * into its pool's bucket, pass 2 takes the buckets' packets, and pass 3
 * initialises the headers, copies the frames and writes the metadata.
 * `slot` (one byte per frame) and `got` (n_cap packets) are the set's
 * delivery scratch; more than RX_MAX_POOLS distinct pools in a burst fall
 * back to rx_prepare_each. */
static void rx_prepare(rt_pktio_t *e, rx_set_t *s, int lo, int hi, rx_cnt_t *c)
{
	uint8_t *slot = rx_tmp_bytes(s);
	odp_packet_t *got = s->tmp;
	rx_buckets_t bk;

	if (e->drv != DRV_PCAP || !slot) {
		rx_prepare_each(e, s, lo, hi, c);
		return;
	}
	bk.n = 0;
	/* pass 1: the decision per frame */
	for (int i = lo; i < hi; i++) {
		if (i + 16 < hi)
			__builtin_prefetch(&s->res[i + 16]);
		mi_cls_result_t r;
		odp_pool_t pool;
		const rx_verdict_t v = rx_decide(e, &s->res[i], &r, &pool, NULL);

		s->pk[i] = ODP_PACKET_INVALID;
		slot[i] = 0xff;
		rx_count(v, r.err, c);
		if (v != RX_DELIVER)
			continue;
		const int k = rx_bucket_of(&bk, pool);

		if (k < 0) {   /* start over frame by frame */
			memset(c, 0, sizeof(*c));
			rx_prepare_each(e, s, lo, hi, c);
			return;
		}
		if (s->slen[i] > bk.b[k].cap) {   /* odp_packet_alloc fails: no packet taken */
			rx_count_no_packet(e, ODP_PACKET_INVALID, c);
			continue;
		}
		slot[i] = (uint8_t)k;
		bk.b[k].cnt++;
	}
	/* pass 2: each pool's packets at once */
	rx_buckets_take(&bk, got, lo);
	/* pass 3: headers, frames, metadata */
	for (int i = lo; i < hi; i++) {
		if (i + 8 < hi) {   /* frames read in place are cold in the CPU caches */
			const uint8_t *nf = s->base + s->soff[i + 8];
			const uint32_t nl = s->slen[i + 8];

			for (uint32_t b = 0; b < nl; b += 64)
				__builtin_prefetch(nf + b);
		}
		if (slot[i] == 0xff)
			continue;
		rx_bucket_t *b = &bk.b[slot[i]];
		const odp_packet_t pkt = rx_bucket_next(b, got);

		if (pkt == ODP_PACKET_INVALID) {   /* the pool ran short */
			rx_count_no_packet(e, ODP_PACKET_INVALID, c);
			continue;
		}
		if (b->used + 3 < b->have) {   /* a later packet of this pool: its header */
			const pkt_hdr_t *nh = rt_pkt_hdr(got[b->base + b->used + 3]);

			/* the buffer follows the 64-B aligned header (odp_rt.c pool
			 * layout): its first data line, without reading the header */
			__builtin_prefetch(nh, 1);
			__builtin_prefetch((const uint8_t *)nh + ((sizeof(pkt_hdr_t) + 63u) & ~(size_t)63u) +
					   RT_PKT_HEADROOM, 1);
		}
		const uint32_t len = s->slen[i];
		mi_cls_result_t r;

		rx_record(e, &s->res[i], &r);
		const uint64_t ta = rx_prof > 0 ? __rdtsc() : 0;

		rt_packet_init(pkt, len);
		const uint64_t tb = rx_prof > 0 ? __rdtsc() : 0;

		memcpy(odp_packet_data(pkt), s->base + s->soff[i], len);
		if (rx_prof > 0) {
			e->prof[6] += tb - ta;
			e->prof[7] += __rdtsc() - tb;
		}
		rx_fill(e, rt_pkt_hdr(pkt), &r, len, c);
		s->pk[i] = pkt;
	}
}

/* Classifier off: the delivered packets pk[0..n) go to the caller's out[]
 * (at most max_out, the rest are freed).  Returns how many it got. */
static inline int rx_to_caller(const odp_packet_t pk[], int n, odp_packet_t out[], int max_out)
{
	const int num_rx = n < max_out ? n : (max_out > 0 ? max_out : 0);

	if (num_rx)
		memcpy(out, pk, (size_t)num_rx * sizeof(odp_packet_t));
	odp_packet_free_multi(&pk[num_rx], n - num_rx);
	return num_rx;
}

/* Enqueue the delivered packets pk[0..n) of set s in arrival order.  _odp_cls_enq
 * (odp_classification_internal.h:171-201) enqueues runs of equal
 * (dst_queue, CoS); when every run of the burst takes the plain enqueue (no
 * packet vectors, no aggregator), the runs of one queue are joined into one
 * enqueue call per queue instead -- each queue still receives its packets in
 * arrival order, and nothing outside the burst can tell the two apart (the
 * whole burst is enqueued before the receive call returns).  Per-CoS queue
 * statistics are kept as per run.  Runs of CoS with packet vectors or
 * aggregators keep the reference's per-run form (their vector boundaries
 * depend on it). */
static void rx_enqueue(rx_set_t *s, odp_packet_t pk[], int n)
{
	odp_packet_t *tmp = s->tmp;
	uint8_t *gidx = rx_tmp_bytes(s);
	rx_qgroups_t g;
	int cnt[RX_GROUP_MAXQ], fill[RX_GROUP_MAXQ];
	int plain = 1;
	int8_t mode_of_cos[256];

	if (!tmp) {   /* no scratch to sort in: packet by packet */
		for (int i = 0; i < n; i++)
			cos_enq_run(&pk[i], 1);
		return;
	}
	memset(mode_of_cos, -1, sizeof(mode_of_cos));
	memset(g.slot, 0, sizeof(g.slot));
	g.n = 0;
	for (int i = 0; i < n; i++) {
		const pkt_hdr_t *h = rt_pkt_hdr(pk[i]);
		const int known = g.n;
		const int k = rx_cos_plain(mode_of_cos, h->cos & 0xffu) ? rx_qgroup_of(&g, h->dst_queue) : -1;

		if (k < 0) {   /* vectors, an aggregator, or more than RX_GROUP_MAXQ queues */
			plain = 0;
			break;
		}
		if (k == known)
			cnt[k] = 0;
		gidx[i] = (uint8_t)k;
		cnt[k]++;
	}
	if (!plain) {
		/* the reference's form: one enqueue per run */
		int nrun = 0;

		for (int i = 0; i < n; i++) {
			if (nrun) {
				pkt_hdr_t *ph = rt_pkt_hdr(pk[i - 1]), *h = rt_pkt_hdr(pk[i]);

				if (ph->dst_queue != h->dst_queue || ph->cos != h->cos) {
					cos_enq_run(&pk[i - nrun], nrun);
					nrun = 0;
				}
			}
			nrun++;
		}
		if (nrun)
			cos_enq_run(&pk[n - nrun], nrun);
		return;
	}
	/* counting sort by queue, stable: each group's packets in arrival order */
	int at = 0;

	for (int k = 0; k < g.n; k++) {
		fill[k] = at;
		at += cnt[k];
	}
	for (int i = 0; i < n; i++)
		tmp[fill[gidx[i]]++] = pk[i];
	/* (the group bytes are done with: each group's CoS values go there) */
	at = 0;
	for (int k = 0; k < g.n; k++) {
		odp_packet_t *gp = tmp + at;

		for (int j = 0; j < cnt[k]; j++)
			gidx[j] = (uint8_t)rt_pkt_hdr(gp[j])->cos;
		rx_enq_group(g.q[k], gp, gidx, cnt[k]);
		at += cnt[k];
	}
}

/* Enqueue the grouped packets of a GPU delivery: group g (queue gq[g]) holds
 * entries perm[at .. at + gcnt[g]) in arrival order. */
static void rx_enqueue_groups(rx_set_t *s)
{
	uint8_t *cos = rx_tmp_bytes(s);
	uint32_t at = 0;

	for (int g = 0; g < s->ng; g++) {
		const uint32_t num = s->gcnt[g];

		if (!num)
			continue;
		for (uint32_t k = 0; k < num; k++) {
			const uint32_t j = s->perm[at + k];

			s->tmp[k] = s->ent[j];
			cos[k] = s->res[s->dlv[j].rec].cos;
		}
		rx_enq_group(s->gq[g], s->tmp, cos, (int)num);
		at += num;
	}
}

/* Delivery of set s on the GPU (mi_cls_deliver_submit): the host decides
 * every frame from its record (parse drop, CoS drop / discard, destination
 * pool: the same decisions and counters as rx_prepare), takes the packets
 * from each pool at once, and hands the GPU one entry per delivered packet;
 * the GPU writes the packets' metadata, copies frames that change buffers
 * (pcap frames, loop packets switching pools) and groups the packets by
 * queue; the host then enqueues each queue's packets with one call.  The
 * host touches no packet header or frame byte on this path.  This starts
 * it: the decisions, the packets, the entries, the kernel submitted (the set
 * is then `delivering` until rx_dlv_end).  Returns 0, or -1 when the burst
 * needs the host path (a destination pool not page-locked, more than
 * RX_MAX_POOLS pools, frames the GPU cannot address) -- nothing has been
 * done then. */
_Static_assert(RX_GROUP_MAXQ <= MI_CLS_DLV_GROUPS && RX_MAX_POOLS <= 0x10, "delivery codes");
static int rx_dlv_start(rt_pktio_t *e, rx_set_t *s, rx_cnt_t *c)
{
	const odp_proto_layer_t layer = e->parse_layer;
	uint8_t *slot = rx_tmp_bytes(s);
	odp_packet_t *got = s->tmp;
	rx_buckets_t bk;
	/* a frame's byte from pass 1 to pass 3: the bucket of its pool, or */
	enum {
		A_INPLACE = 0x10,   /* a loop packet stays in its own buffer */
		A_TOO_LONG,         /* longer than a packet of its pool: no packet */
		A_VERDICT = 0x20,   /* + its rx_verdict_t: not delivered */
		A_ERR = 0x80        /* with any of them: the record has error flags */
	};

	if (!gpu_deliver_on() || !s->dlv_pinned || !slot || layer == ODP_PROTO_LAYER_NONE ||
	    !mi_cls_host_mapped(s->base))
		return -1;
	const uint64_t td0 = prof_ns();
	s->dgen = odp_amd_cls_generation();
	/* pass 1: the decision per frame, no side effects yet */
	rx_cos_cache_t cc;

	memset(cc.seen, 0, sizeof(cc.seen));
	bk.n = 0;
	for (int i = 0; i < s->n; i++) {
		mi_cls_result_t r;
		odp_pool_t pool;
		uint8_t a;

		if (i + 16 < s->n)
			__builtin_prefetch(&s->res[i + 16]);
		const rx_verdict_t v = rx_decide(e, &s->res[i], &r, &pool, &cc);

		if (v != RX_DELIVER) {
			a = (uint8_t)(A_VERDICT + v);
		} else if (e->drv == DRV_LOOP && (odp_pool_t)(uintptr_t)s->ppool[i] == pool) {
			/* the GPU writes the packet's own header */
			if (!rt_pool(pool)->pinned)
				return -1;
			a = A_INPLACE;
		} else {
			const int k = rx_bucket_of(&bk, pool);

			if (k < 0 || !bk.b[k].pinned)
				return -1;
			if (s->slen[i] > bk.b[k].cap) {   /* odp_packet_alloc fails */
				a = A_TOO_LONG;
			} else {
				a = (uint8_t)k;
				bk.b[k].cnt++;
			}
		}
		slot[i] = r.err ? a | A_ERR : a;
	}
	/* pass 2: each pool's packets at once */
	rx_buckets_take(&bk, got, 0);
	/* pass 3: counters, drops, entries (queue groups: every plain-enqueue
	 * queue of the burst, at most MI_CLS_DLV_GROUPS) */
	rx_qgroups_t g;
	int grouped = e->cls_enabled, nold = 0;
	int8_t mode_of_cos[256];
	uint32_t ne = 0;

	memset(mode_of_cos, -1, sizeof(mode_of_cos));
	memset(g.slot, 0, sizeof(g.slot));
	g.n = 0;
	for (int i = 0; i < s->n; i++) {
		const mi_cls_result_t *rec = &s->res[i];   /* (its CoS and queue: any layer's) */
		const uint32_t len = s->slen[i];
		const int a = slot[i] & ~A_ERR, err = slot[i] & A_ERR;
		odp_packet_t pkt = e->drv == DRV_LOOP ? s->pk[i] : ODP_PACKET_INVALID;

		s->pk[i] = ODP_PACKET_INVALID;
		rx_count(a >= A_VERDICT ? (rx_verdict_t)(a - A_VERDICT) : RX_DELIVER, err, c);
		if (a >= A_VERDICT) {
			odp_packet_free(pkt);
			continue;
		}
		uint8_t fl = MI_CLS_DLV_FRESH | MI_CLS_DLV_COPY;
		odp_packet_t dst;

		if (a == A_INPLACE) {
			dst = pkt;
			fl = 0;
		} else {
			dst = a == A_TOO_LONG ? ODP_PACKET_INVALID : rx_bucket_next(&bk.b[a], got);
			if (dst == ODP_PACKET_INVALID) {   /* too long, or the pool ran short */
				rx_count_no_packet(e, pkt, c);
				odp_packet_free(pkt);
				continue;
			}
			if (pkt != ODP_PACKET_INVALID)
				s->old[nold++] = pkt;   /* freed once the GPU copied it */
		}
		if (!err) {
			c->octets += len;
			c->packets++;
		}
		mi_cls_dlv_t *d = &s->dlv[ne];
		uint8_t qid = 0xff;

		d->meta = (uint64_t)(uintptr_t)&rt_pkt_hdr(dst)->meta;
		d->data_off = a == A_INPLACE ? s->pdoff[i] : RT_PKT_HEADROOM;
		/* the metadata line is written whole: a packet received in place
		 * keeps its user pointer (read with its headroom at staging) */
		d->user_ptr = a == A_INPLACE ? (uint64_t)(uintptr_t)s->pup[i] : 0u;
		d->dst_queue = 0;
		d->src = s->soff[i];
		d->rec = (uint32_t)i;
		d->len = (uint16_t)len;
		if (e->cls_enabled) {
			const odp_queue_t q = rec->queue == 0 ? cc.q0[rec->cos]
				: odp_amd_cls_queue_of(rec->cos, rec->queue);

			fl |= MI_CLS_DLV_CLS;
			d->dst_queue = (uint64_t)(uintptr_t)q;
			if (grouped && rx_cos_plain(mode_of_cos, rec->cos)) {
				const int k = rx_qgroup_of(&g, q);

				if (k < 0)
					grouped = 0;
				else
					qid = (uint8_t)k;
			} else {
				grouped = 0;
			}
		}
		d->flags = fl;
		d->qid = qid;
		s->ent[ne++] = dst;
	}
	if (ne > MI_CLS_DLV_GROUP_MAX)   /* larger than the device grouping serves */
		grouped = 0;
	if (!grouped)   /* per-run enqueue (vectors, aggregators, > 64 queues) */
		for (uint32_t j = 0; j < ne; j++)
			s->dlv[j].qid = 0xff;
	s->ne = ne;
	s->nold = nold;
	s->grouped = grouped;
	s->ng = g.n;
	memcpy(s->gq, g.q, (size_t)g.n * sizeof(odp_queue_t));
	s->cnt = *c;
	s->dticket = 0;
	s->delivering = 1;
	e->prof[8] += prof_ns() - td0;
	e->prof[11]++;
	if (ne) {
		mi_cls_dlv_args_t a;

		a.base = s->base;
		a.res = s->res;
		a.dlv = s->dlv;
		a.n = ne;
		a.layer = (uint32_t)layer;
		a.input = (uint64_t)(uintptr_t)e->hdl;
		a.headroom = RT_PKT_HEADROOM;
		a.data_from_meta = rt_data_from_meta();
		a.perm = s->perm;
		a.gcnt = s->gcnt;
		s->dticket = 0;
		const uint64_t ts0 = prof_ns();
		int rc = odp_amd_cls_deliver(e->hdl, &a, &s->dticket);

		e->prof[12] += prof_ns() - ts0;

		if (rc) {
			s->dticket = 0;
			s->derr = rc;   /* rx_dlv_end drops the packets */
		}
	}
	return 0;
}

/* The control plane changed while set s's GPU delivery was in flight: its
 * packets' CoS, queues and pools were settled under the old tables, and a
 * queue destroyed since may have had its slot reused by a new one.  The burst
 * is classified again under the current tables and each delivered packet
 * re-resolved from its new record: a packet whose outcome is no longer an
 * enqueue is freed (CoS discards counted, and it leaves in_packets /
 * in_octets), one whose CoS pool changed is copied into that pool, and every
 * packet takes its CoS, mark and queue from the new record.  The burst is then
 * enqueued per run.  Frames the old rules dropped or discarded stay dropped:
 * their packets were freed when the delivery started, so a frame that the new
 * rules would enqueue is not recovered.  That is within the reference's
 * contract for packets in flight during a rule change, whose classification
 * is indeterminate (odp_classification.c:1373-1374); it is not the result of
 * a receive call made wholly after the change. */
static void rx_dlv_regen(rt_pktio_t *e, rx_set_t *s, rx_cnt_t *c)
{
	uint32_t m = 0;
	int rc = odp_amd_cls_classify_host(e->hdl, s->base, s->bytes, s->soff, s->slen, (uint32_t)s->n,
					   s->res, 0);

	s->grouped = 0;
	if (rc) {
		RT_ERR("pktio %s: GPU classify failed (%s), %u packets dropped\n", e->name,
		       mi_cls_strerror(rc), s->ne);
		odp_packet_free_multi(s->ent, (int)s->ne);
		c->in_discards += s->ne;
		s->ne = 0;
		return;
	}
	for (uint32_t j = 0; j < s->ne; j++) {
		odp_packet_t pkt = s->ent[j];
		mi_cls_result_t r;
		odp_pool_t pool;
		const uint32_t len = s->dlv[j].len;
		const rx_verdict_t v = rx_decide(e, &s->res[s->dlv[j].rec], &r, &pool, NULL);

		if (v != RX_DELIVER) {
			/* (its error flags were counted when the delivery started) */
			if (v == RX_COS_DISCARD)
				c->in_discards++;
			if (!r.err) {
				c->packets--;
				c->octets -= len;
			}
			odp_packet_free(pkt);
			continue;
		}
		if (odp_packet_pool(pkt) != pool) {
			/* _odp_pktio_packet_to_pool under the new CoS */
			odp_packet_t np = odp_packet_alloc(pool, len);

			if (np == ODP_PACKET_INVALID) {
				c->in_discards++;
				if (!r.err) {
					c->packets--;
					c->octets -= len;
				}
				odp_packet_free(pkt);
				continue;
			}
			pkt_hdr_t *oh = rt_pkt_hdr(pkt), *nh = rt_pkt_hdr(np);

			memcpy(odp_packet_data(np), oh->head + oh->data_off, len);
			nh->in_flags = oh->in_flags;
			nh->err = oh->err;
			nh->l2 = oh->l2;
			nh->l3 = oh->l3;
			nh->l4 = oh->l4;
			nh->input = oh->input;
			nh->user_ptr = oh->user_ptr;
			odp_packet_free(pkt);
			pkt = np;
		}
		pkt_hdr_t *h = rt_pkt_hdr(pkt);

		h->in_flags = r.in_flags;
		h->cos = r.cos;
		h->cls_mark = r.mark;
		h->dst_queue = odp_amd_cls_queue_of(r.cos, r.queue);
		s->ent[m++] = pkt;
	}
	s->ne = m;
}

/* End the GPU delivery of set s (rx_dlv_start): wait for the kernel, give
 * pool-switched packets their user pointers, enqueue (classifier on) or
 * return the packets in out[] (at most max_out), add the counters.
 * Returns the packets placed in out[]. */
static int rxc_end(rt_pktio_t *e, rx_set_t *s, odp_packet_t out[], int max_out);

static int rx_dlv_end(rt_pktio_t *e, rx_set_t *s, odp_packet_t out[], int max_out)
{
	if (s->chain)
		return rxc_end(e, s, out, max_out);
	const uint64_t tk0 = prof_ns();
	rx_cnt_t *c = &s->cnt;
	int num_rx = 0, rc = s->derr;

	if (!rc && s->dticket)
		rc = odp_amd_cls_deliver_wait(e->hdl, s->dticket);
	s->delivering = 0;
	s->dticket = 0;
	s->derr = 0;
	if (rc) {
		RT_ERR("pktio %s: GPU delivery failed (%s), %u packets dropped\n", e->name,
		       mi_cls_strerror(rc), s->ne);
		odp_packet_free_multi(s->ent, (int)s->ne);
		odp_packet_free_multi(s->old, s->nold);
		c->in_discards += s->ne;
		s->ne = 0;
		s->nold = 0;
	}
	/* pool switch: the new packet keeps the user pointer */
	if (s->nold) {
		int o = 0;

		for (uint32_t j = 0; j < s->ne && o < s->nold; j++)
			if (s->dlv[j].flags & MI_CLS_DLV_FRESH)
				rt_pkt_hdr(s->ent[j])->user_ptr = rt_pkt_hdr(s->old[o++])->user_ptr;
		odp_packet_free_multi(s->old, s->nold);
		s->nold = 0;
	}
	if (e->cls_enabled && s->ne && s->dgen != odp_amd_cls_generation())
		rx_dlv_regen(e, s, c);
	const uint64_t tk1 = prof_ns();

	if (!e->cls_enabled)
		num_rx = rx_to_caller(s->ent, (int)s->ne, out, max_out);
	else if (s->grouped)
		rx_enqueue_groups(s);
	else if (s->ne)
		rx_enqueue(s, s->ent, (int)s->ne);
	s->ne = 0;
	e->prof[9] += tk1 - tk0;
	e->prof[10] += prof_ns() - tk1;
	rx_cnt_flush(e, c);
	return num_rx;
}

/* Delivery of set s on the host (the burst needs the host path): rx_prepare,
 * then the delivered packets, compacted in arrival order, to their queues or
 * out[]; the counters added.  t2: when the delivery began. */
static int rx_deliver_host(rt_pktio_t *e, rx_set_t *s, rx_cnt_t *c, odp_packet_t out[], int max_out,
			   uint64_t t2)
{
	int nd = 0, num_rx = 0;

	rx_prepare(e, s, 0, s->n, c);
	const uint64_t t3 = prof_ns();

	e->prof[4] += t3 - t2;
	for (int i = 0; i < s->n; i++)
		if (s->pk[i] != ODP_PACKET_INVALID)
			s->pk[nd++] = s->pk[i];
	if (e->cls_enabled)
		rx_enqueue(s, s->pk, nd);
	else
		num_rx = rx_to_caller(s->pk, nd, out, max_out);
	const uint64_t t4 = prof_ns();

	e->prof[5] += t4 - t3;
	e->prof[2] += t4 - t2;
	rx_cnt_flush(e, c);
	return num_rx;
}

/* Wait for set s's classification; a burst that was in flight while the
 * control plane changed is classified again.  Returns 0, or -1 when the
 * burst was dropped (rx_drop). */
static int rx_classified(rt_pktio_t *e, rx_set_t *s)
{
	const odp_proto_layer_t layer = e->parse_layer;
	uint64_t t1 = prof_ns();

	if (s->ticket) {
		int rc = odp_amd_cls_classify_host_wait(e->hdl, s->ticket);

		s->ticket = 0;
		if (rc) {
			rx_drop(e, s, rc);
			return -1;
		}
	}
	/* The control plane changed while the burst was in flight (a CoS
	 * destroyed, its queues or pool changed, PMRs added or removed): its
	 * records name CoS indexes of the old rule snapshot, so classify it again
	 * under the current one -- what the synchronous path, which has no gap
	 * between classify and enqueue, would deliver on this call. */
	if (layer != ODP_PROTO_LAYER_NONE && e->cls_enabled && s->gen != odp_amd_cls_generation()) {
		int rc = odp_amd_cls_classify_host(e->hdl, s->base, s->bytes, s->soff, s->slen,
						   (uint32_t)s->n, s->res, 0);

		if (rc) {
			rx_drop(e, s, rc);
			return -1;
		}
	}
	e->prof[1] += prof_ns() - t1;
	s->pending = 0;
	rx_tmp_ensure(s);
	return 0;
}

/* Wait for set s's records and deliver its packets now: classified ones to
 * their CoS queues, the rest (classifier disabled) into out[] (at most
 * max_out).  Returns the packets placed in out[]. */
static int rx_finish(rt_pktio_t *e, rx_set_t *s, odp_packet_t out[], int max_out)
{
	rx_cnt_t c;

	if (rx_classified(e, s))
		return 0;
	const uint64_t t2 = prof_ns();

	memset(&c, 0, sizeof(c));
	if (rx_dlv_start(e, s, &c) == 0) {
		const int num_rx = rx_dlv_end(e, s, out, max_out);

		e->prof[2] += prof_ns() - t2;
		return num_rx;
	}
	return rx_deliver_host(e, s, &c, out, max_out, t2);
}

/* Set of age k: staged k calls ago (age 0: this call). */
static rx_set_t *rx_age(rt_pktio_t *e, int k)
{
	return &e->rs[(e->cur + RX_SETS - k) % RX_SETS];
}

/* Classifier on: wait for set s's records and start its GPU delivery,
 * leaving it in flight (rx_dlv_end on a later call); a burst that needs the
 * host path is delivered now. */
static void rx_finish_start(rt_pktio_t *e, rx_set_t *s)
{
	rx_cnt_t c;

	if (rx_classified(e, s))
		return;
	const uint64_t t2 = prof_ns();

	memset(&c, 0, sizeof(c));
	if (rx_dlv_start(e, s, &c) == 0) {
		e->prof[2] += prof_ns() - t2;
		return;
	}
	/* the host path delivers s now: every older burst still in its GPU
	 * delivery is enqueued first, oldest first (arrival order per queue) */
	for (int k = RX_SETS - 1; k > RX_CLS_DEPTH; k--) {
		rx_set_t *b = rx_age(e, k);

		if (b->delivering)
			(void)rx_dlv_end(e, b, NULL, 0);
	}
	(void)rx_deliver_host(e, s, &c, NULL, 0, t2);
}

/* ------------------------------------------------------- receive chain
 * One submission per burst (mi_cls_rx_chain_submit): the classification,
 * the per-frame decisions of rx_dlv_start (parse drop, CoS drop / discard,
 * destination pool, too long for its pool, queue group) and the delivery
 * run on the GPU one after the other, with no host step between them.  The
 * packets the frames go into are taken from the pools before the submit (as
 * many per pool as the previous bursts used, plus a margin); a burst that
 * needs more of a pool than it was given is delivered again on the host
 * (rxc_end), so every outcome stays the reference's
 * (pktio/loop.c:253-384, pcap.c:299-352).  ODP_AMD_RX_CHAIN=0 turns it off.
 * (Its switch and its table, rx_chain_on and rxc_table, stand above the
 * staging, which asks whether a loop burst will take the chain.) */

/* A burst that does not take the chain, or leaves it for the host path
 * (rxc_end): a loop burst left for the GPU to stage is staged by the host now
 * (the classic path reads its descriptors); one that cannot be is dropped
 * and counted, s->n then 0.  Returns 0, rxc_submit's "not chained". */
static int rxc_no(rt_pktio_t *e, rx_set_t *s)
{
	if (s->gstage) {
		s->gstage = 0;
		if (loop_stage_hdrs(e, s, (uint32_t)s->n)) {
			rx_drop(e, s, -ENOMEM);
			s->n = 0;
		}
	}
	return 0;
}

/* Every packet taken for set s's chain, back to its pool. */
static void rxc_return(rx_set_t *s)
{
	for (int j = 0; j < s->nsl; j++)
		for (uint32_t k = 0; k < s->cnp; k++)
			if (s->chave[j][k])
				rt_packet_return_raw(s->cpool[k],
						     (const odp_packet_t *)(const void *)(s->got + s->cbase[j][k]),
						     (int)s->chave[j][k]);
	memset(s->chave, 0, sizeof(s->chave));
}

/* Wait for set s's chain slices [0, nj); the first failure. */
static int rxc_wait(rt_pktio_t *e, rx_set_t *s, int nj)
{
	int rc = 0;

	for (int j = 0; j < nj; j++) {
		const int r = odp_amd_cls_deliver_wait_dev(e->hdl, (uint32_t)j, s->sl_tk[j]);

		s->sl_tk[j] = 0;
		if (r && !rc)
			rc = r;
	}
	return rc;
}

/* Submit set s's burst as a chain: 1, or 0 when it takes the other path
 * (nothing done then, but for rxc_no's staging). */
static int rxc_submit(rt_pktio_t *e, rx_set_t *s)
{
	const uint32_t n = (uint32_t)s->n;

	if (!rx_chain_on() || !gpu_deliver_on() || !e->cls_enabled || e->parse_layer != ODP_PROTO_LAYER_ALL ||
	    !s->rxc_pinned || !s->dlv_pinned || !s->arr_pinned || n == 0 || n > MI_CLS_DLV_GROUP_MAX ||
	    (e->drv == DRV_LOOP && !s->pk_pinned) || !mi_cls_host_mapped(s->base) || rxc_table(e))
		return rxc_no(e, s);
	if (e->drv == DRV_LOOP && !s->gstage) {
		/* the GPU reads the loop packets' metadata (a pool switch takes the
		 * old packet's user pointer): every packet in a page-locked pool
		 * (checked by address for a GPU-staged burst, by pool here) */
		for (uint32_t i = 0; i < n; i++)
			if (!s->ppool[i] || !e->rxtab->rt_pinned[(s->ppool[i] - 1u) & 63u])
				return rxc_no(e, s);
	}
	/* slices: one per device of the pktio, contiguous, in device order (so
	 * enqueueing them in order keeps every queue's arrival order,
	 * odp_classification_internal.h:208-236) */
	int nsl = odp_amd_cls_devices(e->hdl);

	if (nsl < 1)
		nsl = 1;
	if (nsl > RX_SLICES)
		nsl = RX_SLICES;
	if ((uint32_t)nsl > n)
		nsl = (int)n;
	s->nsl = nsl;
	for (int j = 0; j <= nsl; j++)
		s->sl_lo[j] = (uint32_t)((uint64_t)n * (uint32_t)j / (uint32_t)nsl);
	/* the packets of each pool slot, per slice, in the order its frames
	 * take them */
	uint32_t at = 0;

	memset(s->cbase, 0, sizeof(s->cbase));
	memset(s->chave, 0, sizeof(s->chave));
	s->cnp = e->rx_np;
	for (uint32_t k = 0; k < s->cnp; k++)
		s->cpool[k] = e->rx_pools[k];
	for (int j = 0; j < nsl; j++) {
		const uint32_t ns = s->sl_lo[j + 1] - s->sl_lo[j];

		for (uint32_t k = 0; k < s->cnp; k++) {
			/* the last bursts' need of the slot, this slice's share (a
			 * little more when the burst is split) */
			uint32_t want = e->rx_want[k] ?
				(uint32_t)(((uint64_t)e->rx_want[k] * ns + n - 1u) / n) + (nsl > 1 ? 8u : 0u) : ns;

			if (want > ns)
				want = ns;
			if (at + want > s->got_cap)
				want = s->got_cap - at;
			/* Packets are taken before the GPU decides, up to RX_SETS - 1
			 * bursts ahead, each with a margin.  With several pool slots a
			 * slot's take is a prediction and can fall short: the take then
			 * leaves a burst's worth (n) in the pool, so a burst that comes
			 * back short and is redone on the host (rxc_end) still finds
			 * packets that younger chains hold only speculatively; a take
			 * cut by this cap comes back short itself and is delivered by the
			 * host path, which allocates exactly what each frame needs in
			 * arrival order (pktio/loop.c:253-384, odp_packet_io.c:680-705).
			 * A single slot takes min(n, available): every frame needs at
			 * most one packet of it, so such a burst is short only when the
			 * pool is, as the reference's would be (no reserve then: it would
			 * cut the pipeline's takes on pools sized for the bursts in
			 * flight, 46 -> 23 Mpkt/s on a 20 k-packet pool). */
			if (e->rx_np > 1) {
				const uint32_t av = rt_pool_avail(e->rx_pools[k]);
				const uint32_t cap = av > n ? av - n : 0u;

				if (want > cap)
					want = cap;
			}
			s->cbase[j][k] = at;
			s->chave[j][k] = want ? (uint32_t)rt_packet_alloc_raw(s->cpool[k], 0,
									      (odp_packet_t *)(void *)(s->got + at),
									      (int)want) : 0u;
			at += s->chave[j][k];
		}
	}
	s->gen = odp_amd_cls_generation();
	s->dgen = e->rxtab_gen;
	s->dticket = 0;
	const uint64_t tc = prof_ns();

	for (int j = 0; j < nsl; j++) {
		const uint32_t lo = s->sl_lo[j];
		mi_cls_rxc_args_t a;

		memset(&a, 0, sizeof(a));
		a.base = s->base;
		a.soff = s->soff + lo;
		a.slen = s->slen + lo;
		a.res = s->res + lo;
		a.n = s->sl_lo[j + 1] - lo;
		a.layer = (uint32_t)e->parse_layer;
		a.input = (uint64_t)(uintptr_t)e->hdl;
		a.headroom = RT_PKT_HEADROOM;
		a.data_from_meta = rt_data_from_meta();
		a.tab = e->rxtab;
		a.got = s->got;
		memcpy(a.got_base, s->cbase[j], sizeof(a.got_base));
		memcpy(a.have, s->chave[j], sizeof(a.have));
		if (e->drv == DRV_LOOP) {
			a.pk = (const uint64_t *)(const void *)(s->pk + lo);
			a.ppool = s->ppool + lo;
			a.stage = (uint32_t)s->gstage;
			a.head_off = (uint16_t)__builtin_offsetof(pkt_hdr_t, head);
			a.pool_off = (uint16_t)__builtin_offsetof(pkt_hdr_t, ev.pool);
		}
		a.meta_off = (uint32_t)__builtin_offsetof(pkt_hdr_t, meta);
		s->rxo[j].not_in_place = 0;
		a.dec = s->dec + lo;
		a.ent = s->cent + lo;
		a.perm = s->perm + lo;
		a.gcnt = s->gcnt + (size_t)j * MI_CLS_DLV_GROUPS;
		a.out = &s->rxo[j];
		s->sl_tk[j] = 0;
		const int crc = odp_amd_cls_rx_chain_dev(e->hdl, (uint32_t)j, s->base, s->bytes, &a,
							 &s->sl_tk[j]);

		if (crc != 0) {
			/* the slices in flight write into packets taken: wait for
			 * them before every packet goes back */
			(void)rxc_wait(e, s, j);
			rxc_return(s);
			e->prof[13] += prof_ns() - tc;
			return rxc_no(e, s);
		}
	}
	e->prof[13] += prof_ns() - tc;
	s->chain = 1;
	s->ticket = 0;
	s->pending = 0;
	s->delivering = 1;
	s->derr = 0;
	return 1;
}

/* End set s's chain: wait for its slices, give back the packets no frame
 * took, free the loop packets that were dropped or copied into another
 * pool, enqueue (slice by slice: one enqueue per queue group, else runs in
 * arrival order), add the counters.  A burst that was short of packets, or
 * that the control plane changed under, is finished on the host instead.
 * Returns the packets placed in out[] (none: the classifier is on). */
static int rxc_end(rt_pktio_t *e, rx_set_t *s, odp_packet_t out[], int max_out)
{
	const uint64_t tk0 = prof_ns();
	int rc = rxc_wait(e, s, s->nsl);
	uint32_t short_pool = 0, nip = 0;

	s->delivering = 0;
	s->chain = 0;
	s->dticket = 0;
	e->prof[9] += prof_ns() - tk0;
	for (int j = 0; j < s->nsl; j++) {
		short_pool |= s->rxo[j].short_pool;
		nip |= s->rxo[j].not_in_place;
	}
	if (!rc) {
		/* the next bursts' packets per slot: this one's need plus a margin */
		for (uint32_t k = 0; k < s->cnp && k < e->rx_np; k++) {
			uint32_t need = 0;

			for (int j = 0; j < s->nsl; j++)
				need += s->rxo[j].need[k];
			e->rx_want[k] = need + need / 4u + 32u;
		}
	}
	if (rc || short_pool || nip || s->dgen != odp_amd_cls_generation()) {
		/* every packet taken for the burst back; the host path then
		 * decides, allocates and delivers from the records (the classify
		 * records are valid; a control-plane change re-classifies).  A loop
		 * burst the GPU staged is staged and classified again by the host
		 * (its headrooms and user pointers are the host path's inputs; a
		 * packet outside the page-locked arena is copied) */
		e->prof[15]++;
		rxc_return(s);
		if (rc) {
			s->gstage = 0;
			rx_drop(e, s, rc);
			return 0;
		}
		const int restage = s->gstage;

		(void)rxc_no(e, s);
		if (restage && (s->n == 0 || rx_classify(e, s, 0)))
			return 0;   /* dropped and counted */
		s->pending = 1;
		return rx_finish(e, s, out, max_out);
	}
	s->gstage = 0;
	e->prof[14]++;
	const uint64_t tk1 = prof_ns();

	for (int j = 0; j < s->nsl; j++)
		for (uint32_t k = 0; k < s->cnp; k++)
			if (s->rxo[j].used[k] < s->chave[j][k])
				rt_packet_return_raw(s->cpool[k],
						     (const odp_packet_t *)(const void *)(s->got + s->cbase[j][k] +
											   s->rxo[j].used[k]),
						     (int)(s->chave[j][k] - s->rxo[j].used[k]));
	if (e->drv == DRV_LOOP) {
		/* loop packets not delivered in their own buffer: dropped,
		 * discarded, or copied into a packet of their CoS pool */
		for (int i = 0; i < s->n; i++)
			if ((s->dec[i] & 3u) != MI_CLS_RXF_INPLACE)
				odp_packet_free(s->pk[i]);
	}
	rx_tmp_ensure(s);
	odp_packet_t *tmp = s->tmp;
	uint8_t *cos = rx_tmp_bytes(s);

	if ((e->rxtab->flags & MI_CLS_RXT_GROUP) && tmp) {
		/* per slice, in device order: group g holds frames perm[at ..
		 * at + gcnt[g]) of the slice (indexes within it) of the queue whose
		 * entries carry group g */
		for (int j = 0; j < s->nsl; j++) {
			const uint32_t lo = s->sl_lo[j];
			const uint32_t *gc = s->gcnt + (size_t)j * MI_CLS_DLV_GROUPS;
			const uint32_t *pm = s->perm + lo;
			uint32_t at = 0;

			for (int g = 0; g < MI_CLS_DLV_GROUPS; g++) {
				const uint32_t num = gc[g] & 0xFFFFu;

				if (!num)
					continue;
				const mi_cls_result_t *r0 = &s->res[lo + pm[at]];
				const odp_queue_t q = (odp_queue_t)(uintptr_t)
					e->rxtab->qh[e->rxtab->cos_q0[r0->cos] + r0->queue];
				const int one_cos = gc[g] >> 24;   /* the decide kernel saw one CoS in the group */

				for (uint32_t k = 0; k < num; k++) {
					tmp[k] = (odp_packet_t)(uintptr_t)s->cent[lo + pm[at + k]];
					if (!one_cos)
						cos[k] = s->res[lo + pm[at + k]].cos;
				}
				if (one_cos) {
					const uint32_t c1 = (gc[g] >> 16) & 0xFFu;
					const int r = rx_enq_plain(q, tmp, (int)num);

					odp_amd_cls_queue_stats_add(c1, cos_slot_of(c1, q), (uint64_t)r,
								    (uint64_t)((int)num - r));
				} else {
					rx_enq_group(q, tmp, cos, (int)num);
				}
				at += num;
			}
		}
	} else {
		/* runs of equal (queue, CoS) in arrival order (_odp_cls_enq) */
		int nd = 0;

		for (int i = 0; i < s->n; i++)
			if (s->cent[i])
				s->pk[nd++] = (odp_packet_t)(uintptr_t)s->cent[i];
		rx_enqueue(s, s->pk, nd);
	}
	rx_cnt_t c = { 0, 0, 0, 0 };

	for (int j = 0; j < s->nsl; j++) {
		c.in_errors += s->rxo[j].in_errors;
		c.in_discards += s->rxo[j].in_discards;
		c.octets += s->rxo[j].octets;
		c.packets += s->rxo[j].packets;
	}
	rx_cnt_flush(e, &c);
	e->prof[10] += prof_ns() - tk1;
	(void)out;
	(void)max_out;
	return 0;
}

/* One receive call.  With the classifier enabled and more frames waiting at
 * the driver, bursts stream through RX_SETS sets by age: staged and
 * submitted for classification (age 0), classification in flight (ages 1 ..
 * RX_CLS_DEPTH), decided from their records and GPU delivery started (age
 * RX_CLS_DEPTH), delivery in flight (older), enqueued (the oldest).  Each
 * GPU step then has that many calls of host work to run behind before a
 * call waits for it (a delivery copies ~1.5 MB of frames over PCIe per
 * 4096-frame burst).  A call with nothing more at the driver delivers
 * everything, oldest first.  Unclassified packets are returned in out[] (at
 * most max_out); classified ones are enqueued to their CoS queues. */
static int pktio_recv(rt_pktio_t *e, uint32_t idx, odp_packet_t out[], int max_out)
{
	rx_set_t *s = rx_age(e, 0);

	/* several input queues exist only with the classifier off, where a call
	 * leaves no burst in flight (pipe is 0): the burst sets stay per pktio */
	e->rx_idx = idx;
	long pending_n = 0;   /* frames staged, not yet taken from pools */
	int in_flight = 0;

	for (int k = 1; k < RX_SETS; k++) {
		const rx_set_t *o = rx_age(e, k);

		pending_n += o->pending ? (long)o->n : 0;
		in_flight |= o->pending || o->delivering;
	}
	const int pipe = e->cls_enabled && e->parse_layer != ODP_PROTO_LAYER_NONE &&
			 rx_pipeline();
	uint32_t burst = rx_burst();
	int num_rx = 0;

	if (rx_prof < 0)
		rx_prof = getenv("ODP_AMD_RX_PROF") != NULL;
	if (!e->cls_enabled && (uint32_t)max_out < burst)
		burst = (uint32_t)max_out;
	if (e->drv == DRV_PCAP) {
		/* pcap frames become packets of the pktio's pool at delivery: stage
		 * no more than the pool can still hold after the bursts in flight,
		 * so a packet allocation never fails on a staged frame (frames not
		 * staged stay in the store for the next call; the reference instead
		 * consumes the frame and stops on a failed allocation, pcap.c:324-327) */
		/* (frames that all go to CoS with pools of their own never take a
		 * packet of the pktio's pool: no bound then) */
		if (rt_pool(e->pool) && !(e->cls_enabled && odp_amd_cls_all_cos_pooled(e->pool))) {
			long room = (long)rt_pool_avail(e->pool) - pending_n;

			if (room < (long)burst)
				burst = room > 0 ? (uint32_t)room : 0u;
		}
	}
	uint64_t t0 = prof_ns();
	int n = stage_frames(e, s, burst, idx);
	uint64_t t1 = prof_ns();

	e->prof[0] += t1 - t0;
	if (n < 0 && !in_flight)
		return n;
	s->n = n > 0 ? n : 0;
	if (n > 0) {
		e->prof[3]++;
		const int chained = pipe && rxc_submit(e, s);

		/* a burst that takes the classic path is staged by the host first
		 * (rxc_no: a no-op unless the GPU was to stage it) */
		if (!chained && !pipe)
			rxc_no(e, s);
		if (!chained && (s->n == 0 || rx_classify(e, s, pipe)))
			n = 0;
		e->prof[1] += prof_ns() - t1;
	}
	/* bursts are delivered in arrival order: the oldest first */
	rx_set_t *z = rx_age(e, RX_SETS - 1);

	if (z->delivering)
		num_rx += rx_dlv_end(e, z, out, max_out);
	/* only a burst really in flight streams (a multi-GPU pktio's submit
	 * completes before it returns: ticket 0) */
	if (n > 0 && pipe && (s->ticket || s->chain) && rx_more(e, idx)) {
		rx_set_t *q = rx_age(e, RX_CLS_DEPTH);

		if (q->pending)
			rx_finish_start(e, q);
		e->cur = (e->cur + 1) % RX_SETS;
		return num_rx;
	}
	/* the rest in arrival order: deliveries in flight, then the bursts
	 * still pending, then s */
	for (int k = RX_SETS - 2; k >= 1; k--) {
		rx_set_t *b = rx_age(e, k);

		if (b->delivering)
			num_rx += rx_dlv_end(e, b, out + num_rx, max_out - num_rx);
		if (b->pending)
			num_rx += rx_finish(e, b, out + num_rx, max_out - num_rx);
	}
	if (n > 0) {
		if (s->delivering)
			num_rx += rx_dlv_end(e, s, out + num_rx, max_out - num_rx);
		else
			num_rx += rx_finish(e, s, out + num_rx, max_out - num_rx);
	}
	return num_rx;
}

/* A pktio that stops (odp_pktio_stop, under rxl): bursts still on the GPU
 * were received before the stop: deliver them, oldest first. */
void rx_drain(rt_pktio_t *e)
{
	for (int k = 1; k <= RX_SETS; k++) {
		rx_set_t *s = &e->rs[(e->cur + k) % RX_SETS];

		if (s->delivering)
			(void)rx_dlv_end(e, s, NULL, 0);
		if (s->pending)
			(void)rx_finish(e, s, NULL, 0);
	}
}

/* receive into the pktin queue (SCHED / QUEUE modes) */
static int poll_into_inq(rt_pktio_t *e)
{
	odp_packet_t pk[RX_BURST_DEFAULT];
	int total = 0;

	/* every input queue in turn, each into its own event queue */
	for (uint32_t idx = 0; idx == 0 || idx < e->num_in; idx++) {
		odp_queue_t inq;
		int n;

		if (!odp_spinlock_trylock(&e->rxl))
			return total;
		if (e->state != ST_STARTED || idx >= (e->num_in ? e->num_in : 1u)) {
			odp_spinlock_unlock(&e->rxl);
			return total;
		}
		inq = e->inq[idx];
		n = pktio_recv(e, idx, pk, RX_BURST_DEFAULT);
		odp_spinlock_unlock(&e->rxl);
		if (n > 0) {
			int r = odp_queue_enq_multi(inq, (const odp_event_t *)(void *)pk, n);

			if (r < 0)
				r = 0;
			if (r < n) {
				odp_packet_free_multi(&pk[r], n - r);
				odp_atomic_add_u64(&e->in_discards, (uint64_t)(n - r));
				odp_atomic_add_u64(&e->inq_st[idx].discards, (uint64_t)(n - r));
			}
			total += n;
		}
	}
	return total;
}

int rt_pktio_sched_poll(void)
{
	int idx[RT_MAX_PKTIO], n, total = 0;

	if (!__atomic_load_n(&num_sched_pktio, __ATOMIC_RELAXED))
		return 0;
	odp_spinlock_lock(&pk_lock);
	n = num_sched_pktio;
	memcpy(idx, sched_list, (size_t)n * sizeof(int));
	odp_spinlock_unlock(&pk_lock);
	for (int i = 0; i < n; i++)
		total += poll_into_inq(&PK[idx[i]]);
	return total;
}

int rt_pktio_poll_index(int idx)
{
	if (idx < 0 || idx >= RT_MAX_PKTIO || !PK[idx].used)
		return 0;
	return poll_into_inq(&PK[idx]);
}

int odp_pktin_recv(odp_pktin_queue_t q, odp_packet_t pkts[], int num)
{
	rt_pktio_t *e = get_pk(q.pktio);
	int n;

	if (!e || num < 0)
		return -1;
	if (e->state != ST_STARTED)
		return 0;
	odp_spinlock_lock(&e->rxl);
	if (q.index < 0 || (uint32_t)q.index >= (e->num_in ? e->num_in : 1u))
		n = -1;
	else
		n = e->state == ST_STARTED ? pktio_recv(e, (uint32_t)q.index, pkts, num) : 0;
	odp_spinlock_unlock(&e->rxl);
	return n;
}

uint64_t odp_pktin_wait_time(uint64_t nsec)
{
	return nsec;
}

int odp_pktin_recv_tmo(odp_pktin_queue_t q, odp_packet_t pkts[], int num, uint64_t wait)
{
	odp_time_t t0 = odp_time_local();

	for (;;) {
		int n = odp_pktin_recv(q, pkts, num);

		if (n != 0 || wait == ODP_PKTIN_NO_WAIT)
			return n;
		if (wait != ODP_PKTIN_WAIT &&
		    odp_time_diff_ns(odp_time_local(), t0) >= wait)
			return 0;
		odp_time_wait_ns(10 * ODP_TIME_USEC_IN_NS);
	}
}

/* Build extension: 1 when the driver has no more input and no receive burst
 * is in flight (pcap past EOF, loop queue empty); 0 otherwise; -1 bad handle. */
int odp_amd_pktio_rx_idle(odp_pktio_t h)
{
	rt_pktio_t *e = get_pk(h);
	int idle;

	if (!e)
		return -1;
	odp_spinlock_lock(&e->rxl);
	idle = 1;
	for (int k = 0; k < RX_SETS; k++)
		if (e->rs[k].pending || e->rs[k].delivering)
			idle = 0;
	if (idle && e->drv == DRV_PCAP) {
		idle = e->eof || e->fs.n == 0 || (e->next >= e->fs.n && e->loops == 1);
	} else if (idle && e->drv == DRV_LOOP) {
		for (uint32_t i = 0; i < ODP_PKTIN_MAX_QUEUES && e->loopq[i] != ODP_QUEUE_INVALID; i++)
			idle &= ((rt_queue_t *)(void *)e->loopq[i])->count == 0;
	}
	odp_spinlock_unlock(&e->rxl);
	return idle;
}
