/*
 * odp_pktio.c -- packet I/O for the MI355X build, control plane and
 * statistics: the pktio table, open / config / start / stop / close of the
 * "loop", "pcap" and "null" drivers, their queue configuration, and the
 * counters' getters.  The receive path is odp_pktin.c, the transmit side
 * odp_pktout.c, the capture file reader odp_pcap.c.
 *
 * Reference behaviour:
 *   platform/linux-generic/odp_packet_io.c  (open/config/start/stop/close,
 *                                            pktin/pktout queue config)
 *   platform/linux-generic/pktio/pcap.c:90-117    devname parsing
 *   platform/linux-generic/pktio/loop.c:172-227   the loop queues
 */
#define _GNU_SOURCE
#include <errno.h>
#include <inttypes.h>
#include <string.h>

#include "odp_pktio_internal.h"

rt_pktio_t PK[RT_MAX_PKTIO];
odp_spinlock_t pk_lock;
/* started SCHED-mode pktios, polled from odp_schedule*() */
int sched_list[RT_MAX_PKTIO];
int num_sched_pktio;

static const uint8_t loop_mac[6] = { 0x02, 0xe9, 0x34, 0x80, 0x73, 0x01 };

uint32_t rt_gpu_index(void)
{
	const char *e = getenv("ODP_AMD_GPU");

	return e ? (uint32_t)atoi(e) : 0u;
}

/* ============================================================ pcap files */
static void store_free(rt_pktio_t *e)
{
	if (e->fs_pinned) {
		mi_cls_host_free(e->fs.buf);
		e->fs.buf = NULL;
		e->fs_pinned = 0;
	}
	pcap_store_free(&e->fs);
}

/* The input file's frames into e->fs (odp_pcap.c).  Returns 0 / -1. */
static int pcap_input_load(rt_pktio_t *e, const char *fname)
{
	uint32_t link = 0;
	const int rc = pcap_load(fname, &e->fs, &link);

	if (rc == PCAP_E_OPEN)
		RT_ERR("failed to open pcap file %s (%s)\n", fname, strerror(errno));
	else if (rc == PCAP_E_FORMAT)
		RT_ERR("%s: not a pcap / pcapng file\n", fname);
	else if (rc == PCAP_E_LINKTYPE && e->fs.pcapng)
		RT_ERR("unsupported datalink type in %s\n", fname);
	else if (rc == PCAP_E_LINKTYPE)
		RT_ERR("unsupported datalink type: %u\n", link);
	if (rc)
		return -1;
	if (e->fs.buf) {
		/* page-locked frame store: the GPU reads the bursts' header windows
		 * in place (zero copy, mi_cls_classify_host) and no staging copy is
		 * made.  ODP_AMD_RX_INPLACE=0 keeps the staged copies (A/B runs). */
		int in_place = -1;   /* per load: not cached */
		uint8_t *pb = env_switch("ODP_AMD_RX_INPLACE", &in_place) ? mi_cls_host_alloc(e->fs.bytes) : NULL;

		if (pb) {
			memcpy(pb, e->fs.buf, e->fs.bytes);   /* the zero tail included */
			free(e->fs.buf);
			e->fs.buf = pb;
			e->fs_pinned = 1;
		}
	}
	return 0;
}

static int pcap_dump_open(rt_pktio_t *e, const char *fname)
{
	e->tx = fopen(fname, "wb");
	if (!e->tx) {
		RT_ERR("failed to open dump file %s\n", fname);
		return -1;
	}
	pcap_dump_header(e->tx);
	return 0;
}

/* _pcapif_parse_devname (pcap.c:90-117) */
static int pcap_open(rt_pktio_t *e, const char *devname)
{
	char in[ODP_PKTIO_NAME_LEN], *tok, *save = NULL;
	char *rx = NULL, *txn = NULL;
	int rc = 0;

	snprintf(in, sizeof(in), "%s", devname);
	e->loops = 1;
	e->loop_cnt = 1;
	for (tok = strtok_r(in + 5, ":", &save); tok; tok = strtok_r(NULL, ":", &save)) {
		if (strncmp(tok, "in=", 3) == 0 && !rx) {
			rx = strdup(tok + 3);
		} else if (strncmp(tok, "out=", 4) == 0 && !txn) {
			txn = strdup(tok + 4);
		} else if (strncmp(tok, "loops=", 6) == 0) {
			e->loops = atoi(tok + 6);
			if (e->loops < 0) {
				RT_ERR("invalid loop count\n");
				rc = -1;
			}
		}
	}
	if (!rc && rx)
		rc = pcap_input_load(e, rx);
	if (!rc && txn)
		rc = pcap_dump_open(e, txn);
	if (!rc && !rx && !txn)
		rc = -1;
	free(rx);
	free(txn);
	e->promisc = 0;   /* pcapif_init sets promisc off (pcap.c:232) */
	return rc;
}

/* ============================================================ open / config */
void odp_pktio_param_init(odp_pktio_param_t *p)
{
	memset(p, 0, sizeof(*p));
	p->in_mode = ODP_PKTIN_MODE_DIRECT;
	p->out_mode = ODP_PKTOUT_MODE_DIRECT;
}

void odp_pktin_queue_param_init(odp_pktin_queue_param_t *p)
{
	memset(p, 0, sizeof(*p));
	p->op_mode = ODP_PKTIO_OP_MT;
	p->num_queues = 1;
	p->classifier_enable = 0;
	odp_queue_param_init(&p->queue_param);
	p->queue_param.type = ODP_QUEUE_TYPE_SCHED;
}

void odp_pktout_queue_param_init(odp_pktout_queue_param_t *p)
{
	memset(p, 0, sizeof(*p));
	p->op_mode = ODP_PKTIO_OP_MT;
	p->num_queues = 1;
}

void odp_pktio_config_init(odp_pktio_config_t *c)
{
	memset(c, 0, sizeof(*c));
	c->parser.layer = ODP_PROTO_LAYER_ALL;
	c->reassembly.max_num_frags = 2;
}

static void queue_drain_destroy(odp_queue_t *q)
{
	odp_event_t ev[64];
	int n;

	if (*q == ODP_QUEUE_INVALID)
		return;
	while ((n = rt_queue_deq_multi_raw((rt_queue_t *)(void *)*q, ev, 64)) > 0)
		odp_event_free_multi(ev, n);
	odp_queue_destroy(*q);
	*q = ODP_QUEUE_INVALID;
}

/* The loop queues of a loop pktio, one per input queue (loop.c:172-206):
 * those it has are drained and destroyed, then n are created, queue i
 * holding at most size[i] events (0, or size NULL: no bound). */
static int loopqs_create(rt_pktio_t *e, uint32_t n, const uint32_t size[])
{
	for (uint32_t i = 0; i < ODP_PKTIN_MAX_QUEUES; i++)
		queue_drain_destroy(&e->loopq[i]);
	for (uint32_t i = 0; i < n; i++) {
		odp_queue_param_t qp;
		char qn[ODP_QUEUE_NAME_LEN];

		odp_queue_param_init(&qp);
		if (i == 0)
			snprintf(qn, sizeof(qn), "%.20s_loopq", e->name);
		else
			snprintf(qn, sizeof(qn), "%.20s_loopq-%u", e->name, i);
		e->loopq[i] = odp_queue_create(qn, &qp);
		if (e->loopq[i] == ODP_QUEUE_INVALID) {
			while (i--)
				queue_drain_destroy(&e->loopq[i]);
			return -1;
		}
		((rt_queue_t *)(void *)e->loopq[i])->limit = size ? size[i] : 0;
	}
	return 0;
}

odp_pktio_t odp_pktio_open(const char *name, odp_pool_t pool, const odp_pktio_param_t *param)
{
	odp_pktio_param_t def;
	int drv;

	if (!name)
		return ODP_PKTIO_INVALID;
	if (strncmp(name, "pcap:", 5) == 0)
		drv = DRV_PCAP;
	else if (strncmp(name, "loop", 4) == 0)
		drv = DRV_LOOP;
	else if (strncmp(name, "null", 4) == 0)
		drv = DRV_NULL;
	else {
		RT_ERR("pktio %s: no driver (this build has loop, pcap:in=/out=, null)\n", name);
		return ODP_PKTIO_INVALID;
	}
	rt_pool_t *pp = rt_pool(pool);

	if (!pp || pp->param.type != ODP_POOL_PACKET) {
		RT_ERR("pktio %s: invalid packet pool\n", name);
		return ODP_PKTIO_INVALID;
	}
	if (!param) {
		odp_pktio_param_init(&def);
		param = &def;
	}
	if (odp_pktio_lookup(name) != ODP_PKTIO_INVALID) {
		RT_ERR("pktio %s already open\n", name);
		return ODP_PKTIO_INVALID;
	}
	/* the classifier endpoint (classifier_t + device context) gives the
	 * handle; ODP_AMD_GPUS="0,1,..." shards each receive burst over several
	 * GPUs (mi_cls_group_classify_host), otherwise ODP_AMD_GPU picks one */
	int gpus[16], ngpu = 0;
	const char *ge = getenv("ODP_AMD_GPUS");

	while (ge && *ge && ngpu < 16) {
		char *end;
		long v = strtol(ge, &end, 10);

		if (end == ge)
			break;
		gpus[ngpu++] = (int)v;
		ge = *end == ',' ? end + 1 : end;
	}
	odp_pktio_t h = ngpu > 1 ? odp_amd_cls_pktio_create_multi(gpus, ngpu)
				 : odp_amd_cls_pktio_create(ngpu == 1 ? gpus[0] : (int)rt_gpu_index());

	if (h == ODP_PKTIO_INVALID)
		return h;
	rt_pktio_t *e = &PK[(uintptr_t)h - 1];

	odp_spinlock_lock(&pk_lock);
	memset(e, 0, sizeof(*e));
	e->used = 1;
	odp_spinlock_unlock(&pk_lock);
	snprintf(e->name, sizeof(e->name), "%s", name);
	e->drv = drv;
	e->hdl = h;
	e->pool = pool;
	e->param = *param;
	odp_pktio_config_init(&e->config);
	odp_spinlock_init(&e->rxl);
	pthread_mutex_init(&e->txl, NULL);
	e->state = ST_OPENED;
	e->promisc = 1;
	if (drv == DRV_PCAP && pcap_open(e, name)) {
		store_free(e);
		e->used = 0;
		odp_amd_cls_pktio_destroy(h);
		return ODP_PKTIO_INVALID;
	}
	if (drv == DRV_LOOP) {
		if (loopqs_create(e, 1, NULL)) {
			e->used = 0;
			odp_amd_cls_pktio_destroy(h);
			return ODP_PKTIO_INVALID;
		}
	}
	/* default queue config as odp_pktio_open does for DISABLED-less modes */
	odp_pktin_queue_param_init(&e->inq_param);
	return h;
}

/* The pool plan's table for this pktio: the control plane's slots
 * (odp_amd_cls_pooltab_cos, under its lock) over the pktio's pool, then each
 * slot's packet capacity from the runtime's pools, the value the receive
 * table's pool_cap takes.  Host only. */
int odp_amd_cls_pooltab_fill(odp_pktio_t h, struct mi_cls_pool_tab *tab, odp_pool_t pools[], uint32_t *nslot,
			     uint64_t *gen)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || !tab || !pools || !nslot || !gen)
		return -EINVAL;
	const int rc = odp_amd_cls_pooltab_cos(e->pool, tab, pools, nslot, gen);

	for (uint32_t k = 0; rc == 0 && k < *nslot && k < MI_CLS_POOL_SLOTS; k++) {
		const rt_pool_t *rp = rt_pool(pools[k]);

		if (!rp || rp->param.type != ODP_POOL_PACKET)
			return -EINVAL;
		tab->slot_cap[k] = rp->data_cap;
	}
	return rc;
}

int odp_amd_cls_pool_own(const odp_packet_t pk[], uint32_t n, const odp_pool_t pools[], uint32_t nslot,
			 uint8_t own[])
{
	if ((n && (!pk || !own)) || (nslot && !pools) || nslot > MI_CLS_POOL_SLOTS)
		return -EINVAL;
	for (uint32_t i = 0; i < n; i++) {
		const odp_pool_t p = pk[i] != ODP_PACKET_INVALID ? odp_packet_pool(pk[i]) : ODP_POOL_INVALID;
		uint32_t k = 0;

		while (k < nslot && pools[k] != p)
			k++;
		own[i] = (uint8_t)(k < nslot ? k + 1u : 0u);
	}
	return 0;
}

/* The pool move's geometry: the runtime's packet layout (a packet handle is
 * its header's address; its metadata line lies meta_off behind it and a fresh
 * packet's data data_from_meta behind the line) and the one range all
 * page-locked pools lie in.  -ENOENT when there is none (pageable pools). */
int odp_amd_cls_pool_move_geom(uint32_t *meta_off, uint32_t *data_from_meta, uint64_t *arena_lo,
			       uint64_t *arena_bytes)
{
	uint8_t *lo;
	size_t span;

	if (!meta_off || !data_from_meta || !arena_lo || !arena_bytes)
		return -EINVAL;
	*meta_off = (uint32_t)__builtin_offsetof(pkt_hdr_t, meta);
	*data_from_meta = rt_data_from_meta();
	*arena_lo = 0;
	*arena_bytes = 0;
	if (!rt_pinned_arena(&lo, &span))
		return -ENOENT;
	*arena_lo = (uint64_t)(uintptr_t)lo;
	*arena_bytes = span;
	return 0;
}

/* The vector fill's geometry: the runtime's packet-vector layout (a vector's
 * handle is its header's address) and the one range all page-locked vector
 * pools lie in.  -ENOENT when there is none. */
int odp_amd_cls_vec_geom(uint32_t *size_off, uint32_t *tbl_off, uint64_t *varena_lo, uint64_t *varena_bytes)
{
	uint8_t *lo;
	size_t span;

	if (!size_off || !tbl_off || !varena_lo || !varena_bytes)
		return -EINVAL;
	*size_off = (uint32_t)__builtin_offsetof(evv_hdr_t, size);
	*tbl_off = (uint32_t)__builtin_offsetof(evv_hdr_t, tbl);
	*varena_lo = 0;
	*varena_bytes = 0;
	if (!rt_vec_arena(&lo, &span))
		return -ENOENT;
	*varena_lo = (uint64_t)(uintptr_t)lo;
	*varena_bytes = span;
	return 0;
}

int odp_amd_cls_vec_take(const odp_pool_t vpools[], uint32_t nslots, const uint64_t need[],
			 uint64_t vgot[], uint32_t vgot_cap, uint32_t vbase[], uint32_t vhave[],
			 uint32_t vcap[])
{
	uint64_t want = 0;
	uint32_t at = 0;

	if (!need || !vbase || !vhave || !vcap || (nslots && !vpools) || nslots > MI_CLS_RUN_VSLOTS)
		return -EINVAL;
	for (uint32_t s = 0; s < nslots; s++) {
		const rt_pool_t *p = rt_pool(vpools[s]);

		if (!p || p->param.type != ODP_POOL_VECTOR)
			return -EINVAL;
		const uint32_t avail = rt_pool_avail(vpools[s]);

		want += need[s] < avail ? need[s] : avail;
	}
	if (want > vgot_cap || (want && !vgot))
		return -ENOSPC;
	for (uint32_t s = 0; s < MI_CLS_RUN_VSLOTS; s++) {
		vbase[s] = at;
		vhave[s] = 0;
		vcap[s] = 0;
		if (s >= nslots)
			continue;
		const rt_pool_t *p = rt_pool(vpools[s]);
		const uint32_t avail = rt_pool_avail(vpools[s]);
		const uint64_t w = need[s] < avail ? need[s] : avail;

		vcap[s] = p->data_cap;
		if (w)
			vhave[s] = (uint32_t)rt_vector_alloc_raw(vpools[s], (odp_event_t *)(void *)(vgot + at), (int)w);
		at += vhave[s];
	}
	return (int)at;
}

/* Queue slot of dst inside the CoS (_odp_cos_queue_idx,
 * odp_classification_internal.h:49-65): 0 for a single-queue CoS. */
static uint32_t vec_cos_slot(uint32_t cos_index, odp_queue_t dst)
{
	odp_cos_t cos = (odp_cos_t)(uintptr_t)(cos_index + 1u);
	uint32_t nq = odp_cls_cos_num_queue(cos), slot = 0;

	if (nq > 1) {
		odp_queue_t qs[32];

		odp_cls_cos_queues(cos, qs, 32);
		for (uint32_t i = 0; i < nq && i < 32; i++)
			if (qs[i] == dst)
				slot = i;
	}
	return slot;
}

/* The entries of value 0 taken out of e[0..n), order kept; returns the rest */
static uint32_t vec_compact(uint64_t e[], uint32_t n)
{
	uint32_t k = 0;

	while (k < n && e[k])
		k++;
	for (uint32_t i = k; i < n; i++)
		if (e[i])
			e[k++] = e[i];
	return k;
}

int64_t odp_amd_cls_vec_enq(const struct mi_cls_run *runs, const struct mi_cls_evrun *evr, uint32_t nruns,
			    uint64_t ev[], const uint64_t lost[], uint32_t nlost,
			    const odp_queue_t dst_queue[], uint32_t ndst, const struct mi_cls_run_tab *rtab,
			    const odp_pool_t vpools[], uint32_t nslots, const uint64_t vgot[],
			    const uint32_t vbase[], const uint32_t vhave[], const struct mi_cls_vec_out *out,
			    const uint32_t seq[], const uint64_t ent[], uint64_t ent_to_handle)
{
	int64_t events = 0;

	if ((nruns && (!runs || !evr || !ev || !dst_queue)) || (nlost && !lost) || !rtab || !out ||
	    (nslots && (!vpools || !vbase || !vhave)) || nslots > MI_CLS_RUN_VSLOTS)
		return -EINVAL;
	for (uint32_t r = 0; r < nruns; r++)
		if (runs[r].dst >= ndst)
			return -EINVAL;
	for (uint32_t r = 0; r < nruns; r++) {
		const mi_cls_run_t *u = &runs[r];
		const mi_cls_evrun_t *x = &evr[r];
		const odp_queue_t dst = dst_queue[u->dst];
		const uint32_t slot = vec_cos_slot(u->cos, dst);
		odp_event_t *e = (odp_event_t *)(void *)(ev + x->ev_first);
		const int vec = (u->flags & MI_CLS_RUN_VEC) != 0;
		const uint32_t vm = rtab->vmax[u->cos] ? rtab->vmax[u->cos] : 1u;
		uint64_t refused_pk = 0;
		int ret;

		/* a refused vector (entry 0 among the run's ev_count): its packets were
		 * put nowhere; with seq and ent they are freed here, else they stay the
		 * caller's (reachable through ent).  Discards either way. */
		for (uint32_t k = 0; vec && k < x->ev_count; k++) {
			if (e[k])
				continue;
			const uint32_t at = k * vm, sz = u->count - at < vm ? u->count - at : vm;

			refused_pk += sz;
			for (uint32_t j = 0; seq && ent && j < sz; j++) {
				const uint64_t l = ent[seq[u->first + at + j]];

				if (l)
					odp_packet_free((odp_packet_t)(uintptr_t)(l - ent_to_handle));
			}
		}
		const uint32_t num = vec_compact(ev + x->ev_first, x->ev_count);

		if (!vec) {
			const odp_queue_t q = (u->flags & MI_CLS_RUN_AGGR) ? odp_queue_aggr(dst, 0) : dst;

			ret = num && q != ODP_QUEUE_INVALID ? odp_queue_enq_multi(q, e, (int)num) : 0;
			if (ret < 0)
				ret = 0;
			if ((uint32_t)ret != num)
				odp_packet_free_multi((const odp_packet_t *)(void *)(e + ret), (int)num - ret);
			odp_amd_cls_queue_stats_add(u->cos, slot, (uint64_t)ret, (uint64_t)u->count - (uint64_t)ret);
			events += ret;
			continue;
		}
		if (num == 0) {   /* no vector: the run's packets are in lost[] (or were refused) */
			odp_amd_cls_queue_stats_add(u->cos, slot, 0, u->count);
			continue;
		}
		ret = dst != ODP_QUEUE_INVALID ? odp_queue_enq_multi(dst, e, (int)num) : -1;
		if ((uint32_t)ret == num) {   /* the queue took what was offered */
			const uint64_t enq = x->pk_enq - refused_pk;

			odp_amd_cls_queue_stats_add(u->cos, slot, enq, (uint64_t)u->count - enq);
			events += ret;
			continue;
		}
		if (ret < 0)
			ret = 0;
		/* the reference's figure (odp_classification_internal.h:125-129) */
		uint64_t enq = (uint64_t)vm * (uint32_t)ret;

		if (enq > u->count)
			enq = u->count;
		odp_amd_cls_queue_stats_add(u->cos, slot, enq, (uint64_t)u->count - enq);
		events += ret;
		for (uint32_t i = (uint32_t)ret; i < num; i++) {
			odp_packet_vector_t pv = odp_packet_vector_from_event(e[i]);
			odp_packet_t *tbl;
			uint32_t sz = odp_packet_vector_tbl(pv, &tbl);

			sz = vec_compact((uint64_t *)(void *)tbl, sz);
			odp_packet_free_multi(tbl, (int)sz);
			odp_packet_vector_free(pv);
		}
	}
	/* one free call for the lost packets; in pieces only to leave out holes */
	if (out->holes == 0 && nlost) {
		odp_packet_free_multi((const odp_packet_t *)(const void *)lost, (int)nlost);
		nlost = 0;
	}
	for (uint32_t i = 0; i < nlost;) {
		odp_packet_t pk[256];
		int k = 0;

		while (i < nlost && k < 256) {
			if (lost[i])
				pk[k++] = (odp_packet_t)(uintptr_t)lost[i];
			i++;
		}
		odp_packet_free_multi(pk, k);
	}
	for (uint32_t s = 0; s < nslots; s++) {
		const uint64_t used = out->vec_used[s] < vhave[s] ? out->vec_used[s] : vhave[s];

		if (used < vhave[s])
			rt_packet_return_raw(vpools[s], (const odp_packet_t *)(const void *)(vgot + vbase[s] + used),
					     (int)(vhave[s] - used));
	}
	return events;
}

odp_pktio_t odp_pktio_lookup(const char *name)
{
	for (int i = 0; i < RT_MAX_PKTIO; i++)
		if (PK[i].used && name && strcmp(PK[i].name, name) == 0)
			return PK[i].hdl;
	return ODP_PKTIO_INVALID;
}

int odp_pktio_capability(odp_pktio_t h, odp_pktio_capability_t *c)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || !c)
		return -1;
	memset(c, 0, sizeof(*c));
	/* loop.c:672-684: one loop queue per input queue, flows spread over them
	 * by the pktin hash; their size is configurable in DIRECT mode */
	c->max_input_queues = e->drv == DRV_LOOP ? ODP_PKTIN_MAX_QUEUES : 1;
	c->max_output_queues = e->drv == DRV_LOOP ? ODP_PKTOUT_MAX_QUEUES : 1;
	c->min_input_queue_size = e->drv == DRV_LOOP ? 1 : 0;
	c->max_input_queue_size = e->drv == DRV_LOOP ? RT_LOOP_MAX_QUEUE_SIZE : 0;
	c->max_output_queue_size = 0;
	c->stats.pktio.counter.in_octets = 1;
	c->stats.pktio.counter.in_packets = 1;
	c->stats.pktio.counter.in_errors = 1;
	c->stats.pktio.counter.in_discards = 1;
	c->stats.pktio.counter.out_octets = 1;
	c->stats.pktio.counter.out_packets = 1;
	if (e->drv == DRV_LOOP) {   /* loop.c:723-728 */
		c->stats.pktin_queue.counter.octets = 1;
		c->stats.pktin_queue.counter.packets = 1;
		c->stats.pktin_queue.counter.errors = 1;
		c->stats.pktin_queue.counter.discards = 1;
		c->stats.pktout_queue.counter.octets = 1;
		c->stats.pktout_queue.counter.packets = 1;
	}
	odp_pktio_config_init(&c->config);
	c->config.parser.layer = ODP_PROTO_LAYER_ALL;
	c->config.pktin.all_bits = RT_PKTIN_OPT_MASK;
	/* loop.c:694-715: checksum insertion (and the per-packet override
	 * enables) on the loop pktio; the pcap driver has no such offload */
	c->config.pktout.all_bits = e->drv == DRV_LOOP ? RT_PKTOUT_OPT_MASK : 0;
	c->config.enable_loop = 0;
	c->set_op.op.promisc_mode = e->drv == DRV_PCAP;
	c->maxlen.equal = 1;
	c->maxlen.min_input = c->maxlen.min_output = 68 + 14;
	c->maxlen.max_input = c->maxlen.max_output = 65535;
	c->loop_supported = ODP_SUPPORT_NO;
	/* odp_packet_io.c:1566-1577: the same for every driver; packets of this
	 * runtime have one segment */
	c->lso.max_profiles = MI_CLS_LSO_PROFILES;
	c->lso.max_profiles_per_pktio = MI_CLS_LSO_PROFILES;
	c->lso.max_packet_segments = 1;
	c->lso.max_segments = MI_CLS_LSO_MAX_SEGMENTS;
	c->lso.max_payload_len = odp_pktio_mtu(h) - 14;
	c->lso.max_payload_offset = MI_CLS_LSO_MAX_PAYLOAD_OFFSET;
	c->lso.mod_op.add_segment_num = 1;
	c->lso.mod_op.write_bits = 1;
	c->lso.max_num_custom = ODP_LSO_MAX_CUSTOM;
	c->lso.proto.ipv4 = 1;
	c->lso.proto.custom = 1;
	return 0;
}

int odp_pktio_config(odp_pktio_t h, const odp_pktio_config_t *config)
{
	rt_pktio_t *e = get_pk(h);
	odp_pktio_config_t def;

	if (!e)
		return -1;
	if (!config) {
		odp_pktio_config_init(&def);
		config = &def;
	}
	/* parser options, pktin checksum validation and drop-on-error options
	 * (bits 2-10), pktout checksum insertion on a loop pktio (bits 1-8); no
	 * timestamps, other pktout offloads or IPsec; enable_lso is accepted
	 * (LSO is common code over every driver, odp_packet_io.c:3305) */
	if ((config->pktin.all_bits & ~RT_PKTIN_OPT_MASK) ||
	    (config->pktout.all_bits & ~(e->drv == DRV_LOOP ? RT_PKTOUT_OPT_MASK : 0ull)) ||
	    config->enable_loop || config->inbound_ipsec || config->outbound_ipsec) {
		RT_ERR("pktio %s: unsupported configuration option\n", e->name);
		return -1;
	}
	if (e->state == ST_STARTED)
		return -1;
	e->config = *config;
	return 0;
}

int odp_pktin_queue_config(odp_pktio_t h, const odp_pktin_queue_param_t *param)
{
	rt_pktio_t *e = get_pk(h);
	odp_pktin_queue_param_t def;

	if (!e || e->state == ST_STARTED)
		return -1;
	if (!param) {
		odp_pktin_queue_param_init(&def);
		param = &def;
	}
	if (e->param.in_mode == ODP_PKTIN_MODE_DISABLED)
		return -1;
	/* odp_packet_io.c:1984-2014: the classifier delivers by CoS, so with it
	 * the driver has one input queue whatever num_queues says */
	odp_pktio_capability_t capa;
	const uint32_t nq = param->classifier_enable ? 1 : param->num_queues;
	const int direct = e->param.in_mode == ODP_PKTIN_MODE_DIRECT;

	if (odp_pktio_capability(h, &capa))
		return -1;
	if (nq == 0 || nq > capa.max_input_queues) {
		RT_ERR("pktio %s: %u input queues requested, 1 .. %u supported\n", e->name,
		       param->num_queues, capa.max_input_queues);
		return -1;
	}
	for (uint32_t i = 0; i < nq && direct; i++) {   /* :2017-2036 */
		const uint32_t qs = param->queue_size[i];

		if (qs && (qs < capa.min_input_queue_size || qs > capa.max_input_queue_size)) {
			RT_ERR("pktio %s: input queue size %u not supported\n", e->name, qs);
			return -1;
		}
	}
	if (param->vector.enable) {
		RT_ERR("pktio %s: packet vectors are not supported\n", e->name);
		return -1;
	}
	/* a re-configuration may change the queue count: no burst of the old
	 * queues stays behind, and the loop queues are made anew (loop.c:172-227) */
	odp_spinlock_lock(&e->rxl);
	for (uint32_t i = 0; i < ODP_PKTIN_MAX_QUEUES; i++)
		queue_drain_destroy(&e->inq[i]);
	e->inq_param = *param;
	e->inq_param.num_queues = nq;
	e->inq_param.queue_param_ovr = NULL;   /* the caller's array: used below only */
	e->cls_enabled = param->classifier_enable;
	e->num_in = 0;
	e->hash_proto = param->hash_enable ? param->hash_proto.all_bits & 63u : 0;
	if (e->drv == DRV_LOOP && loopqs_create(e, nq, direct ? param->queue_size : NULL)) {
		odp_spinlock_unlock(&e->rxl);
		return -1;
	}
	for (uint32_t i = 0; i < nq && !direct; i++) {   /* :2093-2140 */
		odp_queue_param_t qp;
		char qn[ODP_QUEUE_NAME_LEN];

		/* a queue count the classifier forced to 1: the default queue, as
		 * the reference gives every classifier pktin queue (:2109-2110);
		 * a classifier config that asked for one queue keeps its
		 * queue_param, as before */
		if (param->classifier_enable && nq != param->num_queues) {
			odp_queue_param_init(&qp);
		} else {
			qp = param->queue_param;
			if (!param->classifier_enable && param->queue_param_ovr)
				qp.sched.group = param->queue_param_ovr[i].group;
		}
		qp.type = e->param.in_mode == ODP_PKTIN_MODE_SCHED ? ODP_QUEUE_TYPE_SCHED
								    : ODP_QUEUE_TYPE_PLAIN;
		snprintf(qn, sizeof(qn), "odp-pktin-%d-%u", (int)((uintptr_t)h - 1), i);
		e->inq[i] = odp_queue_create(qn, &qp);
		if (e->inq[i] == ODP_QUEUE_INVALID) {
			while (i--)
				queue_drain_destroy(&e->inq[i]);
			odp_spinlock_unlock(&e->rxl);
			return -1;
		}
		if (e->param.in_mode == ODP_PKTIN_MODE_QUEUE)
			((rt_queue_t *)(void *)e->inq[i])->pktin_idx = (int)(uintptr_t)h;
	}
	e->num_in = nq;
	e->inq_configured = 1;
	odp_spinlock_unlock(&e->rxl);
	return 0;
}

int odp_pktout_queue_config(odp_pktio_t h, const odp_pktout_queue_param_t *param)
{
	rt_pktio_t *e = get_pk(h);
	odp_pktio_capability_t c;

	if (!e || e->state == ST_STARTED || odp_pktio_capability(h, &c))
		return -1;
	uint32_t n = param ? param->num_queues : 1;

	if (n == 0 || n > c.max_output_queues)
		return -1;
	e->num_out = n;
	return 0;
}

int odp_pktin_queue(odp_pktio_t h, odp_pktin_queue_t q[], int num)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || e->param.in_mode != ODP_PKTIN_MODE_DIRECT)
		return -1;
	const int nq = e->num_in ? (int)e->num_in : 1;

	for (int i = 0; q && i < num && i < nq; i++) {
		q[i].q = (_odp_pktin_hdl_t)(uintptr_t)h;
		q[i].index = i;
		q[i].pktio = h;
	}
	return nq;
}

int odp_pktin_event_queue(odp_pktio_t h, odp_queue_t q[], int num)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || (e->param.in_mode != ODP_PKTIN_MODE_SCHED &&
		   e->param.in_mode != ODP_PKTIN_MODE_QUEUE))
		return -1;
	int nq = 0;

	while (nq < ODP_PKTIN_MAX_QUEUES && e->inq[nq] != ODP_QUEUE_INVALID)
		nq++;
	for (int i = 0; q && i < num && i < nq; i++)
		q[i] = e->inq[i];
	return nq;
}

int odp_pktout_queue(odp_pktio_t h, odp_pktout_queue_t q[], int num)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || e->param.out_mode != ODP_PKTOUT_MODE_DIRECT)
		return -1;
	if (!e->num_out)
		e->num_out = 1;
	for (int i = 0; i < num && (uint32_t)i < e->num_out; i++) {
		q[i].q = (void *)(uintptr_t)h;
		q[i].index = i;
		q[i].pktio = h;
	}
	return (int)e->num_out;
}

int odp_pktio_start(odp_pktio_t h)
{
	rt_pktio_t *e = get_pk(h);

	if (!e)
		return -1;
	if (e->state == ST_STARTED) {
		RT_ERR("Already started\n");
		return -1;
	}
	if (!e->inq_configured && e->param.in_mode != ODP_PKTIN_MODE_DISABLED &&
	    odp_pktin_queue_config(h, NULL))
		return -1;
	/* odp_packet_io.c:675-677 */
	e->parse_layer = e->cls_enabled ? ODP_PROTO_LAYER_ALL : e->config.parser.layer;
	/* GPU context, rule snapshot and a warm-up launch before traffic */
	if (e->param.in_mode != ODP_PKTIN_MODE_DISABLED && e->parse_layer != ODP_PROTO_LAYER_NONE) {
		/* the options of the layers that are parsed: L3 takes the IPv4
		 * header checksum and the IP drops, L4 everything (odp_parse.c:
		 * 372-414 stop before the rest) */
		uint64_t opt = e->config.pktin.all_bits & RT_PKTIN_OPT_MASK;

		if (e->parse_layer < ODP_PROTO_LAYER_L3)
			opt = 0;
		else if (e->parse_layer == ODP_PROTO_LAYER_L3)
			opt &= (1u << 2) | (1u << 6) | (1u << 7);
		odp_amd_cls_pktin_opt_set(h, opt);
		/* receive calls classify bursts of at most rx_burst() frames */
		odp_amd_cls_batch_hint(h, rx_burst());
		int rc = odp_amd_cls_prepare(h, !e->cls_enabled);

		if (rc) {
			RT_ERR("pktio %s: GPU receive path unavailable (%s)\n", e->name,
			       mi_cls_strerror(rc));
			return -1;
		}
		/* the burst sets' page-locked arrays too: made here, not by the
		 * first bursts (each page-locked allocation is a runtime call) */
		for (int k = 0; k < RX_SETS; k++)
			(void)stage_reserve(&e->rs[k], rx_burst(), 0);
		/* Rule load is control plane (odp_packet_io.c:650-705 does its
		 * setup here too): wait for the program-specialised kernel of the
		 * rules in place now (1-2 s of compile, cached per program for the
		 * process), so the first bursts do not run the generic classifier
		 * (a short capture used to finish before the compile did).
		 * ODP_AMD_SPEC_WAIT=0 starts without waiting. */
		if (e->cls_enabled) {
			const char *w = getenv("ODP_AMD_SPEC_WAIT");

			if (!(w && w[0] == '0'))
				(void)odp_amd_cls_spec_wait(h);
		}
	}
	/* pktout checksum insertion configured: its GPU context before traffic,
	 * also when the input side needs none */
	if (e->drv == DRV_LOOP && ((e->config.pktout.all_bits & RT_PKTOUT_OPT_MASK) ||
				   (e->hash_proto && e->num_in > 1))) {
		int rc = odp_amd_cls_chksum_insert_host(h, NULL, 0, NULL, NULL, NULL, 0, 0, NULL);

		if (rc) {
			RT_ERR("pktio %s: GPU transmit path unavailable (%s)\n", e->name,
			       mi_cls_strerror(rc));
			return -1;
		}
	}
	e->state = ST_STARTED;
	if (e->param.in_mode == ODP_PKTIN_MODE_SCHED) {
		odp_spinlock_lock(&pk_lock);
		sched_list[num_sched_pktio++] = (int)((uintptr_t)h - 1);
		odp_spinlock_unlock(&pk_lock);
	}
	return 0;
}

static void sched_list_remove(int idx)
{
	odp_spinlock_lock(&pk_lock);
	for (int i = 0; i < num_sched_pktio; i++)
		if (sched_list[i] == idx) {
			sched_list[i] = sched_list[--num_sched_pktio];
			break;
		}
	odp_spinlock_unlock(&pk_lock);
}

int odp_pktio_stop(odp_pktio_t h)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || e->state != ST_STARTED) {
		RT_ERR("Not started\n");
		return -1;
	}
	sched_list_remove((int)((uintptr_t)h - 1));
	odp_spinlock_lock(&e->rxl);   /* wait for an in-flight burst */
	rx_drain(e);
	e->state = ST_STOPPED;
	odp_spinlock_unlock(&e->rxl);
	return 0;
}

int odp_pktio_close(odp_pktio_t h)
{
	rt_pktio_t *e = get_pk(h);

	if (!e)
		return -1;
	if (e->state == ST_STARTED) {
		RT_ERR("pktio %s: close while started\n", e->name);
		return -1;
	}
	if (rx_prof > 0 && e->prof[3]) {
		/* the instantiation of the pktio's last classification launch:
		 * word 4 = program-specialised */
		uint32_t li[MI_CLS_LAUNCH_INFO_WORDS] = { 0 };

		(void)odp_amd_cls_last_launch(h, li, MI_CLS_LAUNCH_INFO_WORDS);
		fprintf(stderr, "RXSPEC %s %u\n", e->name, li[4]);
	}
	if (rx_prof > 0 && e->prof[3])
		fprintf(stderr, "RXPROF %s bursts %" PRIu64 " stage_ns %" PRIu64 " classify_ns %" PRIu64
			" deliver_ns %" PRIu64 " (prepare_ns %" PRIu64 " enqueue_ns %" PRIu64
			" alloc_tsc %" PRIu64 " copy_tsc %" PRIu64 ") gpu_bursts %" PRIu64
			" (decide_ns %" PRIu64 " submit_ns %" PRIu64 " kernel_ns %" PRIu64 " enqueue_ns %" PRIu64
			") chain_submit_ns %" PRIu64 " chain_bursts %" PRIu64 " chain_redo %" PRIu64 "\n", e->name,
			e->prof[3], e->prof[0], e->prof[1], e->prof[2], e->prof[4], e->prof[5], e->prof[6],
			e->prof[7], e->prof[11], e->prof[8], e->prof[12], e->prof[9], e->prof[10], e->prof[13],
			e->prof[14], e->prof[15]);
	for (uint32_t i = 0; i < ODP_PKTIN_MAX_QUEUES; i++) {
		queue_drain_destroy(&e->inq[i]);
		queue_drain_destroy(&e->loopq[i]);
	}
	if (e->tx)
		fclose(e->tx);
	store_free(e);
	rx_sets_free(e);
	tx_free(e);
	odp_spinlock_lock(&pk_lock);
	memset(e, 0, sizeof(*e));
	odp_spinlock_unlock(&pk_lock);
	return odp_amd_cls_pktio_destroy(h);
}

/* ============================================================ misc */
int odp_pktio_promisc_mode(odp_pktio_t h)
{
	rt_pktio_t *e = get_pk(h);

	if (!e)
		return -1;
	return e->drv == DRV_PCAP ? e->promisc : 1;
}

int odp_pktio_promisc_mode_set(odp_pktio_t h, odp_bool_t enable)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || e->drv != DRV_PCAP || e->state == ST_STARTED)
		return -1;
	e->promisc = enable;
	return 0;
}

int odp_pktio_mac_addr(odp_pktio_t h, void *mac, int size)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || size < 6)
		return -1;
	memcpy(mac, e->drv == DRV_PCAP ? pcap_mac : loop_mac, 6);
	return 6;
}

uint32_t odp_pktio_mtu(odp_pktio_t h)
{
	rt_pktio_t *e = get_pk(h);

	return e ? (e->drv == DRV_PCAP ? PCAP_MTU_MAX : 9216) : 0;
}

int odp_pktio_stats(odp_pktio_t h, odp_pktio_stats_t *s)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || !s)
		return -1;
	memset(s, 0, sizeof(*s));
	s->in_octets = odp_atomic_load_u64(&e->in_octets);
	s->in_packets = odp_atomic_load_u64(&e->in_packets);
	s->in_discards = odp_atomic_load_u64(&e->in_discards);
	s->in_errors = odp_atomic_load_u64(&e->in_errors);
	s->out_octets = odp_atomic_load_u64(&e->out_octets);
	s->out_packets = odp_atomic_load_u64(&e->out_packets);
	s->out_discards = odp_atomic_load_u64(&e->out_discards);
	return 0;
}

int odp_pktio_stats_reset(odp_pktio_t h)
{
	rt_pktio_t *e = get_pk(h);

	if (!e)
		return -1;
	odp_atomic_init_u64(&e->in_octets, 0);
	odp_atomic_init_u64(&e->in_packets, 0);
	odp_atomic_init_u64(&e->in_discards, 0);
	odp_atomic_init_u64(&e->in_errors, 0);
	odp_atomic_init_u64(&e->out_octets, 0);
	odp_atomic_init_u64(&e->out_packets, 0);
	odp_atomic_init_u64(&e->out_discards, 0);
	for (int i = 0; i < ODP_PKTIN_MAX_QUEUES; i++) {
		odp_atomic_init_u64(&e->inq_st[i].octets, 0);
		odp_atomic_init_u64(&e->inq_st[i].packets, 0);
		odp_atomic_init_u64(&e->inq_st[i].discards, 0);
		odp_atomic_init_u64(&e->inq_st[i].errors, 0);
	}
	for (int i = 0; i < ODP_PKTOUT_MAX_QUEUES; i++) {
		odp_atomic_init_u64(&e->outq_st[i].octets, 0);
		odp_atomic_init_u64(&e->outq_st[i].packets, 0);
	}
	return 0;
}

/* Per-queue counters (odp_packet_io.c:2390-2470 over loop.c:781-805) */
static int pktin_stats_of(rt_pktio_t *e, int idx, odp_pktin_queue_stats_t *s)
{
	if (!e || !s || idx < 0 || (uint32_t)idx >= (e->num_in ? e->num_in : 1u))
		return -1;
	memset(s, 0, sizeof(*s));
	s->octets = odp_atomic_load_u64(&e->inq_st[idx].octets);
	s->packets = odp_atomic_load_u64(&e->inq_st[idx].packets);
	s->discards = odp_atomic_load_u64(&e->inq_st[idx].discards);
	s->errors = odp_atomic_load_u64(&e->inq_st[idx].errors);
	return 0;
}

int odp_pktin_queue_stats(odp_pktin_queue_t q, odp_pktin_queue_stats_t *s)
{
	rt_pktio_t *e = get_pk(q.pktio);

	if (!e || e->param.in_mode != ODP_PKTIN_MODE_DIRECT)
		return -1;
	return pktin_stats_of(e, q.index, s);
}

int odp_pktin_event_queue_stats(odp_pktio_t h, odp_queue_t queue, odp_pktin_queue_stats_t *s)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || queue == ODP_QUEUE_INVALID ||
	    (e->param.in_mode != ODP_PKTIN_MODE_SCHED && e->param.in_mode != ODP_PKTIN_MODE_QUEUE))
		return -1;
	for (int i = 0; i < ODP_PKTIN_MAX_QUEUES; i++)
		if (e->inq[i] == queue)
			return pktin_stats_of(e, i, s);
	return -1;
}

int odp_pktout_queue_stats(odp_pktout_queue_t q, odp_pktout_queue_stats_t *s)
{
	rt_pktio_t *e = get_pk(q.pktio);

	if (!e || !s || e->param.out_mode != ODP_PKTOUT_MODE_DIRECT || q.index < 0 ||
	    (uint32_t)q.index >= (e->num_out ? e->num_out : 1u))
		return -1;
	memset(s, 0, sizeof(*s));
	s->octets = odp_atomic_load_u64(&e->outq_st[q.index].octets);
	s->packets = odp_atomic_load_u64(&e->outq_st[q.index].packets);
	return 0;
}

int odp_pktio_info(odp_pktio_t h, odp_pktio_info_t *info)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || !info)
		return -1;
	info->name = e->name;
	info->drv_name = e->drv == DRV_PCAP ? "pcap" : e->drv == DRV_LOOP ? "loop" : "null";
	info->pool = e->pool;
	info->param = e->param;
	return 0;
}

int odp_pktio_index(odp_pktio_t h)
{
	return get_pk(h) ? (int)((uintptr_t)h - 1) : -1;
}

uint64_t odp_pktio_to_u64(odp_pktio_t h)
{
	return (uint64_t)(uintptr_t)h;
}

void odp_pktio_print(odp_pktio_t h)
{
	rt_pktio_t *e = get_pk(h);
	odp_pktio_stats_t s;

	if (!e)
		return;
	odp_pktio_stats(h, &s);
	printf("Pktio info\n----------\n  name            %s\n  driver          %s\n"
	       "  classifier      %s\n  frames (pcap)   %u\n  in_packets      %" PRIu64 "\n"
	       "  in_errors       %" PRIu64 "\n  in_discards     %" PRIu64 "\n\n", e->name,
	       e->drv == DRV_PCAP ? "pcap" : e->drv == DRV_LOOP ? "loop" : "null",
	       e->cls_enabled ? "enabled (GPU)" : "disabled", e->fs.n, s.in_packets,
	       s.in_errors, s.in_discards);
}

/* Build extension: send calls of the pktio that ran the pktout checksum
 * kernel, and how many of them went through the bounce buffer. */
int odp_amd_pktio_tx_stats(odp_pktio_t h, uint64_t *bursts, uint64_t *bounced)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || !bursts || !bounced)
		return -1;
	pthread_mutex_lock(&e->txl);
	*bursts = e->txg.bursts;
	*bounced = e->txg.bounced;
	pthread_mutex_unlock(&e->txl);
	return 0;
}

/* Build extension: of those send calls, the ones whose launch also computed
 * the pktin flow hash (several hashed input queues). */
int odp_amd_pktio_txq_stats(odp_pktio_t h, uint64_t *hashed)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || !hashed)
		return -1;
	pthread_mutex_lock(&e->txl);
	*hashed = e->txq_bursts;
	pthread_mutex_unlock(&e->txl);
	return 0;
}
