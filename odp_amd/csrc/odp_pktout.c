/*
 * odp_pktout.c -- the transmit side of the "loop", "pcap" and "null" pktios
 * and the stand-alone odp_packet_parse: the host batches (gather_*) that
 * pktout checksum insertion, LSO and odp_packet_parse_multi hand to their
 * kernels, the loop queue pick over several input queues (odp_txq.h),
 * odp_pktout_send and odp_pktout_send_lso.
 *
 * Reference behaviour:
 *   platform/linux-generic/pktio/loop.c:422-598   loopback_fix_checksums,
 *                                                 get_dest_queue, loopback_send
 *   platform/linux-generic/pktio/pcap.c:354-401   _pcapif_dump_pkt, pcapif_send_pkt
 *   platform/linux-generic/odp_packet_io.c:2837-3400  LSO profiles and
 *                                                 odp_pktout_send_lso
 */
#define _GNU_SOURCE
#include <errno.h>
#include <string.h>

#include "odp_pktio_internal.h"
#include "odp_txq.h"

/* ============================================================ transmit */
/* The gather of an offload call (gather_t), stated once for its three
 * callers.  A call's descriptors are built in page-locked arrays carved out
 * of one allocation.  Its frames are worked on in place where every piece
 * lies in the page-locked arena (rt_pinned_arena; below OOB_SPAN, so that
 * arena-relative offsets stay under the kernels' out-of-range offset), in a
 * page-locked pool, with `slack` readable bytes behind it; a call with one
 * piece elsewhere (pageable pools) goes whole through a page-locked bounce
 * buffer, its pieces at 64-B steps.
 *   minimum capacity:  checksum 4096 packets, parse 1024, LSO 64 sources
 *   slack:             checksum and parse 16 B (their kernels read frames in
 *                      16-B pieces), LSO sources and segments 0
 *   length clamp:      checksum and parse 65535 (GATHER_LEN_MAX); LSO plans
 *                      no longer packet
 *   refused:           a bounce layout of OOB_SPAN or more (-E2BIG), no
 *                      memory (-ENOMEM); checksum and parse report both as
 *                      their plain failure
 *   copied back:       checksum every frame, parse nothing, LSO the segments
 *                      of the packets with st == OK
 * Everything here runs under the caller's lock (txl, PRS.lock). */
#define GATHER_LEN_MAX 65535u

/* Begin a call of n entries, `per` bytes of arrays each: g->arr holds g->cap
 * (>= n, >= min_cap) entries of every array.  0, or -ENOMEM. */
static int gather_begin(gather_t *g, uint32_t n, size_t per, uint32_t min_cap)
{
	if (n > g->cap) {
		const size_t cap = n < min_cap ? min_cap : (size_t)n + n / 2;

		hmem_free(g->arr, g->pinned);
		g->cap = 0;
		g->arr = hmem_alloc(cap * per, &g->pinned);
		if (!g->arr)
			return -ENOMEM;
		g->cap = (uint32_t)cap;
	}
	g->lo = NULL;
	g->span = g->bytes = 0;
	g->in_place = g->pinned && rt_pinned_arena(&g->lo, &g->span) && g->span < OOB_SPAN;
	return 0;
}

static inline int pkt_pool_pinned(const pkt_hdr_t *h)
{
	const rt_pool_t *rp = rt_pool((odp_pool_t)(uintptr_t)(h->ev.pool + 1u));

	return rp && rp->pinned;
}

/* Place a piece: its arena-relative offset, or the call drops to the bounce
 * path (and gather_step gives the offset). */
static inline uint32_t gather_place(gather_t *g, const uint8_t *d, uint32_t len, uint32_t slack, int pool_pinned)
{
	g->bytes += (len + 63u) & ~63u;
	if (g->in_place && pool_pinned && d >= g->lo && (size_t)(d - g->lo) + len + slack <= g->span)
		return (uint32_t)(d - g->lo);
	g->in_place = 0;
	return 0;
}

/* After the last piece, g->base / g->bytes for the GPU entry: 0 in place; 1
 * through the bounce buffer, reserved here, where the caller now lays its
 * pieces out in the order it placed them (gather_step); or < 0. */
static int gather_layout(gather_t *g)
{
	if (g->in_place) {
		g->base = g->lo;
		g->bytes = g->span;
		return 0;
	}
	g->bytes += 64;
	if (g->bytes >= OOB_SPAN)
		return -E2BIG;
	if (g->bytes > g->stage_cap) {
		hmem_free(g->stage, g->stage_pinned);
		g->stage_cap = 0;
		g->stage = hmem_alloc(g->bytes + g->bytes / 2, &g->stage_pinned);
		if (!g->stage)
			return -ENOMEM;
		g->stage_cap = g->bytes + g->bytes / 2;
	}
	g->base = g->stage;
	g->pos = 0;
	return 1;
}

static inline uint32_t gather_step(gather_t *g, uint32_t len)
{
	const size_t off = g->pos;

	g->pos += (len + 63u) & ~63u;
	return (uint32_t)off;
}

/* The call's kernel ran */
static inline void gather_ran(gather_t *g)
{
	g->bursts++;
	g->bounced += !g->in_place;
}

static void gather_free(gather_t *g)
{
	hmem_free(g->arr, g->pinned);
	hmem_free(g->stage, g->stage_pinned);
	memset(g, 0, sizeof(*g));
}

void tx_free(rt_pktio_t *e)
{
	gather_free(&e->txg);
	gather_free(&e->lsog);
	pthread_mutex_destroy(&e->txl);
}

/* pktout checksum insertion of a send burst on a loop pktio
 * (loopback_fix_checksums for every packet, pktio/loop.c:422-472, 581) on the
 * GPU: nothing when no default is configured and no packet carries an
 * override that asks for a checksum (no GPU call).  Otherwise the packets'
 * descriptors are built in page-locked memory -- the data address relative to
 * the page-locked arena, as the receive chain's, the length, the l3 / l4
 * offsets and the override bits of the header -- and the kernel works on the
 * frames in place; a burst with a packet outside the arena (pageable pools)
 * goes through a page-locked bounce buffer.  Waits for the kernel.  The
 * packets' override bits stay as they are (a packet the loop queue does not
 * take goes back to the application with them): the loop receive resets them
 * (packet_parse_reset(.., 1), loop.c:308).  0, or -1.
 *
 * dst != NULL (several input queues): dst[i] becomes the loop queue of packet
 * i (get_dest_queue, loop.c:479-530, 582).  With the pktin hash off that is
 * host arithmetic and nothing above changes.  With it on, the call's one
 * launch also computes every packet's flow hash (mi_cls_tx_hash_host: the
 * hash alone when nothing asks for a checksum, writing no frame byte): the
 * descriptors then carry the packet's has_udp / tcp / ipv4 / ipv6 flags, the
 * hash words are one more page-locked array of the gather, and the modulo
 * is taken here. */
static int tx_chksum(rt_pktio_t *e, const odp_packet_t pkts[], int num, uint8_t *dst, uint32_t index)
{
	const uint64_t opt = RT_PKTOUT_TX_WORD(e->config.pktout.all_bits);
	const uint32_t hp = dst ? e->hash_proto : 0;
	int want = (opt & RT_PKTOUT_TX_CK) != 0;

	for (int i = 0; !want && i < num; i++) {
		const uint32_t f = rt_pkt_hdr(pkts[i])->tx_ck;

		want |= (f & (MI_CLS_TXF_L3_SET | MI_CLS_TXF_L3)) == (MI_CLS_TXF_L3_SET | MI_CLS_TXF_L3) ||
			(f & (MI_CLS_TXF_L4_SET | MI_CLS_TXF_L4)) == (MI_CLS_TXF_L4_SET | MI_CLS_TXF_L4);
	}
	if (!hp && dst)
		txq_pick(NULL, (uint32_t)num, index, e->num_in, dst);
	if (!want && !hp)
		return 0;
	const uint32_t n = (uint32_t)num;
	int rc = -1;

	gather_t *g = &e->txg;

	pthread_mutex_lock(&e->txl);
	if (gather_begin(g, n, sizeof(mi_cls_tx_desc_t) + 2 * sizeof(uint32_t) + sizeof(uint16_t), 4096))
		goto out;
	mi_cls_tx_desc_t *desc = (mi_cls_tx_desc_t *)(void *)g->arr;
	uint32_t *off = (uint32_t *)(void *)(desc + g->cap);
	uint32_t *hash = off + g->cap;
	uint16_t *len = (uint16_t *)(void *)(hash + g->cap);

	for (uint32_t i = 0; i < n; i++) {
		const pkt_hdr_t *h = rt_pkt_hdr(pkts[i]);
		/* input flags 13 / 14 / 22 / 23: has_ipv4 / ipv6 / udp / tcp */
		const uint32_t meta = !hp ? 0u
			: (((h->in_flags >> 22) & 1u) ? MI_CLS_TXF_UDP : 0u) |
			  (((h->in_flags >> 23) & 1u) ? MI_CLS_TXF_TCP : 0u) |
			  (((h->in_flags >> 13) & 1u) ? MI_CLS_TXF_IPV4 : 0u) |
			  (((h->in_flags >> 14) & 1u) ? MI_CLS_TXF_IPV6 : 0u);

		len[i] = (uint16_t)(h->len > GATHER_LEN_MAX ? GATHER_LEN_MAX : h->len);
		desc[i] = (mi_cls_tx_desc_t){ .l3 = h->l3, .l4 = h->l4,
					      .flags = (uint8_t)((h->tx_ck & 0xFu) | meta) };
		off[i] = gather_place(g, h->head + h->data_off, len[i], 16, pkt_pool_pinned(h));
	}
	const int bounce = gather_layout(g);

	if (bounce < 0)
		goto out;
	for (uint32_t i = 0; bounce && i < n; i++) {
		const pkt_hdr_t *h = rt_pkt_hdr(pkts[i]);

		off[i] = gather_step(g, len[i]);
		memcpy(g->stage + off[i], h->head + h->data_off, len[i]);
	}
	rc = hp ? odp_amd_cls_tx_hash_host(e->hdl, g->base, g->bytes, off, len, desc, n, opt, NULL, hp, hash,
					   want)
		: odp_amd_cls_chksum_insert_host(e->hdl, g->base, g->bytes, off, len, desc, n, opt, NULL);
	if (rc) {
		RT_ERR("pktio %s: pktout %s failed (%s)\n", e->name, hp ? "flow hash" : "checksum insertion",
		       mi_cls_strerror(rc));
		rc = -1;
		goto out;
	}
	if (hp) {
		txq_pick(hash, n, index, e->num_in, dst);
		e->txq_bursts++;
	}
	for (uint32_t i = 0; bounce && want && i < n; i++) {
		pkt_hdr_t *h = rt_pkt_hdr(pkts[i]);

		memcpy(h->head + h->data_off, g->stage + off[i], len[i]);
	}
	gather_ran(g);
out:
	pthread_mutex_unlock(&e->txl);
	return rc;
}

/* ============================================================ odp_packet_parse */
/* The descriptors, records and bounce buffer of odp_packet_parse_multi:
 * process-wide, as the parse context (odp_amd_cls_parse_host), one call at a
 * time; page-locked where there is a GPU; kept for the process's life. */
static struct {
	pthread_mutex_t lock;
	gather_t g;             /* arrays: records, offsets, lengths */
	int no_gpu_said;
} PRS = { .lock = PTHREAD_MUTEX_INITIALIZER };

/* odp_packet_parse_multi (odp_packet.c:2219-2229 over odp_packet_parse,
 * :2140-2217) with one kernel launch for the whole call: the packets'
 * descriptors -- the byte the parse starts at, relative to the page-locked
 * arena, and frame_len - offset -- are built in page-locked memory and the
 * kernel reads the frames in place; a call with a packet outside the arena
 * (pageable pools) goes through a page-locked bounce buffer, as tx_chksum
 * (nothing is copied back: a parse writes no frame byte).  Then, in order,
 * each packet is reset as packet_parse_reset(hdr, 0) and takes its record's
 * metadata, up to and including the first packet whose parse failed; the
 * packets after that one stay as they were (the reference's loop ends
 * there). */
int odp_packet_parse_multi(const odp_packet_t pkts[], const uint32_t offset[], int num,
			   const odp_packet_parse_param_t *param)
{
	if (num <= 0 || !param || param->proto == ODP_PROTO_NONE || param->last_layer == ODP_PROTO_LAYER_NONE)
		return 0;
	/* odp_packet_parse stops at a packet whose offset is past its data
	 * (packet_map returns NULL) before touching it: nothing from there on
	 * is parsed */
	uint32_t n = 0;

	while (n < (uint32_t)num && offset[n] < rt_pkt_hdr(pkts[n])->len)
		n++;
	if (n == 0)
		return 0;
	int done = 0;

	gather_t *g = &PRS.g;

	pthread_mutex_lock(&PRS.lock);
	if (gather_begin(g, n, sizeof(mi_cls_result_t) + sizeof(uint32_t) + sizeof(uint16_t), 1024))
		goto out;
	mi_cls_result_t *res = (mi_cls_result_t *)(void *)g->arr;
	uint32_t *off = (uint32_t *)(void *)(res + g->cap);
	uint16_t *len = (uint16_t *)(void *)(off + g->cap);

	for (uint32_t i = 0; i < n; i++) {
		const pkt_hdr_t *h = rt_pkt_hdr(pkts[i]);
		const uint32_t rest = h->len - offset[i];

		len[i] = (uint16_t)(rest > GATHER_LEN_MAX ? GATHER_LEN_MAX : rest);
		off[i] = gather_place(g, h->head + h->data_off + offset[i], len[i], 16, pkt_pool_pinned(h));
	}
	const int bounce = gather_layout(g);

	if (bounce < 0)
		goto out;
	for (uint32_t i = 0; bounce && i < n; i++) {
		const pkt_hdr_t *h = rt_pkt_hdr(pkts[i]);

		off[i] = gather_step(g, len[i]);
		memcpy(g->stage + off[i], h->head + h->data_off + offset[i], len[i]);
	}
	const int rc = odp_amd_cls_parse_host(g->base, g->bytes, off, len, n, (uint32_t)param->proto,
					      (uint32_t)param->last_layer, param->chksums.all_chksum & 0xFu, res);

	if (rc) {
		/* no CPU parser stands in (as odp_pktio_start without a GPU) */
		if (rc != -ENODEV || !PRS.no_gpu_said)
			RT_ERR("odp_packet_parse: GPU parse unavailable (%s)\n", mi_cls_strerror(rc));
		PRS.no_gpu_said |= rc == -ENODEV;
		goto out;
	}
	gather_ran(g);
	for (uint32_t i = 0; i < n; i++) {
		pkt_hdr_t *h = rt_pkt_hdr(pkts[i]);
		const mi_cls_result_t *r = &res[i];
		const uint32_t o = offset[i];

		/* packet_parse_reset(hdr, 0): the input flags and error bits are
		 * replaced whole; user_ptr and the pktout overrides (tx_ck) stay */
		h->in_flags = r->in_flags;
		h->err = r->err;
		h->l2 = param->proto == ODP_PROTO_ETH ? (uint16_t)o : ODP_PACKET_OFFSET_INVALID;
		h->l3 = r->l3_offset == 0xFFFFu ? ODP_PACKET_OFFSET_INVALID : (uint16_t)(r->l3_offset + o);
		h->l4 = r->l4_offset == 0xFFFFu ? ODP_PACKET_OFFSET_INVALID : (uint16_t)(r->l4_offset + o);
		if (r->outcome != MI_CLS_OUT_ENQ)
			break;
		done++;
	}
out:
	pthread_mutex_unlock(&PRS.lock);
	return done;
}

int odp_packet_parse(odp_packet_t pkt, uint32_t offset, const odp_packet_parse_param_t *param)
{
	return odp_packet_parse_multi(&pkt, &offset, 1, param) == 1 ? 0 : -1;
}

void odp_amd_packet_parse_stats(uint64_t *calls, uint64_t *bounced)
{
	pthread_mutex_lock(&PRS.lock);
	*calls = PRS.g.bursts;
	*bounced = PRS.g.bounced;
	pthread_mutex_unlock(&PRS.lock);
}

/* A send on a loop pktio with several input queues (loopback_send,
 * loop.c:554-598): the call's one launch (checksums, flow hash), then the
 * packets in arrival order as runs of equal destination queue, one enqueue
 * per run, up to the first run not taken whole.  The number of leading
 * packets sent; the others stay with the caller. */
struct loop_enq {
	rt_pktio_t *e;
	const odp_packet_t *pkts;
};

static int loop_enq_run(void *arg, uint32_t queue, uint32_t first, uint32_t count)
{
	const struct loop_enq *a = arg;

	return odp_queue_enq_multi(a->e->loopq[queue], (const odp_event_t *)(const void *)(a->pkts + first),
				   (int)count);
}

static int loop_send_queues(rt_pktio_t *e, uint32_t oq, const odp_packet_t pkts[], int num)
{
	uint8_t small[1024];
	uint8_t *dst = (size_t)num <= sizeof(small) ? small : malloc((size_t)num);
	struct loop_enq a = { e, pkts };
	int sent = -1;

	if (!dst)
		return -1;
	if (tx_chksum(e, pkts, num, dst, oq) == 0) {
		uint64_t octets = 0;

		sent = (int)txq_send_runs(dst, (uint32_t)num, loop_enq_run, &a);
		for (int i = 0; i < sent; i++)
			octets += odp_packet_len(pkts[i]);
		odp_atomic_add_u64(&e->out_packets, (uint64_t)sent);
		odp_atomic_add_u64(&e->out_octets, octets);
		odp_atomic_add_u64(&e->outq_st[oq].packets, (uint64_t)sent);
		odp_atomic_add_u64(&e->outq_st[oq].octets, octets);
	}
	if (dst != small)
		free(dst);
	return sent;
}

int odp_pktout_send(odp_pktout_queue_t q, const odp_packet_t pkts[], int num)
{
	rt_pktio_t *e = get_pk(q.pktio);

	if (!e || num < 0)
		return -1;
	if (e->state != ST_STARTED)
		return -1;
	const uint32_t oq = (uint32_t)q.index < ODP_PKTOUT_MAX_QUEUES ? (uint32_t)q.index : 0;

	if (e->drv == DRV_LOOP && e->num_in > 1 && num > 0)
		return loop_send_queues(e, oq, pkts, num);
	if (e->drv == DRV_LOOP && num > 0 && tx_chksum(e, pkts, num, NULL, 0))
		return -1;
	uint64_t octets = 0;

	for (int i = 0; i < num; i++)
		octets += odp_packet_len(pkts[i]);
	if (e->drv == DRV_LOOP) {
		int r = odp_queue_enq_multi(e->loopq[0], (const odp_event_t *)(const void *)pkts, num);

		if (r < 0)
			return -1;
		/* a sized loop queue may take fewer: only what was sent counts */
		for (int i = r; i < num; i++)
			octets -= odp_packet_len(pkts[i]);
		odp_atomic_add_u64(&e->out_packets, (uint64_t)r);
		odp_atomic_add_u64(&e->out_octets, octets);
		odp_atomic_add_u64(&e->outq_st[oq].packets, (uint64_t)r);
		odp_atomic_add_u64(&e->outq_st[oq].octets, octets);
		return r;
	}
	for (int i = 0; i < num; i++) {
		if (e->tx) {
			const pkt_hdr_t *p = rt_pkt_hdr(pkts[i]);

			pcap_dump_packet(e->tx, p->head + p->data_off, p->len);
		}
		odp_packet_free(pkts[i]);
	}
	odp_atomic_add_u64(&e->out_packets, (uint64_t)num);
	odp_atomic_add_u64(&e->out_octets, octets);
	odp_atomic_add_u64(&e->outq_st[oq].packets, (uint64_t)num);
	odp_atomic_add_u64(&e->outq_st[oq].octets, octets);
	return num;
}

/* ============================================================ LSO */
/* The LSO profiles (odp_packet_io.c:2837-2950: process-wide, PKTIO_LSO_PROFILES
 * slots, the handle a slot's address) and their form for the kernel. */
struct odp_lso_profile_s {
	int used;
	odp_lso_profile_param_t param;
};

static struct {
	pthread_mutex_t lock;
	struct odp_lso_profile_s prof[MI_CLS_LSO_PROFILES];
	uint32_t num;
	int not_started_said;
} LSO = { .lock = PTHREAD_MUTEX_INITIALIZER };

void odp_lso_profile_param_init(odp_lso_profile_param_t *param)
{
	memset(param, 0, sizeof(*param));
	param->lso_proto = ODP_LSO_PROTO_NONE;
}

/* a valid handle's slot index, or -1 */
static int lso_slot(odp_lso_profile_t h)
{
	if (h < &LSO.prof[0] || h >= &LSO.prof[MI_CLS_LSO_PROFILES] ||
	    ((uintptr_t)h - (uintptr_t)&LSO.prof[0]) % sizeof(LSO.prof[0]))
		return -1;
	return (int)(h - &LSO.prof[0]);
}

odp_lso_profile_t odp_lso_profile_create(odp_pktio_t pktio, const odp_lso_profile_param_t *param)
{
	(void)pktio;
	if (!param)
		return ODP_LSO_PROFILE_INVALID;
	/* :2850-2893 */
	if (param->lso_proto != ODP_LSO_PROTO_IPV4 && param->lso_proto != ODP_LSO_PROTO_CUSTOM) {
		RT_ERR("LSO protocol %d not supported\n", (int)param->lso_proto);
		return ODP_LSO_PROFILE_INVALID;
	}
	if (param->lso_proto == ODP_LSO_PROTO_CUSTOM) {
		if (param->custom.num_custom > ODP_LSO_MAX_CUSTOM)
			return ODP_LSO_PROFILE_INVALID;
		for (uint32_t i = 0; i < param->custom.num_custom; i++) {
			const uint32_t op = param->custom.field[i].mod_op, size = param->custom.field[i].size;

			if (param->custom.field[i].offset > MI_CLS_LSO_MAX_PAYLOAD_OFFSET)
				return ODP_LSO_PROFILE_INVALID;
			if (op == ODP_LSO_WRITE_BITS ? size != 1 : op != ODP_LSO_ADD_SEGMENT_NUM)
				return ODP_LSO_PROFILE_INVALID;
			if (size != 1 && size != 2 && size != 4 && size != 8)
				return ODP_LSO_PROFILE_INVALID;
		}
	}
	odp_lso_profile_t h = ODP_LSO_PROFILE_INVALID;

	pthread_mutex_lock(&LSO.lock);
	for (uint32_t i = 0; LSO.num < MI_CLS_LSO_PROFILES && i < MI_CLS_LSO_PROFILES; i++) {
		if (!LSO.prof[i].used) {
			LSO.prof[i].used = 1;
			LSO.prof[i].param = *param;
			LSO.num++;
			h = &LSO.prof[i];
			break;
		}
	}
	pthread_mutex_unlock(&LSO.lock);
	if (h == ODP_LSO_PROFILE_INVALID)
		RT_ERR("all %u LSO profiles are in use\n", MI_CLS_LSO_PROFILES);
	return h;
}

int odp_lso_profile_destroy(odp_lso_profile_t h)
{
	const int i = lso_slot(h);
	int rc = -1;

	if (i < 0)
		return -1;
	pthread_mutex_lock(&LSO.lock);
	if (LSO.prof[i].used) {
		LSO.prof[i].used = 0;
		LSO.num--;
		rc = 0;
	}
	pthread_mutex_unlock(&LSO.lock);
	return rc;
}

/* :2952-2983 */
int odp_packet_lso_request(odp_packet_t pkt, const odp_packet_lso_opt_t *o)
{
	pkt_hdr_t *h = rt_pkt_hdr(pkt);
	const int i = o ? lso_slot(o->lso_profile) : -1;

	if (i < 0 || !LSO.prof[i].used) {
		RT_ERR("bad LSO profile handle\n");
		return -1;
	}
	if (o->payload_offset > MI_CLS_LSO_MAX_PAYLOAD_OFFSET || o->payload_offset > h->len)
		return -1;
	if (odp_packet_payload_offset_set(pkt, o->payload_offset))
		return -1;
	h->lso_flags |= RT_LSO_REQ;
	h->lso_max_payload = o->max_payload_len;
	h->lso_prof = (uint8_t)i;
	return 0;
}

void odp_packet_lso_request_clr(odp_packet_t pkt)
{
	rt_pkt_hdr(pkt)->lso_flags &= (uint8_t)~RT_LSO_REQ;
}

int odp_packet_has_lso_request(odp_packet_t pkt)
{
	return (rt_pkt_hdr(pkt)->lso_flags & RT_LSO_REQ) != 0;
}

/* odp_packet.c:2452-2470 */
uint32_t odp_packet_payload_offset(odp_packet_t pkt)
{
	const pkt_hdr_t *h = rt_pkt_hdr(pkt);

	return (h->lso_flags & RT_LSO_PAYLOAD_OFF) ? h->payload_off : ODP_PACKET_OFFSET_INVALID;
}

int odp_packet_payload_offset_set(odp_packet_t pkt, uint32_t offset)
{
	pkt_hdr_t *h = rt_pkt_hdr(pkt);

	/* the offset is kept in 16 bits, as the reference's (odp_packet_internal.h:142),
	 * which truncates; here a value that does not fit, or that would read
	 * back as ODP_PACKET_OFFSET_INVALID, is refused and nothing changes */
	if (offset >= ODP_PACKET_OFFSET_INVALID)
		return -1;
	h->lso_flags |= RT_LSO_PAYLOAD_OFF;
	h->payload_off = (uint16_t)offset;
	return 0;
}

/* The live profiles as the kernel's table (slot i: profile i; an unused
 * slot stays zero, which no descriptor may name). */
static void lso_table(mi_cls_lso_profile_t tab[MI_CLS_LSO_PROFILES])
{
	memset(tab, 0, MI_CLS_LSO_PROFILES * sizeof(tab[0]));
	pthread_mutex_lock(&LSO.lock);
	for (uint32_t i = 0; i < MI_CLS_LSO_PROFILES; i++) {
		const odp_lso_profile_param_t *p = &LSO.prof[i].param;

		if (!LSO.prof[i].used)
			continue;
		tab[i].proto = (uint8_t)p->lso_proto;
		tab[i].num_custom = p->lso_proto == ODP_LSO_PROTO_CUSTOM ? p->custom.num_custom : 0;
		for (uint32_t f = 0; f < tab[i].num_custom; f++) {
			mi_cls_lso_field_t *d = &tab[i].field[f];

			d->mod_op = (uint8_t)p->custom.field[f].mod_op;
			d->offset = (uint8_t)p->custom.field[f].offset;
			d->size = p->custom.field[f].size;
			d->mask[0] = p->custom.field[f].write_bits.first_seg.mask[0];
			d->mask[1] = p->custom.field[f].write_bits.middle_seg.mask[0];
			d->mask[2] = p->custom.field[f].write_bits.last_seg.mask[0];
			d->value[0] = p->custom.field[f].write_bits.first_seg.value[0];
			d->value[1] = p->custom.field[f].write_bits.middle_seg.value[0];
			d->value[2] = p->custom.field[f].write_bits.last_seg.value[0];
		}
	}
	pthread_mutex_unlock(&LSO.lock);
}

/* One source packet of an odp_pktout_send_lso call. */
typedef struct lso_plan {
	uint32_t hdr, pay, left, l3;
	int nseg;               /* 1: goes out whole */
	uint8_t prof;
	uint8_t st;             /* the kernel's verdict (MI_CLS_LSO_ST_*), set by lso_launch */
	uint32_t first;         /* its first segment in the call's segment list */
} lso_plan_t;

/* Run the LSO kernel for the segmented packets of a call (one launch):
 * descriptors, segment table and status bytes in page-locked memory; the
 * frames in place when every source and segment lies in the page-locked
 * arena, else through a bounce buffer (sources copied in, segments copied
 * out), with tx_chksum's conditions.  The pktio's arrays are shared by its
 * senders, so everything that reads them happens under txl: each segmented
 * packet's verdict is copied into its plan entry (pl[i].st) before the lock
 * is released.  0, or a negative errno. */
static int lso_launch(rt_pktio_t *e, const odp_packet_t pkts[], lso_plan_t *pl, int end, uint32_t nsrc,
		      const odp_packet_t segs[], uint32_t nsegs)
{
	mi_cls_lso_profile_t tab[MI_CLS_LSO_PROFILES];
	int rc = -ENOMEM;

	lso_table(tab);
	gather_t *g = &e->lsog;

	pthread_mutex_lock(&e->txl);
	if (gather_begin(g, nsrc, sizeof(mi_cls_lso_desc_t) + MI_CLS_LSO_MAX_SEGMENTS * sizeof(mi_cls_lso_seg_t) +
			 sizeof(uint32_t) + sizeof(uint16_t) + 1u, 64))
		goto out;
	/* per source: descriptor, MI_CLS_LSO_MAX_SEGMENTS segment entries, offset, length, status */
	mi_cls_lso_desc_t *desc = (mi_cls_lso_desc_t *)(void *)g->arr;
	mi_cls_lso_seg_t *seg = (mi_cls_lso_seg_t *)(void *)(desc + g->cap);
	uint32_t *off = (uint32_t *)(void *)(seg + (size_t)g->cap * MI_CLS_LSO_MAX_SEGMENTS);
	uint16_t *len = (uint16_t *)(void *)(off + g->cap);
	uint8_t *st = (uint8_t *)(void *)(len + g->cap);
	uint32_t k = 0;

	for (int i = 0; i < end; i++) {
		if (pl[i].nseg < 2)
			continue;
		const pkt_hdr_t *h = rt_pkt_hdr(pkts[i]);

		len[k] = (uint16_t)h->len;
		desc[k] = (mi_cls_lso_desc_t){ .hdr_len = (uint16_t)pl[i].hdr, .seg_payload = (uint16_t)pl[i].pay,
					       .l3 = (uint16_t)pl[i].l3, .profile = pl[i].prof,
					       .nseg = (uint8_t)pl[i].nseg, .first_seg = pl[i].first };
		st[k] = 0;
		off[k] = gather_place(g, h->head + h->data_off, h->len, 0, pkt_pool_pinned(h));
		/* the segments come from the source's pool: its test serves them */
		for (uint32_t j = pl[i].first; j < pl[i].first + (uint32_t)pl[i].nseg; j++) {
			const pkt_hdr_t *sh = rt_pkt_hdr(segs[j]);

			seg[j].src = k;
			seg[j].off = gather_place(g, sh->head + sh->data_off, sh->len, 0, 1);
		}
		k++;
	}
	const int bounce = rc = gather_layout(g);

	if (bounce < 0)
		goto out;
	k = 0;
	for (int i = 0; bounce && i < end; i++) {
		if (pl[i].nseg < 2)
			continue;
		const pkt_hdr_t *h = rt_pkt_hdr(pkts[i]);

		off[k] = gather_step(g, h->len);
		memcpy(g->stage + off[k++], h->head + h->data_off, h->len);
		for (uint32_t j = pl[i].first; j < pl[i].first + (uint32_t)pl[i].nseg; j++)
			seg[j].off = gather_step(g, rt_pkt_hdr(segs[j])->len);
	}
	rc = odp_amd_cls_lso_segment_host(e->hdl, g->base, g->bytes, off, len, desc, nsrc, seg, nsegs, tab,
					  MI_CLS_LSO_PROFILES, st);
	if (rc)
		goto out;
	for (uint32_t j = 0; bounce && j < nsegs; j++) {
		pkt_hdr_t *sh = rt_pkt_hdr(segs[j]);

		if (st[seg[j].src] == MI_CLS_LSO_ST_OK)
			memcpy(sh->head + sh->data_off, g->stage + seg[j].off, sh->len);
	}
	k = 0;
	for (int i = 0; i < end; i++)
		if (pl[i].nseg >= 2)
			pl[i].st = st[k++];
	gather_ran(g);
out:
	pthread_mutex_unlock(&e->txl);
	return rc;
}

/* odp_pktout_send_lso (odp_packet_io.c:3253-3348) with one kernel launch for
 * the whole call: every packet is planned on the host (mi_cls_lso_plan,
 * _odp_lso_num_packets), the segments of the packets that need them are
 * allocated from each source's pool (:3172-3189), one launch cuts and edits
 * them all (_odp_lso_create_packets), and the list -- a packet's segments, or
 * the packet itself -- goes to odp_pktout_send in order.  The list ends at the
 * first packet without a request (opt == NULL), whose plan or allocation
 * fails, or whose header the kernel refuses.  Returns the source packets
 * completely sent; their originals are freed when they were segmented; a
 * packet of which only some segments were taken counts as failed: its unsent
 * segments are freed and its original stays with the caller (:3284-3297). */
int odp_pktout_send_lso(odp_pktout_queue_t q, const odp_packet_t pkts[], int num, const odp_packet_lso_opt_t *opt)
{
	rt_pktio_t *e = get_pk(q.pktio);

	if (!e || num <= 0)
		return -1;
	/* as odp_pktout_send: nothing is sent on a pktio that is not started --
	 * which is every pktio where there is no GPU (odp_pktio_start fails):
	 * no CPU segmentation stands in, said once */
	if (e->state != ST_STARTED) {
		if (!LSO.not_started_said)
			RT_ERR("pktio %s: odp_pktout_send_lso on a pktio that is not started\n", e->name);
		LSO.not_started_said = 1;
		return -1;
	}
	lso_plan_t *pl = calloc((size_t)num, sizeof(*pl));
	odp_packet_t *segs = NULL, *out = NULL;
	uint32_t nsegs = 0, nsrc = 0;
	int end = 0, sent = 0, ret = -1;

	if (!pl)
		return -1;
	/* ---- plan and allocate */
	for (end = 0; end < num; end++) {
		const pkt_hdr_t *h = rt_pkt_hdr(pkts[end]);
		lso_plan_t *p = &pl[end];
		uint32_t maxp;
		int slot;

		if (opt) {
			slot = lso_slot(opt->lso_profile);
			p->hdr = opt->payload_offset;
			maxp = opt->max_payload_len;
		} else {
			if (!(h->lso_flags & RT_LSO_REQ)) {
				RT_ERR("no LSO options on packet %d\n", end);
				if (end == 0)
					goto done;   /* -1 (:3330) */
				break;
			}
			slot = h->lso_prof;
			p->hdr = odp_packet_payload_offset(pkts[end]);
			maxp = h->lso_max_payload;
		}
		if (slot < 0 || !LSO.prof[slot].used || h->len > 65535u)
			break;
		const uint32_t proto = (uint32_t)LSO.prof[slot].param.lso_proto;

		p->prof = (uint8_t)slot;
		p->l3 = h->l3;
		p->nseg = mi_cls_lso_plan(h->len, p->hdr, maxp, proto, p->l3, &p->pay, &p->left);
		if (p->nseg <= 0)
			break;
		if (p->nseg == 1)
			continue;
		odp_packet_t *ns = realloc(segs, (nsegs + (uint32_t)p->nseg) * sizeof(*segs));

		if (!ns)
			break;
		segs = ns;
		/* the full ones, then the left-over one (:3172-3189) */
		const int full = p->left ? p->nseg - 1 : p->nseg;
		const odp_pool_t pool = odp_packet_pool(pkts[end]);
		int got = odp_packet_alloc_multi(pool, p->hdr + p->pay, &segs[nsegs], full);

		if (got == full && p->left) {
			segs[nsegs + (uint32_t)full] = odp_packet_alloc(pool, p->hdr + p->left);
			got += segs[nsegs + (uint32_t)full] != ODP_PACKET_INVALID;
		}
		if (got < p->nseg) {
			if (got > 0)
				odp_packet_free_multi(&segs[nsegs], got);
			break;
		}
		p->first = nsegs;
		if (proto == ODP_LSO_PROTO_IPV4)   /* lso_update_ipv4 sets it (:2994) */
			for (int s = 0; s < p->nseg; s++)
				odp_packet_l3_offset_set(segs[nsegs + (uint32_t)s], p->l3);
		nsegs += (uint32_t)p->nseg;
		nsrc++;
	}
	/* ---- one launch for every segmented packet of the call */
	if (nsrc) {
		const int rc = lso_launch(e, pkts, pl, end, nsrc, segs, nsegs);
		int cut = -1;   /* the first packet whose segments are dropped */

		if (rc)   /* no CPU segmentation stands in: the list ends at the first segmented packet */
			RT_ERR("pktio %s: LSO segmentation failed (%s)\n", e->name, mi_cls_strerror(rc));
		for (int i = 0; i < end && cut < 0; i++)
			if (pl[i].nseg >= 2 && (rc || pl[i].st != MI_CLS_LSO_ST_OK))
				cut = i;
		if (cut >= 0) {
			for (int i = cut; i < end; i++)
				if (pl[i].nseg >= 2)
					odp_packet_free_multi(&segs[pl[i].first], pl[i].nseg);
			end = cut;
		}
	}
	/* ---- the output list, in order */
	uint32_t nout = 0;

	for (int i = 0; i < end; i++)
		nout += (uint32_t)pl[i].nseg;
	ret = 0;
	if (nout == 0)
		goto done;
	out = malloc(nout * sizeof(*out));
	if (!out) {
		for (int i = 0; i < end; i++)
			if (pl[i].nseg >= 2)
				odp_packet_free_multi(&segs[pl[i].first], pl[i].nseg);
		goto done;
	}
	nout = 0;
	for (int i = 0; i < end; i++) {
		if (pl[i].nseg >= 2)
			memcpy(&out[nout], &segs[pl[i].first], (size_t)pl[i].nseg * sizeof(*out));
		else
			out[nout] = pkts[i];
		nout += (uint32_t)pl[i].nseg;
	}
	int r = odp_pktout_send(q, out, (int)nout);

	if (r < 0)
		r = 0;
	uint32_t pos = 0;

	for (int i = 0; i < end; i++) {
		const uint32_t n = (uint32_t)pl[i].nseg;

		if (pos + n <= (uint32_t)r && sent == i) {
			sent++;
			if (n >= 2)
				odp_packet_free(pkts[i]);   /* the original (:3300) */
		} else if (n >= 2) {
			/* not, or only partly, taken: its unsent segments are freed */
			const uint32_t took = (uint32_t)r > pos ? (uint32_t)r - pos : 0;

			odp_packet_free_multi(&out[pos + took], (int)(n - took));
		}
		pos += n;
	}
	ret = sent;
done:
	free(out);
	free(segs);
	free(pl);
	return ret;
}

int odp_amd_pktio_lso_stats(odp_pktio_t h, uint64_t *bursts, uint64_t *bounced)
{
	rt_pktio_t *e = get_pk(h);

	if (!e || !bursts || !bounced)
		return -1;
	pthread_mutex_lock(&e->txl);
	*bursts = e->lsog.bursts;
	*bounced = e->lsog.bounced;
	pthread_mutex_unlock(&e->txl);
	return 0;
}
