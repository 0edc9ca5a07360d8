/*
 * odp_pktio.c -- packet I/O for the MI355X build: the "loop" and "pcap"
 * drivers and the GPU receive path they share.
 *
 * Reference behaviour:
 *   platform/linux-generic/odp_packet_io.c  (open/config/start/stop/close,
 *                                            pktin/pktout queue config)
 *   platform/linux-generic/pktio/loop.c:253-384   loopback_recv
 *   platform/linux-generic/pktio/pcap.c:90-401    devname parsing, promisc
 *                                                 filter, pcapif_recv_pkt
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
 * The pcap reader (classic pcap and pcapng, both byte orders) replaces
 * libpcap, which this image does not have.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <x86intrin.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <time.h>

#include "odp_rt_internal.h"
#include "odp_txq.h"
#include "mi_cls.h"

static int rx_prof = -1;   /* ODP_AMD_RX_PROF set: receive-path phase times */

static uint64_t prof_ns(void)
{
	struct timespec ts;

	if (rx_prof <= 0)
		return 0;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

enum { DRV_LOOP = 1, DRV_PCAP, DRV_NULL };
enum { ST_OPENED = 0, ST_STARTED, ST_STOPPED };

#define RX_BURST_DEFAULT 4096
/* receive pipeline depth (pktio_recv): classifications and GPU deliveries
 * in flight */
#define RX_CLS_DEPTH 1
#define RX_DLV_DEPTH 3
/* staging sets per pktio: the burst being staged, those whose classification
 * is in flight and those whose GPU delivery is */
#define RX_SETS (1 + RX_CLS_DEPTH + RX_DLV_DEPTH)
/* in-place loop bursts: offsets from the pinned arena's base stay below the
 * kernel's out-of-range offset */
#define OOB_SPAN ((size_t)0xF0000000u)
#define PCAP_MTU_MAX (64 * 1024)
/* devices one receive chain spans (a multi-GPU pktio: one slice each) */
#define RX_SLICES 8

/* Per-chunk pktio counters of a delivery. */
typedef struct {
	uint64_t in_errors, in_discards, octets, packets;
} rx_cnt_t;

/* The host batch of one offload caller (pktout checksum insertion, LSO,
 * odp_packet_parse_multi), kept across its calls: the functions are
 * gather_*, below. */
typedef struct {
	uint8_t *arr;           /* one allocation the caller carves its per-entry arrays from */
	uint32_t cap;           /* entries */
	int pinned;
	uint8_t *stage;         /* bounce buffer */
	size_t stage_cap;
	int stage_pinned;
	uint64_t bursts, bounced;   /* calls that ran the kernel / of them through the bounce buffer */
	/* the call in hand */
	int in_place;
	uint8_t *lo;            /* the page-locked arena */
	size_t span;
	uint8_t *base;          /* what the GPU entry is given: the arena or the bounce buffer, */
	size_t bytes, pos;      /* its size; the next bounce offset */
} gather_t;

/* One receive burst on its way through the GPU. */
typedef struct {
	uint8_t *stage;         /* copies of the frames (64 B aligned offsets) */
	size_t stage_cap;
	int stage_pinned;
	const uint8_t *base;    /* the burst's frames: base + soff[i], slen[i] bytes */
	size_t bytes;
	uint32_t *soff;
	uint16_t *slen;
	mi_cls_result_t *res;
	odp_packet_t *pk;       /* loop driver: the packets themselves */
	odp_packet_t *tmp;      /* delivery: packets grouped by queue */
	uint32_t tmp_cap;
	uint32_t n_cap;
	int arr_pinned;
	/* GPU delivery (mi_cls_deliver_submit): entries, permutation and
	 * group counts in page-locked memory; the packet of each entry */
	mi_cls_dlv_t *dlv;
	uint32_t *perm;
	uint32_t *gcnt;
	odp_packet_t *ent;      /* delivered packet per entry */
	odp_packet_t *old;      /* loop packets whose frames the GPU copies out (pool switch) */
	uint8_t *ppool;         /* loop: each packet's pool index + 1 (read at staging) */
	uint16_t *pdoff;        /* loop: each packet's headroom */
	const void **pup;       /* loop: each packet's user pointer */
	int dlv_pinned;
	/* a GPU delivery in flight (rx_dlv_start .. rx_dlv_end) */
	int delivering;
	uint64_t dticket;
	int derr;               /* the submit failed */
	uint32_t ne;            /* entries */
	int nold, grouped, ng;
	odp_queue_t gq[MI_CLS_DLV_GROUPS];
	rx_cnt_t cnt;
	int n;
	int pending;            /* staged (and submitted), not delivered */
	uint64_t ticket;        /* odp_amd_cls_classify_host_submit, 0 = done */
	uint64_t gen;           /* control-plane generation the set was submitted under */
	uint64_t dgen;          /* generation its delivery was decided under (rx_dlv_start) */
	/* receive chain (rxc_submit .. rxc_end): the burst classified, decided
	 * and delivered by the GPU from one submission, `delivering` from it */
	int chain;
	int gstage;             /* loop burst staged by the GPU (only pk[] is set) */
	int pk_pinned;          /* pk / ppool page-locked */
	int rxc_pinned;         /* dec / cent / got / rxo page-locked */
	uint32_t *dec;          /* per frame: decision word (MI_CLS_RXF_*, mi_cls.h) */
	uint64_t *cent;         /* per frame: its packet, 0 none */
	uint64_t *got;          /* packets taken for the burst, per pool slot */
	uint32_t got_cap;
	mi_cls_rx_out_t *rxo;   /* per slice */
	/* a pktio over several devices (ODP_AMD_GPUS) runs one chain per device,
	 * each over a contiguous slice of the burst with packets of its own */
	int nsl;                /* slices */
	uint32_t sl_lo[RX_SLICES + 1];   /* slice j: frames [sl_lo[j], sl_lo[j + 1]) */
	uint64_t sl_tk[RX_SLICES];       /* its ticket on device j */
	uint32_t cnp;
	uint32_t cbase[RX_SLICES][MI_CLS_RX_POOLS], chave[RX_SLICES][MI_CLS_RX_POOLS];
	odp_pool_t cpool[MI_CLS_RX_POOLS];
} rx_set_t;

typedef struct {
	int used;
	char name[ODP_PKTIO_NAME_LEN];
	int drv;
	odp_pktio_t hdl;
	odp_pool_t pool;
	odp_pktio_param_t param;
	odp_pktio_config_t config;
	odp_pktin_queue_param_t inq_param;
	odp_queue_t inq[ODP_PKTIN_MAX_QUEUES];   /* SCHED / QUEUE mode input queues */
	int inq_configured;
	uint32_t num_in;            /* input queues (0 until configured: one) */
	uint32_t hash_proto;        /* pktin hash: hash_enable ? hash_proto.all_bits : 0 */
	uint32_t rx_idx;            /* input queue of the receive call in progress (rxl) */
	/* per-queue counters (loop.c:781-805): pktio_stats stays their sum */
	struct {
		odp_atomic_u64_t octets, packets, discards, errors;
	} inq_st[ODP_PKTIN_MAX_QUEUES];
	struct {
		odp_atomic_u64_t octets, packets;
	} outq_st[ODP_PKTOUT_MAX_QUEUES];
	uint32_t num_out;
	int state;
	int cls_enabled;
	odp_proto_layer_t parse_layer;
	int promisc;
	odp_spinlock_t rxl;
	odp_atomic_u64_t in_octets, in_packets, in_discards, in_errors;
	odp_atomic_u64_t out_octets, out_packets, out_discards;
	/* pcap */
	uint8_t *fbuf;
	uint32_t *foff;
	uint16_t *flen;
	uint32_t nframes, next;
	int loops, loop_cnt, eof;
	FILE *tx;
	/* loop: one loop queue per input queue */
	odp_queue_t loopq[ODP_PKTIN_MAX_QUEUES];
	size_t fbuf_bytes;      /* frame store size incl. 64 B of zero padding */
	int fbuf_pinned;        /* page-locked: the GPU reads frames in place */
	/* GPU bursts: RX_SETS staging sets, so one burst is staged while older
	 * ones are classified and delivered (pipelined receive, pktio_recv) */
	rx_set_t rs[RX_SETS];
	int cur;                /* set the next burst is staged into */
	/* receive chain: the control plane's table (per generation), the pools
	 * of its slots and how many packets of each a burst is given */
	mi_cls_rxtab_t *rxtab;
	int rxtab_pinned, rxtab_ok;
	uint64_t rxtab_gen;
	odp_pool_t rx_pools[MI_CLS_RX_POOLS];
	uint32_t rx_np, rx_want[MI_CLS_RX_POOLS];
	/* transmit: the gathers of pktout checksum insertion (a send burst) and
	 * of LSO (an odp_pktout_send_lso call), both under txl */
	pthread_mutex_t txl;    /* held across the kernel's launch and wait */
	gather_t txg, lsog;
	uint64_t txq_bursts;    /* sends whose launch computed the flow hash */
	uint64_t prof[16];      /* ODP_AMD_RX_PROF: ns staging / classifying / delivering, bursts,
				 * then of delivering: ns preparing / enqueueing, TSC ticks in
				 * packet allocation / frame copies; GPU delivery: ns deciding +
				 * taking packets + entries, ns in the delivery kernel (submit to
				 * wait), ns enqueueing, bursts; receive chain: ns in its
				 * submit call (odp_amd_cls_rx_chain) */
} rt_pktio_t;

static void rx_sets_free(rt_pktio_t *e);
static void tx_free(rt_pktio_t *e);
static void fbuf_free(rt_pktio_t *e);
static int rx_finish(rt_pktio_t *e, rx_set_t *s, odp_packet_t out[], int max_out);
static int rx_dlv_end(rt_pktio_t *e, rx_set_t *s, odp_packet_t out[], int max_out);
static int stage_reserve(rx_set_t *s, uint32_t n, size_t bytes);
static int rxc_loop_stage_ok(rt_pktio_t *e, rx_set_t *s, uint32_t max);

static rt_pktio_t PK[RT_MAX_PKTIO];
static odp_spinlock_t pk_lock;
/* started SCHED-mode pktios, polled from odp_schedule*() */
static int sched_list[RT_MAX_PKTIO];
static int num_sched_pktio;

static const uint8_t pcap_mac[6] = { 0x02, 0x00, 0x00, 0x00, 0x00, 0x02 };
static const uint8_t loop_mac[6] = { 0x02, 0xe9, 0x34, 0x80, 0x73, 0x01 };

uint32_t rt_gpu_index(void)
{
	const char *e = getenv("ODP_AMD_GPU");

	return e ? (uint32_t)atoi(e) : 0u;
}

/* An on/off environment switch (on unless its value starts with '0'), read
 * once into *cached (-1 before). */
static int env_switch(const char *name, int *cached)
{
	if (*cached < 0) {
		const char *v = getenv(name);

		*cached = !(v && v[0] == '0');
	}
	return *cached;
}

static uint32_t rx_burst(void)
{
	static uint32_t b;

	if (!b) {
		const char *e = getenv("ODP_AMD_RX_BURST");

		b = e && atoi(e) > 0 ? (uint32_t)atoi(e) : RX_BURST_DEFAULT;
	}
	return b;
}

static rt_pktio_t *get_pk(odp_pktio_t h)
{
	uintptr_t i = (uintptr_t)h;

	if (i == 0 || i > RT_MAX_PKTIO || !PK[i - 1].used)
		return NULL;
	return &PK[i - 1];
}

/* ============================================================ pcap reader */
static uint32_t rd32s(const uint8_t *p, int swap)
{
	uint32_t v;

	memcpy(&v, p, 4);
	return swap ? __builtin_bswap32(v) : v;
}

static uint16_t rd16s(const uint8_t *p, int swap)
{
	uint16_t v;

	memcpy(&v, p, 2);
	return swap ? __builtin_bswap16(v) : v;
}

/* append one frame to the packed, 64 B aligned frame store */
static int frame_add(rt_pktio_t *e, const uint8_t *d, uint32_t caplen, size_t *cap_b,
		     uint32_t *cap_n, size_t *used_b)
{
	if (caplen > 65535 || caplen == 0)
		return 0;   /* longer than the u16 descriptor: not received */
	if (e->nframes == *cap_n) {
		uint32_t nn = *cap_n ? *cap_n * 2 : 1024;
		uint32_t *o = realloc(e->foff, nn * sizeof(uint32_t));
		uint16_t *l = o ? realloc(e->flen, nn * sizeof(uint16_t)) : NULL;

		if (!o || !l)
			return -1;
		e->foff = o;
		e->flen = l;
		*cap_n = nn;
	}
	size_t need = *used_b + ((caplen + 63u) & ~63u);

	if (need > *cap_b) {
		size_t nb = *cap_b ? *cap_b : (1u << 20);

		while (nb < need)
			nb *= 2;
		uint8_t *b = realloc(e->fbuf, nb);

		if (!b)
			return -1;
		memset(b + *cap_b, 0, nb - *cap_b);
		e->fbuf = b;
		*cap_b = nb;
	}
	memcpy(e->fbuf + *used_b, d, caplen);
	e->foff[e->nframes] = (uint32_t)*used_b;
	e->flen[e->nframes] = (uint16_t)caplen;
	e->nframes++;
	*used_b = need;
	return 0;
}

/* Classic pcap (0xa1b2c3d4 / 0xa1b23c4d, either byte order) and pcapng
 * (SHB / IDB / EPB / SPB / PB blocks).  Only DLT_EN10MB (1) is accepted,
 * as in _pcapif_init_rx (pcap.c:130-134).  Returns 0 / -1. */
static int pcap_load(rt_pktio_t *e, const char *fname)
{
	FILE *f = fopen(fname, "rb");
	uint8_t *buf = NULL;
	long sz;
	size_t cap_b = 0, used_b = 0;
	uint32_t cap_n = 0;
	int rc = -1;

	if (!f) {
		RT_ERR("failed to open pcap file %s (%s)\n", fname, strerror(errno));
		return -1;
	}
	if (fseek(f, 0, SEEK_END) || (sz = ftell(f)) < 0 || fseek(f, 0, SEEK_SET))
		goto out;
	buf = malloc((size_t)sz + 1);
	if (!buf || fread(buf, 1, (size_t)sz, f) != (size_t)sz)
		goto out;
	if (sz < 24)
		goto bad;
	uint32_t m = rd32s(buf, 0);

	if (m == 0xa1b2c3d4u || m == 0xa1b23c4du || m == 0xd4c3b2a1u || m == 0x4d3cb2a1u) {
		int sw = (m == 0xd4c3b2a1u || m == 0x4d3cb2a1u);

		if ((rd32s(buf + 20, sw) & 0x0fffffffu) != 1u) {
			RT_ERR("unsupported datalink type: %u\n", rd32s(buf + 20, sw));
			goto out;
		}
		for (long p = 24; p + 16 <= sz;) {
			uint32_t incl = rd32s(buf + p + 8, sw);

			if (p + 16 + (long)incl > sz)
				break;
			if (frame_add(e, buf + p + 16, incl, &cap_b, &cap_n, &used_b))
				goto out;
			p += 16 + incl;
		}
		rc = 0;
	} else if (m == 0x0a0d0d0au) {
		int sw = 0;
		uint32_t link[64], nif = 0, snap[64];

		for (long p = 0; p + 12 <= sz;) {
			uint32_t type = rd32s(buf + p, sw);

			if (type == 0x0a0d0d0au) {   /* section header: byte order */
				uint32_t bom;

				memcpy(&bom, buf + p + 8, 4);
				sw = bom == 0x4d3c2b1au;
				nif = 0;
			}
			uint32_t blen = rd32s(buf + p + 4, sw);

			if (blen < 12 || p + (long)blen > sz)
				break;
			const uint8_t *b = buf + p + 8;

			if (type == 1 && nif < 64) {             /* interface description */
				link[nif] = rd16s(b, sw);
				snap[nif] = rd32s(b + 4, sw);
				nif++;
			} else if (type == 6 && blen >= 32) {   /* enhanced packet */
				uint32_t ifc = rd32s(b, sw), cap = rd32s(b + 12, sw);

				if (ifc < nif && link[ifc] != 1)
					goto bad_link;
				if (20 + cap <= blen - 12 &&
				    frame_add(e, b + 20, cap, &cap_b, &cap_n, &used_b))
					goto out;
			} else if (type == 3 && blen >= 16) {   /* simple packet */
				uint32_t olen = rd32s(b, sw), cap = olen;

				if (nif && link[0] != 1)
					goto bad_link;
				if (nif && snap[0] && cap > snap[0])
					cap = snap[0];
				if (4 + cap <= blen - 12 &&
				    frame_add(e, b + 4, cap, &cap_b, &cap_n, &used_b))
					goto out;
			} else if (type == 2 && blen >= 32) {   /* obsolete packet block */
				uint32_t ifc = rd16s(b, sw), cap = rd32s(b + 12, sw);

				if (ifc < nif && link[ifc] != 1)
					goto bad_link;
				if (20 + cap <= blen - 12 &&
				    frame_add(e, b + 20, cap, &cap_b, &cap_n, &used_b))
					goto out;
			}
			p += blen;
		}
		rc = 0;
	} else {
		goto bad;
	}
	goto out;
bad_link:
	RT_ERR("unsupported datalink type in %s\n", fname);
	goto out;
bad:
	RT_ERR("%s: not a pcap / pcapng file\n", fname);
out:
	if (rc == 0 && e->fbuf) {
		/* page-locked frame store: the GPU reads the bursts' header windows
		 * in place (zero copy, mi_cls_classify_host) and no staging copy is
		 * made.  ODP_AMD_RX_INPLACE=0 keeps the staged copies (A/B runs). */
		int in_place = -1;   /* per load: not cached */
		uint8_t *pb = env_switch("ODP_AMD_RX_INPLACE", &in_place) ? mi_cls_host_alloc(used_b + 64) : NULL;

		e->fbuf_bytes = used_b + 64;
		if (pb) {
			memcpy(pb, e->fbuf, used_b);
			memset(pb + used_b, 0, 64);
			free(e->fbuf);
			e->fbuf = pb;
			e->fbuf_pinned = 1;
		}
	}
	free(buf);
	fclose(f);
	return rc;
}

static int pcap_dump_open(rt_pktio_t *e, const char *fname)
{
	const uint32_t hdr[6] = { 0xa1b2c3d4u, 0x00040002u, 0, 0, PCAP_MTU_MAX, 1 };

	e->tx = fopen(fname, "wb");
	if (!e->tx) {
		RT_ERR("failed to open dump file %s\n", fname);
		return -1;
	}
	fwrite(hdr, sizeof(hdr), 1, e->tx);
	fflush(e->tx);
	return 0;
}

static void pcap_dump(rt_pktio_t *e, odp_packet_t pkt)
{
	struct timeval tv;
	uint32_t h[4];
	pkt_hdr_t *p = rt_pkt_hdr(pkt);

	gettimeofday(&tv, NULL);
	h[0] = (uint32_t)tv.tv_sec;
	h[1] = (uint32_t)tv.tv_usec;
	h[2] = h[3] = p->len;
	fwrite(h, sizeof(h), 1, e->tx);
	fwrite(p->head + p->data_off, 1, p->len, e->tx);
	fflush(e->tx);
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
		rc = pcap_load(e, rx);
	if (!rc && txn)
		rc = pcap_dump_open(e, txn);
	if (!rc && !rx && !txn)
		rc = -1;
	free(rx);
	free(txn);
	e->promisc = 0;   /* pcapif_init sets promisc off (pcap.c:232) */
	return rc;
}

/* BPF "ether dst <pcap_mac> or broadcast or multicast" (pcap.c:176-186) */
static int pcap_filter_pass(const rt_pktio_t *e, const uint8_t *d, uint32_t len)
{
	if (e->promisc)
		return 1;
	if (len < 6)
		return 0;
	return memcmp(d, pcap_mac, 6) == 0 || (d[0] & 1u);
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
		fbuf_free(e);
		free(e->foff);
		free(e->flen);
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
	 * (bits 2-10), pktout checksum insertion on a loop pktio (bits 0-7); no
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
	/* bursts still on the GPU were received before the stop: deliver them,
	 * oldest first */
	for (int k = 1; k <= RX_SETS; k++) {
		rx_set_t *s = &e->rs[(e->cur + k) % RX_SETS];

		if (s->delivering)
			(void)rx_dlv_end(e, s, NULL, 0);
		if (s->pending)
			(void)rx_finish(e, s, NULL, 0);
	}
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
	fbuf_free(e);
	free(e->foff);
	free(e->flen);
	rx_sets_free(e);
	tx_free(e);
	odp_spinlock_lock(&pk_lock);
	memset(e, 0, sizeof(*e));
	odp_spinlock_unlock(&pk_lock);
	return odp_amd_cls_pktio_destroy(h);
}

/* ============================================================ receive */
/* Host memory the GPU can read in place (page-locked) where there is a GPU,
 * ordinary memory otherwise (parse layer NONE needs none). */
static void *hmem_alloc(size_t bytes, int *pinned)
{
	void *p = mi_cls_host_alloc(bytes);

	*pinned = p != NULL;
	return p ? p : malloc(bytes);
}

static void hmem_free(void *p, int pinned)
{
	if (pinned)
		mi_cls_host_free(p);
	else
		free(p);
}

static void fbuf_free(rt_pktio_t *e)
{
	hmem_free(e->fbuf, e->fbuf_pinned);
	e->fbuf = NULL;
	e->fbuf_pinned = 0;
}

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

static void rx_sets_free(rt_pktio_t *e)
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
static int stage_reserve(rx_set_t *s, uint32_t n, size_t bytes)
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
		const int in_place = e->fbuf_pinned && s->arr_pinned;

		if (in_place)
			s->base = e->fbuf;
		while (n < max) {
			if (e->next >= e->nframes) {
				if (e->nframes == 0 || e->eof)
					break;
				/* _pcapif_reopen (pcap.c:257-278): note loop_cnt starts at 1 */
				if (e->loops != 0 && ++e->loop_cnt >= e->loops) {
					e->eof = 1;
					break;
				}
				e->next = 0;
			}
			const uint32_t fo = e->foff[e->next];
			const uint8_t *d = e->fbuf + fo;
			uint16_t l = e->flen[e->next];

			e->next++;
			if (!pcap_filter_pass(e, d, l))
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
		s->bytes = in_place ? e->fbuf_bytes : off + 64;
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
		return e->nframes && !e->eof &&
		       (e->next < e->nframes || e->loops == 0 || e->loop_cnt + 1 < e->loops);
	if (e->drv == DRV_LOOP)
		return ((rt_queue_t *)(void *)e->loopq[idx])->count > 0;
	return 0;
}

/* ODP_AMD_RX_PIPELINE=0: classify each burst synchronously */
static int rx_pipeline(void)
{
	static int on = -1;

	return env_switch("ODP_AMD_RX_PIPELINE", &on);
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

/* ODP_AMD_RX_GPU_DELIVER=0: host delivery only */
static int gpu_deliver_on(void)
{
	static int on = -1;

	return env_switch("ODP_AMD_RX_GPU_DELIVER", &on);
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
 * (pktio/loop.c:253-384, pcap.c:299-352).  ODP_AMD_RX_CHAIN=0 turns it off. */
static int rx_chain_on(void)
{
	static int on = -1;

	return env_switch("ODP_AMD_RX_CHAIN", &on);
}

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

static void tx_free(rt_pktio_t *e)
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
	const uint64_t opt = e->config.pktout.all_bits & RT_PKTOUT_OPT_MASK;
	const uint32_t hp = dst ? e->hash_proto : 0;
	int want = (opt & 0xF0u) != 0;

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
		if (e->tx)
			pcap_dump(e, pkts[i]);
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
	       e->cls_enabled ? "enabled (GPU)" : "disabled", e->nframes, s.in_packets,
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
		idle = e->eof || e->nframes == 0 || (e->next >= e->nframes && e->loops == 1);
	} else if (idle && e->drv == DRV_LOOP) {
		for (uint32_t i = 0; i < ODP_PKTIN_MAX_QUEUES && e->loopq[i] != ODP_QUEUE_INVALID; i++)
			idle &= ((rt_queue_t *)(void *)e->loopq[i])->count == 0;
	}
	odp_spinlock_unlock(&e->rxl);
	return idle;
}
