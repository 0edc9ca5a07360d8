/*
 * odp_pktio_internal.h -- what the packet I/O units share:
 *   odp_pktio.c    control plane and statistics (owns the pktio table)
 *   odp_pktin.c    the receive path
 *   odp_pktout.c   the transmit side and odp_packet_parse
 * over odp_pcap.h, the capture file reader (plain C, no ODP types).
 *
 * Everything declared here is internal to the library (hidden visibility).
 */
#ifndef ODP_AMD_PKTIO_INTERNAL_H_
#define ODP_AMD_PKTIO_INTERNAL_H_

#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "odp_rt_internal.h"
#include "odp_pcap.h"
#include "mi_cls.h"

#pragma GCC visibility push(hidden)

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
/* devices one receive chain spans (a multi-GPU pktio: one slice each) */
#define RX_SLICES 8

/* Per-chunk pktio counters of a delivery. */
typedef struct {
	uint64_t in_errors, in_discards, octets, packets;
} rx_cnt_t;

/* The host batch of one offload caller (pktout checksum insertion, LSO,
 * odp_packet_parse_multi), kept across its calls: the functions are
 * gather_*, odp_pktout.c. */
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

/* One receive burst on its way through the GPU (odp_pktin.c). */
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
	/* ---- control (odp_pktio.c writes; every unit reads) */
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
	uint32_t rx_idx;            /* input queue of the receive call in progress (rxl; odp_pktin.c) */
	/* per-queue counters (loop.c:781-805): pktio_stats stays their sum;
	 * the receive and transmit paths add, the control unit reads and resets */
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
	/* ---- capture store (pcap driver): loaded at open and freed at close by
	 * odp_pktio.c; the read position is odp_pktin.c's (under rxl), the dump
	 * file odp_pktout.c's */
	pcap_store_t fs;        /* the input file's frames; fs.bytes is the classify entry's limit */
	int fs_pinned;          /* fs.buf is a page-locked copy: the GPU reads frames in place */
	uint32_t next;          /* frame the next burst starts at */
	int loops, loop_cnt, eof;
	FILE *tx;
	/* loop: one loop queue per input queue (made by odp_pktio.c) */
	odp_queue_t loopq[ODP_PKTIN_MAX_QUEUES];
	/* ---- receive sets (odp_pktin.c, under rxl) */
	/* GPU bursts: RX_SETS staging sets, so one burst is staged while older
	 * ones are classified and delivered (pipelined receive, pktio_recv) */
	rx_set_t rs[RX_SETS];
	int cur;                /* set the next burst is staged into */
	/* ---- chain table (odp_pktin.c, under rxl) */
	/* receive chain: the control plane's table (per generation), the pools
	 * of its slots and how many packets of each a burst is given */
	mi_cls_rxtab_t *rxtab;
	int rxtab_pinned, rxtab_ok;
	uint64_t rxtab_gen;
	odp_pool_t rx_pools[MI_CLS_RX_POOLS];
	uint32_t rx_np, rx_want[MI_CLS_RX_POOLS];
	/* ---- transmit (odp_pktout.c) */
	/* the gathers of pktout checksum insertion (a send burst) and of LSO (an
	 * odp_pktout_send_lso call), both under txl */
	pthread_mutex_t txl;    /* held across the kernel's launch and wait */
	gather_t txg, lsog;
	uint64_t txq_bursts;    /* sends whose launch computed the flow hash */
	/* ---- receive profile (odp_pktin.c adds, odp_pktio.c prints at close) */
	uint64_t prof[16];      /* ODP_AMD_RX_PROF: ns staging / classifying / delivering, bursts,
				 * then of delivering: ns preparing / enqueueing, TSC ticks in
				 * packet allocation / frame copies; GPU delivery: ns deciding +
				 * taking packets + entries, ns in the delivery kernel (submit to
				 * wait), ns enqueueing, bursts; receive chain: ns in its
				 * submit call (odp_amd_cls_rx_chain) */
} rt_pktio_t;

/* odp_pktio.c: the pktio table, its lock, and the started SCHED-mode pktios
 * that odp_schedule*() polls (rt_pktio_sched_poll, odp_pktin.c) */
extern rt_pktio_t PK[RT_MAX_PKTIO];
extern odp_spinlock_t pk_lock;
extern int sched_list[RT_MAX_PKTIO];
extern int num_sched_pktio;

/* odp_pktin.c */
extern int rx_prof;   /* ODP_AMD_RX_PROF set: receive-path phase times (-1: not read yet) */
uint32_t rx_burst(void);
int stage_reserve(rx_set_t *s, uint32_t n, size_t bytes);
void rx_sets_free(rt_pktio_t *e);
void rx_drain(rt_pktio_t *e);

/* odp_pktout.c */
void tx_free(rt_pktio_t *e);

#pragma GCC visibility pop

static inline rt_pktio_t *get_pk(odp_pktio_t h)
{
	uintptr_t i = (uintptr_t)h;

	if (i == 0 || i > RT_MAX_PKTIO || !PK[i - 1].used)
		return NULL;
	return &PK[i - 1];
}

/* An on/off environment switch (on unless its value starts with '0'), read
 * once into *cached (-1 before). */
static inline int env_switch(const char *name, int *cached)
{
	if (*cached < 0) {
		const char *v = getenv(name);

		*cached = !(v && v[0] == '0');
	}
	return *cached;
}

static inline uint64_t prof_ns(void)
{
	struct timespec ts;

	if (rx_prof <= 0)
		return 0;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

/* Host memory the GPU can read in place (page-locked) where there is a GPU,
 * ordinary memory otherwise (parse layer NONE needs none). */
static inline void *hmem_alloc(size_t bytes, int *pinned)
{
	void *p = mi_cls_host_alloc(bytes);

	*pinned = p != NULL;
	return p ? p : malloc(bytes);
}

static inline void hmem_free(void *p, int pinned)
{
	if (pinned)
		mi_cls_host_free(p);
	else
		free(p);
}

#endif
