/*
 * odp_rt_internal.h -- private structures shared by the runtime sources
 * (odp_rt.c: init/shm/pools/packets/events/queues/scheduler,
 *  odp_pktio.c / odp_pktin.c / odp_pktout.c: packet I/O control plane,
 *  the GPU receive path and the transmit side, odp_pktio_internal.h).
 */
#ifndef ODP_AMD_RT_INTERNAL_H_
#define ODP_AMD_RT_INTERNAL_H_

#include <pthread.h>

#include "odp_api.h"
#include "mi_cls.h"

#define RT_MAX_POOLS   64
#define RT_MAX_QUEUES  1024
#define RT_MAX_PKTIO   64
#define RT_LOOP_MAX_QUEUE_SIZE 1024   /* LOOP_MAX_QUEUE_SIZE, pktio/loop.c:46 */
#define RT_MAX_AGGR    4
/* CONFIG_PACKET_HEADROOM (platform/linux-generic/include/odp_config_internal.h:105) */
/* odp_pktin_config_opt_t bits the receive path implements: ipv4/udp/tcp/
 * sctp checksum validation and the five drop-on-error options */
#define RT_PKTIN_OPT_MASK 0x7FCull
/* odp_pktout_config_opt_t bits a loop pktio implements: the four checksum
 * insertion defaults (bits 5-8) and their per-packet override enables (1-4);
 * bit 0 is ts_ena, which it does not.  The option word of
 * mi_cls_chksum_insert (include/mi_cls.h) is these bits without bit 0. */
#define RT_PKTOUT_OPT_MASK 0x1FEull
#define RT_PKTOUT_TX_WORD(all_bits) (((all_bits) & RT_PKTOUT_OPT_MASK) >> 1)
#define RT_PKTOUT_TX_CK 0xF0ull   /* ipv4 / udp / tcp / sctp _chksum of that word */
#define RT_PKT_HEADROOM 128
#define RT_PKT_TAILROOM 64

#define RT_LSO_REQ 1u
#define RT_LSO_PAYLOAD_OFF 2u

#define RT_ERR(...) fprintf(stderr, "odp: " __VA_ARGS__)

/* common event header: packets and event vectors start with it */
typedef struct ev_hdr {
	uint8_t type;           /* odp_event_type_t */
	uint8_t subtype;
	uint16_t pool;          /* pool index */
	uint32_t index;         /* element index in the pool */
	struct ev_hdr *next;
} ev_hdr_t;

/* packet metadata: the fields odp_packet_hdr_t carries on the receive path
 * (platform/linux-generic/include/odp_packet_internal.h:55-70,112-139).
 * From data_off on they are mi_cls_pkt_meta_t, the block the GPU receive
 * delivery writes (mi_cls_deliver_submit). */
typedef struct pkt_hdr {
	ev_hdr_t ev;
	uint8_t *head;          /* buffer start */
	uint32_t buf_len;       /* headroom + data capacity + tailroom */
	uint32_t rsv;
	/* the metadata block fills the header's second cache line: the GPU
	 * writes it whole, and the line the pool and queues use stays the
	 * host's */
	uint8_t pad[32];
	union {
		mi_cls_pkt_meta_t meta;
		struct {
			uint32_t data_off;      /* current headroom */
			uint32_t len;
			uint64_t in_flags;      /* packet_parser_t.input_flags */
			uint8_t err;            /* flags.all.error (7 bits) */
			uint8_t cos;            /* CoS index, 0xff none */
			uint16_t cls_mark;
			uint16_t l2, l3, l4;
			/* pktout checksum overrides (MI_CLS_TXF_*: l3/l4_chksum_set,
			 * l3/l4_chksum of packet_parser_t.flags); the GPU receive
			 * delivery writes the block whole, this field as 0 */
			uint16_t tx_ck;
			/* LSO request state (odp_packet_lso_request; reference
			 * p.flags.lso / payload_off, payload_offset, lso_profile_idx,
			 * lso_max_payload) in the block's reserved words: the GPU
			 * deliveries write them as 0, so a received packet carries
			 * none; odp_packet_alloc clears them */
			uint16_t payload_off;
			uint8_t lso_flags;      /* RT_LSO_REQ | RT_LSO_PAYLOAD_OFF */
			uint8_t lso_prof;
			odp_queue_t dst_queue;
			odp_pktio_t input;
			const void *user_ptr;
			uint32_t lso_max_payload;
			uint32_t rsv2;
		};
	};
} pkt_hdr_t;

_Static_assert(sizeof(((pkt_hdr_t *)0)->meta) == 64 && __builtin_offsetof(pkt_hdr_t, meta) == 64 &&
	       __builtin_offsetof(pkt_hdr_t, user_ptr) - __builtin_offsetof(pkt_hdr_t, meta) ==
	       __builtin_offsetof(mi_cls_pkt_meta_t, user_ptr) &&
	       __builtin_offsetof(pkt_hdr_t, dst_queue) - __builtin_offsetof(pkt_hdr_t, meta) ==
	       __builtin_offsetof(mi_cls_pkt_meta_t, dst_queue) &&
	       __builtin_offsetof(pkt_hdr_t, l4) - __builtin_offsetof(pkt_hdr_t, meta) ==
	       __builtin_offsetof(mi_cls_pkt_meta_t, l4) &&
	       __builtin_offsetof(pkt_hdr_t, in_flags) - __builtin_offsetof(pkt_hdr_t, meta) ==
	       __builtin_offsetof(mi_cls_pkt_meta_t, in_flags),
	       "pkt_hdr_t fields must overlay mi_cls_pkt_meta_t");

typedef struct evv_hdr {
	ev_hdr_t ev;
	uint32_t size;
	uint32_t max_size;
	odp_event_t tbl[];
} evv_hdr_t;

typedef struct rt_pool {
	int used;
	char name[ODP_POOL_NAME_LEN];
	odp_pool_param_t param;
	uint8_t *mem;
	size_t elem_size;
	uint32_t num;
	uint32_t data_cap;      /* packet data capacity (excl. head/tailroom) */
	ev_hdr_t **free_stk;    /* free events: a stack of pointers (bulk take / give
				 * copy pointers; no walk through the events) */
	uint32_t num_free;      /* on free_stk (thread caches not counted) */
	uint32_t gen;           /* creation number: tags the thread caches */
	int pinned;             /* mem is page-locked and device-addressed at its host
				 * addresses (GPU receive delivery reads / writes it) */
	int vpinned;            /* the same for a packet-vector pool (the vector fill
				 * writes its vectors); kept apart from `pinned`, which
				 * speaks of packets alone */
	odp_spinlock_t lock;
} rt_pool_t;

typedef struct rt_queue rt_queue_t;

struct rt_queue {
	int used;
	char name[ODP_QUEUE_NAME_LEN];
	odp_queue_param_t param;
	odp_spinlock_t lock;
	odp_event_t *ring;
	uint32_t cap, head, count;
	void *context;
	int owner;              /* atomic/ordered context holder: thread id + 1 */
	int sched_slot;         /* index in the scheduler list, -1 none */
	/* event aggregation (queue_types.h num_aggr / odp_queue_aggr) */
	uint32_t num_aggr;
	rt_queue_t *aggr[RT_MAX_AGGR];
	int is_aggr;
	rt_queue_t *base;
	odp_event_aggr_config_t aggr_cfg;
	evv_hdr_t *cur_vec;
	uint64_t cur_t0;
	/* plain pktin queue (ODP_PKTIN_MODE_QUEUE): pktio to poll when empty */
	int pktin_idx;          /* pktio index + 1, 0 none */
	/* a loop pktio's loop queue of a configured size: events it holds at
	 * most (0: no bound, every other queue) */
	uint32_t limit;
};

/* runtime-private entry points */
pkt_hdr_t *rt_pkt_hdr(odp_packet_t pkt);
rt_pool_t *rt_pool(odp_pool_t pool);
/* free events of a pool this thread can allocate: its free list plus the
 * calling thread's cache */
uint32_t rt_pool_avail(odp_pool_t pool);
/* up to num packets of a pool whose buffers hold len bytes, headers NOT
 * initialised (rt_packet_init does that, e.g. after a prefetch); returns the
 * count taken */
int rt_packet_alloc_raw(odp_pool_t pool, uint32_t len, odp_packet_t pkt[], int num);
void rt_packet_init(odp_packet_t pkt, uint32_t len);
/* packets taken with rt_packet_alloc_raw and not used, back to their pool */
void rt_packet_return_raw(odp_pool_t pool, const odp_packet_t pkt[], int num);
int rt_queue_enq_multi(rt_queue_t *q, const odp_event_t ev[], int num);
int rt_queue_deq_multi_raw(rt_queue_t *q, odp_event_t ev[], int num);
int rt_thread_id(void);
/* scheduler hooks for SCHED-mode packet input (odp_pktin.c) */
int rt_pktio_sched_poll(void);
int rt_pktio_poll_index(int idx);
uint32_t rt_gpu_index(void);
int rt_queue_is_valid(odp_queue_t h);
/* the address range spanned by the pinned packet pools ([*lo, *lo + *bytes));
 * 0 when there is none */
int rt_pinned_arena(uint8_t **lo, size_t *bytes);
/* 1 when every handle of pk[0..n) is a header in a page-locked pool (the
 * GPU may read it): the handles' addresses against the pools' ranges */
int rt_pinned_handles(const odp_packet_t pk[], int n);
/* bytes from a packet header's metadata block to its data at the default
 * headroom (fixed by the pool layout) */
uint32_t rt_data_from_meta(void);
/* the address range spanned by the page-locked packet-vector pools; 0 when
 * there is none */
int rt_vec_arena(uint8_t **lo, size_t *bytes);
/* up to num vectors of an ODP_POOL_VECTOR pool with one call, sizes not set;
 * returns the count taken.  rt_packet_return_raw gives unused ones back. */
int rt_vector_alloc_raw(odp_pool_t pool, odp_event_t v[], int num);

#endif /* ODP_AMD_RT_INTERNAL_H_ */
