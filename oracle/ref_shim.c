/*
 * ref_shim.c -- runs the reference's OWN parser, checksum and classifier code
 * (odp_parse.c, odp_packet.c, odp_chksum.c, odp_hash_crc_gen.c,
 * odp_classification.c, arch/default/odp_hash_crc32.c, compiled unchanged by
 * oracle/Makefile's ref-lib target) behind the C ABI of the CPU restatement
 * (orc_* in odp_cls_oracle.c), so that the restatement and the kernels can be
 * compared with the reference itself.
 *
 *   *** TEST INFRASTRUCTURE -- NOT PART OF THE PRODUCT ***
 *
 * This file is this project's text.  It is compiled against the reference's
 * headers and holds two things:
 *
 *   1. stand-ins for the symbols the six reference sources leave undefined
 *      (shared memory, queues, the pktio entry table, logging, the thread
 *      state, the event / pool plumbing that the parse and match paths never
 *      reach);
 *   2. ref_*: reset, the control-plane calls (each one calls the real
 *      odp_cls_* / odp_cos_* / odp_pktio_*_cos_set function), a batch
 *      classify that runs the receive order of pktio/loop.c over a fake
 *      odp_packet_hdr_t, and odp_packet_parse on the same fake packet.
 * The transmit side (ref_tx_*) is in ref_loop_shim.c; ref_shim.h is what the
 * two share.
 *
 * Everything is single-threaded.  The reference never returns from a CoS
 * cycle (match_pmr_cos), so ref_classify_batch refuses a table whose rule
 * graph has one.
 */
#include <odp_api.h>

#include <odp_init_internal.h>
#include <odp_packet_internal.h>
#include <odp_packet_io_internal.h>
#include <odp_parse_internal.h>
#include <odp_pool_internal.h>
#include <odp_classification_datamodel.h>
#include <odp_classification_internal.h>
#include <odp_string_internal.h>
#include <odp/api/plat/thread_inline_types.h>
#include <odp/api/plat/event_inline_types.h>
#include <odp/api/plat/pool_inline_types.h>

#include "ref_shim.h"

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* parse_model.py / oracle.py pass these as plain integers */
_Static_assert(ODP_PROTO_ETH == 1 && ODP_PROTO_IPV4 == 2 && ODP_PROTO_IPV6 == 3, "proto numbers");
_Static_assert(ODP_PROTO_LAYER_L2 == 1 && ODP_PROTO_LAYER_L3 == 2 && ODP_PROTO_LAYER_L4 == 3 &&
	       ODP_PROTO_LAYER_ALL == 4, "layer numbers");
_Static_assert(ODP_PMR_LEN == 0 && ODP_PMR_CUSTOM_L3 == 20 && ODP_PMR_INNER_HDR_OFF == 32,
	       "term numbers");
_Static_assert(ODP_COS_ACTION_ENQUEUE == 0 && ODP_COS_ACTION_DROP == 1, "action numbers");

/* ============================================================ stand-ins */
/* A call that the parse / match / table code can never make ends the run
 * (UNREACHED, ref_shim.h). */

/* --- shared memory: one zeroed heap block per reserve */
odp_shm_t odp_shm_reserve(const char *name, uint64_t size, uint64_t align, uint32_t flags)
{
	void *p = NULL;

	(void)name;
	(void)flags;
	if (align < sizeof(void *))
		align = sizeof(void *);
	if (posix_memalign(&p, align, size))
		return ODP_SHM_INVALID;
	memset(p, 0, size);
	return (odp_shm_t)p;
}

void *odp_shm_addr(odp_shm_t shm)
{
	return (void *)shm;
}

int odp_shm_free(odp_shm_t shm)
{
	free((void *)shm);
	return 0;
}

/* --- queues: handles 1, 2, 3, ... in creation order, never reused, so a
 * handle names one slot of one CoS's queue group for the whole run */
static uintptr_t n_queues;

odp_queue_t odp_queue_create(const char *name, const odp_queue_param_t *param)
{
	(void)name;
	(void)param;
	return (odp_queue_t)++n_queues;
}

int odp_queue_destroy(odp_queue_t queue)
{
	(void)queue;
	return 0;
}

void odp_queue_param_init(odp_queue_param_t *param)
{
	memset(param, 0, sizeof(*param));
	param->type = ODP_QUEUE_TYPE_PLAIN;
}

odp_queue_type_t odp_queue_type(odp_queue_t queue)
{
	(void)queue;
	return ODP_QUEUE_TYPE_PLAIN;
}

int odp_queue_info(odp_queue_t queue, odp_queue_info_t *info)
{
	(void)queue;
	(void)info;
	return -1;
}

uint64_t odp_queue_to_u64(odp_queue_t hdl)
{
	return (uintptr_t)hdl;
}

/* --- pktio: one entry, handle 1 */
static pktio_entry_t the_entry;
void *_odp_pktio_entry_ptr[CONFIG_PKTIO_ENTRIES];
#define THE_PKTIO ((odp_pktio_t)(uintptr_t)1)

uint64_t odp_pktio_to_u64(odp_pktio_t pktio)
{
	return (uintptr_t)pktio;
}

/* --- log sink, thread state, strings */
static int log_sink(odp_log_level_t level, const char *fmt, ...)
{
	(void)level;
	(void)fmt;
	return 0;
}

odp_log_func_t _odp_log_fn = log_sink;

static _odp_thread_state_t the_thread = { .log_fn = log_sink, .type = ODP_THREAD_CONTROL, .thr = 0 };
__thread _odp_thread_state_t *_odp_this_thread = &the_thread;

int _odp_snprint(char *str, size_t size, const char *format, ...)
{
	va_list ap;
	int n;

	va_start(ap, format);
	n = vsnprintf(str, size, format, ap);
	va_end(ap);
	if (n < 0)
		return 0;
	return (size_t)n >= size ? (int)size - 1 : n;
}

char *_odp_strcpy(char *restrict dst, const char *restrict src, size_t sz)
{
	if (sz) {
		strncpy(dst, src, sz - 1);
		dst[sz - 1] = 0;
	}
	return dst;
}

/* --- event / pool plumbing: the offset tables of the event and pool inline
 * accessors (the parse, checksum and match paths read packets through
 * odp_packet.c's own _odp_packet_inline table, never through these two, so
 * they only have to exist), and the allocator entry points, which nothing on
 * the tested paths reaches */
const _odp_event_inline_offset_t _odp_event_inline_offset;
const _odp_pool_inline_offset_t _odp_pool_inline;

odp_event_t _odp_event_alloc(pool_t *pool)
{
	(void)pool;
	UNREACHED();
}

int _odp_event_alloc_multi(pool_t *pool, _odp_event_hdr_t *event_hdr[], int num)
{
	(void)pool;
	(void)event_hdr;
	(void)num;
	UNREACHED();
}

void _odp_event_free(odp_event_t event)
{
	(void)event;
	UNREACHED();
}

void _odp_event_free_multi(_odp_event_hdr_t *event_hdr[], int num_free)
{
	(void)event_hdr;
	(void)num_free;
	UNREACHED();
}

void _odp_event_free_sp(_odp_event_hdr_t *event_hdr[], int num)
{
	(void)event_hdr;
	(void)num;
	UNREACHED();
}

int _odp_event_is_valid(odp_event_t event)
{
	(void)event;
	UNREACHED();
}

void odp_buffer_free(odp_buffer_t buf)
{
	(void)buf;
	UNREACHED();
}

int odp_pool_info(odp_pool_t pool, odp_pool_info_t *info)
{
	(void)pool;
	(void)info;
	return -1;
}

/* ================================================================ ref_* */
/* the Term struct of oracle/oracle.py (orc_term_t) */
typedef struct {
	int term;
	uint8_t value[16];
	uint8_t mask[16];
	uint32_t val_sz;
	uint32_t offset;
} ref_term_t;

/* the 16-byte record of include/mi_cls.h (mi_cls_result_t, orc_result_t) */
typedef struct {
	uint32_t in_flags;
	uint8_t  err;
	uint8_t  outcome;
	uint8_t  cos;
	uint8_t  hops;
	uint16_t queue;
	uint16_t mark;
	uint16_t l3_offset;
	uint16_t l4_offset;
} ref_result_t;

_Static_assert(sizeof(ref_result_t) == 16, "result record is 16 bytes");

enum { OUT_ENQ = 0, OUT_COS_DROP = 1, OUT_DISCARD = 2, OUT_PARSE_DROP = 3 };

static odp_pktin_config_opt_t pktin_opt;

/* Tables zeroed, no default / error CoS, options off.  The table sizes are
 * the reference's compile-time constants: 64 CoS, 256 PMRs, 8 PMRs per CoS. */
int ref_reset(void)
{
	if (_odp_cls_global && _odp_classification_term_global())
		return -1;
	_odp_cls_global = NULL;
	if (_odp_classification_init_global())
		return -1;
	memset(&the_entry, 0, sizeof(the_entry));
	the_entry.handle = THE_PKTIO;
	the_entry.pool = ODP_POOL_INVALID;
	_odp_pktio_entry_ptr[0] = &the_entry;
	if (_odp_pktio_classifier_init(&the_entry))
		return -1;
	pktin_opt.all_bits = 0;
	n_queues = 0;
	return 0;
}

void ref_limits(uint32_t *max_cos, uint32_t *max_pmr, uint32_t *max_per_cos)
{
	*max_cos = CLS_COS_MAX_ENTRY;
	*max_pmr = CLS_PMR_MAX_ENTRY;
	*max_per_cos = CLS_PMR_PER_COS_MAX;
}

/* Same arguments and return value (handle = slot + 1, 0 refused) as
 * orc_cos_create; hash_proto_in is odp_pktin_hash_proto_t.all_bits. */
int ref_cos_create(int action, uint32_t num_queue, int has_queue, uint32_t hash_proto_in,
		   int stats_enable)
{
	odp_cls_cos_param_t param;

	odp_cls_cos_param_init(&param);
	param.action = (odp_cos_action_t)action;
	param.num_queue = num_queue;
	if (has_queue)
		param.queue = odp_queue_create(NULL, NULL);
	param.hash_proto.all_bits = hash_proto_in;
	param.stats_enable = stats_enable != 0;
	return (int)(uintptr_t)odp_cls_cos_create(NULL, &param);
}

int ref_cos_destroy(int h)
{
	return odp_cos_destroy((odp_cos_t)(uintptr_t)h);
}

int ref_pmr_create(const ref_term_t *terms, int num_terms, uint32_t mark, int src, int dst)
{
	odp_pmr_param_t p[num_terms > 0 ? num_terms : 1];
	odp_pmr_create_opt_t opt;
	int i;

	for (i = 0; i < num_terms; i++) {
		odp_cls_pmr_param_init(&p[i]);
		p[i].term = (odp_cls_pmr_term_t)terms[i].term;
		p[i].match.value = terms[i].value;
		p[i].match.mask = terms[i].mask;
		p[i].val_sz = terms[i].val_sz;
		p[i].offset = terms[i].offset;
	}
	odp_cls_pmr_create_opt_init(&opt);
	opt.terms = p;
	opt.num_terms = num_terms;
	opt.mark = mark;
	return (int)(uintptr_t)odp_cls_pmr_create_opt(&opt, (odp_cos_t)(uintptr_t)src,
						      (odp_cos_t)(uintptr_t)dst);
}

int ref_pmr_destroy(int h)
{
	return odp_cls_pmr_destroy((odp_pmr_t)(uintptr_t)h);
}

int ref_default_cos_set(int h)
{
	return odp_pktio_default_cos_set(THE_PKTIO, (odp_cos_t)(uintptr_t)h);
}

int ref_error_cos_set(int h)
{
	return odp_pktio_error_cos_set(THE_PKTIO, (odp_cos_t)(uintptr_t)h);
}

void ref_pktin_opt_set(uint64_t opt)
{
	pktin_opt.all_bits = opt;
}

/* odp_cls_cos_stats refuses a destroyed CoS; the counter itself stays in the
 * table, where orc_cos_stats_packets reads it too */
uint64_t ref_cos_stats_packets(int h)
{
	odp_cls_cos_stats_t st;

	if (h < 1 || h > CLS_COS_MAX_ENTRY)
		return 0;
	if (odp_cls_cos_stats((odp_cos_t)(uintptr_t)h, &st) == 0)
		return st.packets;
	return odp_atomic_load_u64(&_odp_cls_global->cos_tbl.cos_entry[h - 1].stats.packets);
}

/* 1 when some CoS can reach itself over the rule lists as they stand (links
 * to destroyed CoS included: they come back to life when the slot is reused) */
static int has_cycle(void)
{
	cos_t *tbl = _odp_cls_global->cos_tbl.cos_entry;
	uint8_t state[CLS_COS_MAX_ENTRY] = { 0 };   /* 0 new, 1 on the path, 2 done */
	int stack[CLS_COS_MAX_ENTRY], next[CLS_COS_MAX_ENTRY];
	int root, sp;

	for (root = 0; root < CLS_COS_MAX_ENTRY; root++) {
		if (state[root])
			continue;
		sp = 0;
		stack[0] = root;
		next[0] = 0;
		state[root] = 1;
		while (sp >= 0) {
			cos_t *c = &tbl[stack[sp]];
			uint32_t n = odp_atomic_load_u32(&c->num_rule);

			if ((uint32_t)next[sp] == n) {
				state[stack[sp--]] = 2;
				continue;
			}
			int to = (int)(c->linked_cos[next[sp]++] - tbl);

			if (state[to] == 1)
				return 1;
			if (state[to] == 0) {
				state[to] = 1;
				stack[++sp] = to;
				next[sp] = 0;
			}
		}
	}
	return 0;
}

/* A packet header over a private copy of the frame followed by TAIL_ZEROS
 * zero bytes: one segment, no pool behind it. */
odp_packet_hdr_t *ref_fake_packet(const uint8_t *frame, uint32_t len, uint8_t **data)
{
	static odp_packet_hdr_t hdr;

	*data = calloc(1, (size_t)len + TAIL_ZEROS);
	if (!*data)
		return NULL;
	memcpy(*data, frame, len);
	memset(&hdr, 0, sizeof(hdr));
	hdr.event_hdr.pool = ODP_POOL_INVALID;
	hdr.event_hdr.base_data = *data;
	hdr.event_hdr.buf_end = *data + len + TAIL_ZEROS;
	hdr.event_hdr.event_type = ODP_EVENT_PACKET;
	hdr.event_hdr.subtype = ODP_EVENT_PACKET_BASIC;
	hdr.seg_data = *data;
	hdr.seg_len = len;
	hdr.frame_len = len;
	hdr.seg_count = 1;
	hdr.tailroom = TAIL_ZEROS;
	hdr.input = ODP_PKTIO_INVALID;
	hdr.dst_queue = ODP_QUEUE_INVALID;
	return &hdr;
}

/* the slot of a hash queue in its CoS's group (queue_grp_tbl, 32 per CoS) */
static uint16_t queue_slot(uint32_t cos_index, odp_queue_t q)
{
	const odp_queue_t *grp = &_odp_cls_global->queue_grp_tbl.queue[cos_index * CLS_COS_QUEUE_MAX];
	uint16_t j;

	for (j = 0; j < CLS_COS_QUEUE_MAX; j++)
		if (grp[j] == q)
			return j;
	return 0xFFFF;
}

/* The receive order of pktio/loop.c for one frame (parse reset, parse with
 * the pktin options at layer ALL, classify) into the record the oracle's
 * classify_one() writes:
 *   parse -1            PARSE_DROP, cos 0xFF, queue 0, mark 0
 *   classify -1         DISCARD (no CoS), cos 0xFF, queue 0
 *   classify 1          COS_DROP, queue 0; the reference does not say which
 *                       CoS dropped (it returns before pkt_hdr->cos is set):
 *                       cos is written 0xFF and the comparison masks it
 *   classify 0          ENQ, cos = pkt_hdr->cos, queue = the slot of
 *                       dst_queue in the CoS's hash group, 0 without a group
 *   mark                cls_mark when input_flags.cls_mark is set, else 0
 *   hops                no counterpart in the reference: 0 */
static int classify_one(const uint8_t *frame, uint32_t len, ref_result_t *o)
{
	uint8_t *data;
	odp_packet_hdr_t *hdr = ref_fake_packet(frame, len, &data);
	odp_pool_t pool = ODP_POOL_INVALID;
	int r;

	if (!hdr)
		return -1;
	memset(o, 0, sizeof(*o));
	o->cos = 0xFF;
	packet_parse_reset(hdr, 1);
	r = _odp_packet_parse_common(hdr, data, len, len, ODP_PROTO_LAYER_ALL, pktin_opt);
	if (r < 0) {
		o->outcome = OUT_PARSE_DROP;
	} else {
		r = _odp_cls_classify_packet(&the_entry, data, &pool, hdr);
		if (r < 0) {
			o->outcome = OUT_DISCARD;
		} else if (r > 0) {
			o->outcome = OUT_COS_DROP;
		} else {
			o->outcome = OUT_ENQ;
			o->cos = hdr->cos;
			if (_odp_cls_global->cos_tbl.cos_entry[hdr->cos].queue_group)
				o->queue = queue_slot(hdr->cos, hdr->dst_queue);
		}
		if (hdr->p.input_flags.cls_mark)
			o->mark = hdr->cls_mark;
	}
	o->in_flags = (uint32_t)hdr->p.input_flags.all;
	o->err = (uint8_t)hdr->p.flags.all.error;
	o->l3_offset = hdr->p.l3_offset;
	o->l4_offset = hdr->p.l4_offset;
	free(data);
	return 0;
}

/* 0 done, -1 no memory, -2 refused: the rule graph has a cycle */
int ref_classify_batch(const uint8_t *buf, const uint32_t *off, const uint16_t *len, uint32_t n,
		       ref_result_t *out)
{
	uint32_t i;

	if (has_cycle())
		return -2;
	for (i = 0; i < n; i++)
		if (classify_one(buf + off[i], len[i], &out[i]))
			return -1;
	return 0;
}

/* odp_packet_parse + odp_packet_parse_result on the fake packet */
typedef struct {
	int32_t  ret;
	uint32_t in_flags;     /* low word of the header's input_flags */
	uint32_t err;          /* flags.all.error */
	uint32_t l2, l3, l4;   /* the header's offsets */
	uint64_t result_flags; /* odp_packet_parse_result_t.flag.all */
	uint32_t res_len, res_l2, res_l3, res_l4;
	uint32_t l2_type, l3_type, l4_type;
	uint32_t l3_chksum_status, l4_chksum_status;
} ref_parse_out_t;

int ref_packet_parse(const uint8_t *frame, uint32_t len, uint32_t offset, int proto, int layer,
		     uint32_t chksums, ref_parse_out_t *out)
{
	uint8_t *data;
	odp_packet_hdr_t *hdr = ref_fake_packet(frame, len, &data);
	odp_packet_parse_param_t param;
	odp_packet_parse_result_t res;

	if (!hdr)
		return -1;
	packet_parse_reset(hdr, 1);
	memset(&param, 0, sizeof(param));
	param.proto = (odp_proto_t)proto;
	param.last_layer = (odp_proto_layer_t)layer;
	param.chksums.all_chksum = chksums;
	memset(out, 0, sizeof(*out));
	out->ret = odp_packet_parse(packet_handle(hdr), offset, &param);
	odp_packet_parse_result(packet_handle(hdr), &res);
	out->in_flags = (uint32_t)hdr->p.input_flags.all;
	out->err = hdr->p.flags.all.error;
	out->l2 = hdr->p.l2_offset;
	out->l3 = hdr->p.l3_offset;
	out->l4 = hdr->p.l4_offset;
	out->result_flags = res.flag.all;
	out->res_len = res.packet_len;
	out->res_l2 = res.l2_offset;
	out->res_l3 = res.l3_offset;
	out->res_l4 = res.l4_offset;
	out->l2_type = (uint32_t)res.l2_type;
	out->l3_type = (uint32_t)res.l3_type;
	out->l4_type = (uint32_t)res.l4_type;
	out->l3_chksum_status = (uint32_t)res.l3_chksum_status;
	out->l4_chksum_status = (uint32_t)res.l4_chksum_status;
	free(data);
	return 0;
}

#ifdef REF_SHIM_MAIN
/*
 * ref_shim_main CORPUS OUT: a stand-alone program over the same code (a
 * transmit corpus, "RST1": see tx_main below), for a
 * run under the host sanitizers (the fake packet headers and the zero tail
 * are what could be read out of bounds).  CORPUS, written by
 * oracle/reflib.py write_corpus(), all little-endian:
 *   "RSC1", u64 pktin options,
 *   u32 n_ops, then per op one byte kind and
 *     1 cos          u8 action, u8 has_queue, u8 stats, u32 num_queue, u32 hash_proto
 *     2 pmr          u8 n_terms, u32 mark, i32 src, i32 dst (CoS numbers in
 *                    creation order), n_terms ref_term_t
 *     3 pmr_destroy  u32 PMR number        4 cos_destroy  u32 CoS number
 *     5 default      i32 CoS number or -1  6 error        i32 CoS number or -1
 *   u32 n_frames, then per frame u16 len and the bytes.
 * OUT receives the n_frames records, then one ref_parse_out_t per frame and
 * parse offset 0 / 2 / 19 (where the frame is longer) for ETH, IPV4 and IPV6
 * at layer ALL with every checksum on.
 */
static void need(int ok, const char *what)
{
	if (!ok) {
		fprintf(stderr, "ref_shim_main: %s\n", what);
		exit(2);
	}
}

static void rd(FILE *f, void *p, size_t n)
{
	need(fread(p, 1, n, f) == n, "corpus truncated");
}

/*
 * A transmit corpus (oracle/reflib.py write_tx_corpus()), all little-endian:
 *   "RST1", u32 n_opts and the pktout option words, u32 n_hps and the
 *   hash_proto words, u32 n_cases, then per case u16 len, u16 l3, u16 l4,
 *   u8 flags and the bytes.
 * OUT receives, per option word and case, the frame as ref_tx_fix_checksums
 * leaves it, then per hash_proto word and case the six queue indices of
 * ref_tx_dest_queue_batch.  Every frame lives in a heap block of its exact
 * size, and so does every output.
 */
static int tx_main(FILE *f, FILE *o)
{
	uint32_t n_opts, n_hps, n, i, k, opts[64], hps[64];
	long at;

	rd(f, &n_opts, 4);
	need(n_opts <= 64, "too many option rows");
	rd(f, opts, 4 * n_opts);
	rd(f, &n_hps, 4);
	need(n_hps <= 64, "too many hash_proto rows");
	rd(f, hps, 4 * n_hps);
	rd(f, &n, 4);
	at = ftell(f);
	for (k = 0; k < n_opts + n_hps; k++) {
		need(fseek(f, at, SEEK_SET) == 0, "seek");
		for (i = 0; i < n; i++) {
			ref_tx_desc_t d = { 0 };
			uint32_t zero = 0;
			uint16_t len;
			uint8_t *fr, *out;

			rd(f, &len, 2);
			rd(f, &d.l3, 2);
			rd(f, &d.l4, 2);
			rd(f, &d.flags, 1);
			fr = malloc(len ? len : 1);
			need(fr != NULL, "memory");
			rd(f, fr, len);
			if (k < n_opts) {
				out = malloc(len ? len : 1);
				need(out != NULL, "memory");
				need(ref_tx_fix_checksums(fr, len, d.l3, d.l4, d.flags, opts[k], out) == 0, "fix");
				need(fwrite(out, 1, len, o) == len, "write");
			} else {
				out = malloc(REF_TX_NMOD);
				need(out != NULL, "memory");
				need(ref_tx_dest_queue_batch(fr, &zero, &len, &d, 1, hps[k - n_opts], 5, out) == 0,
				     "dest queue");
				need(fwrite(out, 1, REF_TX_NMOD, o) == REF_TX_NMOD, "write");
			}
			free(out);
			free(fr);
		}
	}
	need(fclose(o) == 0, "close");
	fclose(f);
	return 0;
}

int main(int argc, char **argv)
{
	static const uint32_t offs[3] = { 0, 2, 19 };
	uint32_t n_ops, n_frames, i, u, n_cos = 0, n_pmr = 0;
	int cos[1024], pmr[4096];
	uint64_t opt;
	char magic[4];
	FILE *f, *o;

	need(argc == 3, "usage: ref_shim_main CORPUS OUT");
	f = fopen(argv[1], "rb");
	o = fopen(argv[2], "wb");
	need(f && o, "cannot open files");
	rd(f, magic, 4);
	if (!memcmp(magic, "RST1", 4))
		return tx_main(f, o);
	need(!memcmp(magic, "RSC1", 4), "bad magic");
	rd(f, &opt, 8);
	need(ref_reset() == 0, "reset");
	rd(f, &n_ops, 4);
	for (i = 0; i < n_ops; i++) {
		uint8_t kind, b[3];
		int32_t s, d;

		rd(f, &kind, 1);
		if (kind == 1) {
			uint32_t nq, hp;

			rd(f, b, 3);
			rd(f, &nq, 4);
			rd(f, &hp, 4);
			need(n_cos < 1024, "too many CoS");
			cos[n_cos++] = ref_cos_create(b[0], nq, b[1], hp, b[2]);
		} else if (kind == 2) {
			ref_term_t t[255];

			rd(f, b, 1);
			rd(f, &u, 4);
			rd(f, &s, 4);
			rd(f, &d, 4);
			rd(f, t, b[0] * sizeof(t[0]));
			need(n_pmr < 4096 && (uint32_t)s < n_cos && (uint32_t)d < n_cos, "bad pmr op");
			pmr[n_pmr++] = ref_pmr_create(t, b[0], u, cos[s], cos[d]);
		} else if (kind == 3 || kind == 4) {
			rd(f, &u, 4);
			need(u < (kind == 3 ? n_pmr : n_cos), "bad destroy op");
			if (kind == 3)
				ref_pmr_destroy(pmr[u]);
			else
				ref_cos_destroy(cos[u]);
		} else if (kind == 5 || kind == 6) {
			rd(f, &s, 4);
			need(s < (int32_t)n_cos, "bad cos set op");
			if (kind == 5)
				ref_default_cos_set(s < 0 ? 0 : cos[s]);
			else
				ref_error_cos_set(s < 0 ? 0 : cos[s]);
		} else {
			need(0, "bad op kind");
		}
	}
	ref_pktin_opt_set(opt);
	rd(f, &n_frames, 4);
	{
		long at = ftell(f);
		int pass;

		for (pass = 0; pass < 2; pass++) {
			need(fseek(f, at, SEEK_SET) == 0, "seek");
			for (i = 0; i < n_frames; i++) {
				uint16_t len;
				uint32_t zero = 0;
				uint8_t *fr;

				rd(f, &len, 2);
				fr = malloc(len ? len : 1);   /* exact size: no slack to hide an overread */
				need(fr != NULL, "memory");
				rd(f, fr, len);
				if (pass == 0) {
					ref_result_t r;

					need(ref_classify_batch(fr, &zero, &len, 1, &r) == 0, "classify");
					need(fwrite(&r, sizeof(r), 1, o) == 1, "write");
				} else {
					int proto, k;

					for (k = 0; k < 3; k++) {
						if (offs[k] >= len)
							continue;
						for (proto = 1; proto <= 3; proto++) {
							ref_parse_out_t po;

							need(ref_packet_parse(fr, len, offs[k], proto, ODP_PROTO_LAYER_ALL,
									      0xF, &po) == 0, "parse");
							need(fwrite(&po, sizeof(po), 1, o) == 1, "write");
						}
					}
				}
				free(fr);
			}
		}
	}
	need(fclose(o) == 0, "close");
	fclose(f);
	if (_odp_classification_term_global())
		return 1;
	return 0;
}
#endif
