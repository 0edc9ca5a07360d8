/*
 * parse_driver.c -- test driver for odp_packet_parse / odp_packet_parse_multi,
 * odp_packet_parse_result and odp_packet_l2/l3/l4_type.  Test infrastructure
 * only.
 *
 * usage: parse_driver surface
 *     No GPU needed.  Output lines:
 *       N <parse proto NONE> <layer NONE> <offset == len> <multi: the same three>
 *       G <odp_packet_parse of a good frame> <odp_packet_parse_multi of two>
 *       X <input_flags hex> <err hex> <l2 type> <l3 type> <l4 type> <l3 status>
 *         <l4 status> <result flag word hex> <packet_len> <l2> <l3> <l4>
 *           odp_packet_parse_result / the type accessors of a packet whose
 *           metadata was set by hand (flags and errors written into the
 *           header, offsets with the setters), through _multi
 *
 *        parse_driver run <file>
 *     <file> lines:
 *       C <name> <proto> <last_layer> <chksums> <plus> <hex frame>
 *           the reference's case shape (test/validation/api/packet/packet.c:
 *           3718-3783): ten packets with the frame behind the ten L2 offsets,
 *           odp_packet_parse(pkt[0], plus) and odp_packet_parse_multi of the
 *           other nine from offset + plus.  Output:
 *             R <name> <parse return> <multi return>
 *             P <name> <i> <flags> <err> <l2> <l3> <l4> <l2 type> <l3 type>
 *               <l4 type> <l3 status> <l4 status> <result word> <packet_len>
 *               <l3 status before> <l4 status before>      (0 unknown 1 bad 2 ok)
 *       M <good hex frame> <failing hex frame>
 *           eight packets, the failing frame at index 3, sentinel offsets
 *           (l3 5, l4 7) on all: "M <multi return>" and per packet
 *           "MP <i> <flags> <err> <l2> <l3> <l4>"; then "U <user pointer kept>
 *           <tx override bits hex>" of a packet parsed with a user pointer and
 *           odp_packet_l4_chksum_insert(pkt, 1) set; "N ..." as above; two
 *           threads parsing ten packets each at the same time, "T <thread>
 *           <i> <return> <flags> <err> <l2> <l3> <l4>"; and "B <1 if any call
 *           went through the bounce buffer>".
 *
 *        parse_driver batch <file>
 *     Whole odp_packet_parse_multi calls of any size, over one or two pools
 *     ("parse_pool", "parse_pool2": ODP_AMD_PAGEABLE_POOLS picks which are
 *     pageable).  <file> lines:
 *       F <hex frame>       one more frame of the frame list
 *       B <n> <pools>       one call (ETH, ALL, all checksums) on n packets:
 *           packet i holds frame i % frames behind L2 offset i % 10 and comes
 *           from pool i % pools.  Output: "Q <return> <calls> <bounced>" (what
 *           odp_amd_packet_parse_stats counted for this call) and per packet
 *           "QP <i> <flags> <err> <l2> <l3> <l4>".
 */
#define _GNU_SOURCE
#include <inttypes.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "odp_api.h"

#define NPKT 10
static const uint32_t l2_offset[NPKT] = { 0, 2, 8, 12, 19, 36, 64, 120, 207, 0 };

/* the packet header's metadata block (odp_rt_internal.h pkt_hdr_t: at byte 64;
 * in_flags at +8, err at +16, the pktout override bits at +26) */
uint8_t *rt_pkt_hdr(odp_packet_t pkt);
#define META(pkt) (rt_pkt_hdr(pkt) + 64)

static odp_pool_t pool;
static odp_instance_t inst;

static int unhex(const char *s, uint8_t *out, int cap)
{
	int n = 0;

	for (; s[0] && s[1] && s[0] != '\n' && n < cap; s += 2, n++) {
		unsigned v;

		if (sscanf(s, "%2x", &v) != 1)
			return -1;
		out[n] = (uint8_t)v;
	}
	return n;
}

static odp_packet_t mkpkt(const uint8_t *frame, uint32_t len, uint32_t offs)
{
	odp_packet_t pkt = odp_packet_alloc(pool, len + offs);
	uint8_t fill[256];

	if (pkt == ODP_PACKET_INVALID)
		exit(10);
	for (uint32_t i = 0; i < offs; i++)
		fill[i] = (uint8_t)i;
	if ((offs && odp_packet_copy_from_mem(pkt, 0, offs, fill)) ||
	    odp_packet_copy_from_mem(pkt, offs, len, frame))
		exit(11);
	return pkt;
}

static uint64_t flags_of(odp_packet_t pkt)
{
	uint64_t f;

	memcpy(&f, META(pkt) + 8, 8);
	return f;
}

static void meta_line(const char *tag, odp_packet_t pkt)
{
	printf("%s 0x%" PRIx64 " 0x%x %u %u %u", tag, flags_of(pkt), META(pkt)[16],
	       odp_packet_l2_offset(pkt), odp_packet_l3_offset(pkt), odp_packet_l4_offset(pkt));
}

static void result_line(odp_packet_t pkt)
{
	odp_packet_parse_result_t r, *rp = &r;

	memset(&r, 0xA5, sizeof(r));
	odp_packet_parse_result_multi(&pkt, &rp, 1);
	if (r.l2_offset != odp_packet_l2_offset(pkt) || r.l3_offset != odp_packet_l3_offset(pkt) ||
	    r.l4_offset != odp_packet_l4_offset(pkt) || r.l2_type != odp_packet_l2_type(pkt) ||
	    r.l3_type != odp_packet_l3_type(pkt) || r.l4_type != odp_packet_l4_type(pkt) ||
	    r.l3_chksum_status != odp_packet_l3_chksum_status(pkt) ||
	    r.l4_chksum_status != odp_packet_l4_chksum_status(pkt))
		exit(12);
	printf(" %u 0x%x %u %d %d 0x%" PRIx64 " %u", r.l2_type, r.l3_type, r.l4_type, (int)r.l3_chksum_status,
	       (int)r.l4_chksum_status, (uint64_t)r.flag.all, r.packet_len);
}

static void none_line(const uint8_t *frame, uint32_t len)
{
	odp_packet_t pkt = mkpkt(frame, len, 0);
	odp_packet_parse_param_t p = { ODP_PROTO_NONE, ODP_PROTO_LAYER_ALL, { .all_chksum = 0 } };
	odp_packet_parse_param_t q = { ODP_PROTO_ETH, ODP_PROTO_LAYER_NONE, { .all_chksum = 0 } };
	odp_packet_parse_param_t ok = { ODP_PROTO_ETH, ODP_PROTO_LAYER_ALL, { .all_chksum = 0 } };
	uint32_t zero = 0, end = len;

	odp_packet_l3_offset_set(pkt, 5);
	printf("N %d %d %d %d %d %d\n", odp_packet_parse(pkt, 0, &p), odp_packet_parse(pkt, 0, &q),
	       odp_packet_parse(pkt, len, &ok), odp_packet_parse_multi(&pkt, &zero, 1, &p),
	       odp_packet_parse_multi(&pkt, &zero, 1, &q), odp_packet_parse_multi(&pkt, &end, 1, &ok));
	if (odp_packet_l3_offset(pkt) != 5 || flags_of(pkt) != 0)   /* nothing was touched */
		exit(13);
	odp_packet_free(pkt);
}

static int surface(void)
{
	const uint8_t frame[60] = { 2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 0x08, 0x00, 0x45, 0, 0, 46, 0, 0, 0, 0,
				    64, 17, 0x66, 0xa6, 10, 0, 0, 1, 10, 0, 0, 100, 4, 0, 8, 0, 0, 26 };
	odp_packet_parse_param_t ok = { ODP_PROTO_ETH, ODP_PROTO_LAYER_ALL, { .all_chksum = 0 } };
	const uint32_t offs[2] = { 0, 0 };
	odp_packet_t pk[2] = { mkpkt(frame, sizeof(frame), 0), mkpkt(frame, sizeof(frame), 0) };

	none_line(frame, sizeof(frame));
	printf("G %d", odp_packet_parse(pk[0], 0, &ok));
	printf(" %d\n", odp_packet_parse_multi(pk, offs, 2, &ok));
	/* hand-set metadata: one word per flag, and a few mixed ones */
	uint64_t words[40];
	int nw = 0;

	for (int b = 3; b <= 26; b++)
		words[nw++] = 1ull << b;
	words[nw++] = 0x402078;                 /* eth ipv4 udp */
	words[nw++] = 0x2002078;                /* icmp over ipv4 */
	words[nw++] = 0x2004078;                /* icmp over ipv6 */
	words[nw++] = 0xC0802078ull;            /* tcp, both checksums done */
	for (int i = 0; i < nw; i++) {
		for (int e = 0; e < 2; e++) {
			const uint8_t err = e ? (uint8_t)(1u << (i % 7)) : 0;

			memcpy(META(pk[0]) + 8, &words[i], 8);
			META(pk[0])[16] = err;
			odp_packet_l2_offset_set(pk[0], 1);
			odp_packet_l3_offset_set(pk[0], 15);
			odp_packet_l4_offset_set(pk[0], 35);
			meta_line("X", pk[0]);
			result_line(pk[0]);
			printf("\n");
		}
	}
	odp_packet_free_multi(pk, 2);
	return 0;
}

static void run_case(const char *name, int proto, int layer, unsigned sel, uint32_t plus,
		     const uint8_t *frame, uint32_t len)
{
	odp_packet_t pkt[NPKT];
	uint32_t offs[NPKT];
	int pre3[NPKT], pre4[NPKT];
	odp_packet_parse_param_t parse;

	for (int i = 0; i < NPKT; i++) {
		pkt[i] = mkpkt(frame, len, l2_offset[i]);
		offs[i] = l2_offset[i] + plus;
		pre3[i] = (int)odp_packet_l3_chksum_status(pkt[i]);
		pre4[i] = (int)odp_packet_l4_chksum_status(pkt[i]);
	}
	parse.proto = (odp_proto_t)proto;
	parse.last_layer = (odp_proto_layer_t)layer;
	parse.chksums.all_chksum = sel;
	const int r0 = odp_packet_parse(pkt[0], offs[0], &parse);
	const int rm = odp_packet_parse_multi(&pkt[1], offs + 1, NPKT - 1, &parse);

	printf("R %s %d %d\n", name, r0, rm);
	for (int i = 0; i < NPKT; i++) {
		char tag[96];

		snprintf(tag, sizeof(tag), "P %s %d", name, i);
		meta_line(tag, pkt[i]);
		result_line(pkt[i]);
		printf(" %d %d\n", pre3[i], pre4[i]);
	}
	odp_packet_free_multi(pkt, NPKT);
}

static void multi_stop(const uint8_t *good, uint32_t glen, const uint8_t *bad, uint32_t blen)
{
	odp_packet_t pkt[8];
	uint32_t offs[8] = { 0 };
	odp_packet_parse_param_t parse = { ODP_PROTO_ETH, ODP_PROTO_LAYER_ALL, { .all_chksum = 0xF } };

	for (int i = 0; i < 8; i++) {
		pkt[i] = i == 3 ? mkpkt(bad, blen, 0) : mkpkt(good, glen, 0);
		odp_packet_l3_offset_set(pkt[i], 5);
		odp_packet_l4_offset_set(pkt[i], 7);
	}
	printf("M %d\n", odp_packet_parse_multi(pkt, offs, 8, &parse));
	for (int i = 0; i < 8; i++) {
		char tag[32];

		snprintf(tag, sizeof(tag), "MP %d", i);
		meta_line(tag, pkt[i]);
		printf("\n");
	}
	/* user pointer and a pktout override survive (packet_parse_reset(hdr, 0)) */
	uint16_t ovr;

	odp_packet_user_ptr_set(pkt[7], &parse);
	odp_packet_l4_chksum_insert(pkt[7], 1);
	if (odp_packet_parse(pkt[7], 0, &parse))
		exit(14);
	memcpy(&ovr, META(pkt[7]) + 26, 2);
	printf("U %d 0x%x\n", odp_packet_user_ptr(pkt[7]) == (void *)&parse, ovr);
	odp_packet_free_multi(pkt, 8);
}

struct thr {
	int id;
	const uint8_t *frame;
	uint32_t len;
	odp_packet_t pkt[NPKT];
	int ret[NPKT];
};

static void *thr_main(void *arg)
{
	struct thr *t = arg;
	odp_packet_parse_param_t parse = { ODP_PROTO_ETH, ODP_PROTO_LAYER_ALL, { .all_chksum = 0xF } };

	if (odp_init_local(inst, ODP_THREAD_WORKER))
		exit(15);
	/* single calls and a multi call, several rounds, beside the other thread */
	for (int round = 0; round < 8; round++) {
		for (int i = 0; i < NPKT / 2; i++)
			t->ret[i] = odp_packet_parse(t->pkt[i], l2_offset[i], &parse);
		const int n = odp_packet_parse_multi(&t->pkt[NPKT / 2], &l2_offset[NPKT / 2], NPKT - NPKT / 2,
						     &parse);

		for (int i = NPKT / 2; i < NPKT; i++)
			t->ret[i] = i - NPKT / 2 < n ? 0 : -1;
	}
	odp_term_local();
	return NULL;
}

static void two_threads(const uint8_t *frame, uint32_t len)
{
	struct thr t[2];
	pthread_t th[2];

	for (int k = 0; k < 2; k++) {
		t[k].id = k;
		for (int i = 0; i < NPKT; i++)
			t[k].pkt[i] = mkpkt(frame, len, l2_offset[i]);
	}
	for (int k = 0; k < 2; k++)
		if (pthread_create(&th[k], NULL, thr_main, &t[k]))
			exit(16);
	for (int k = 0; k < 2; k++)
		pthread_join(th[k], NULL);
	for (int k = 0; k < 2; k++) {
		for (int i = 0; i < NPKT; i++) {
			char tag[32];

			snprintf(tag, sizeof(tag), "T %d %d %d", k, i, t[k].ret[i]);
			meta_line(tag, t[k].pkt[i]);
			printf("\n");
		}
		odp_packet_free_multi(t[k].pkt, NPKT);
	}
}

#define BATCH_FRAMES 32
#define BATCH_MAX 2048

static int batch(FILE *f, odp_pool_t pool2)
{
	static char line[8192], hex[4096];
	static uint8_t frame[BATCH_FRAMES][2048];
	static odp_packet_t pkt[BATCH_MAX];
	static uint32_t offs[BATCH_MAX];
	uint32_t flen[BATCH_FRAMES];
	const odp_pool_t pools[2] = { pool, pool2 };
	const odp_packet_parse_param_t parse = { ODP_PROTO_ETH, ODP_PROTO_LAYER_ALL, { .all_chksum = 0xF } };
	unsigned nf = 0, n, np;

	while (fgets(line, sizeof(line), f)) {
		if (sscanf(line, "F %4095s", hex) == 1) {
			const int l = nf < BATCH_FRAMES ? unhex(hex, frame[nf], sizeof(frame[nf])) : -1;

			if (l <= 0)
				return 5;
			flen[nf++] = (uint32_t)l;
		} else if (sscanf(line, "B %u %u", &n, &np) == 2) {
			uint64_t c0, b0, c1, b1;

			if (!nf || !n || n > BATCH_MAX || np < 1 || np > 2)
				return 5;
			for (unsigned i = 0; i < n; i++) {
				pool = pools[i % np];
				offs[i] = l2_offset[i % NPKT];
				pkt[i] = mkpkt(frame[i % nf], flen[i % nf], offs[i]);
			}
			pool = pools[0];
			odp_amd_packet_parse_stats(&c0, &b0);
			const int r = odp_packet_parse_multi(pkt, offs, (int)n, &parse);

			odp_amd_packet_parse_stats(&c1, &b1);
			printf("Q %d %" PRIu64 " %" PRIu64 "\n", r, c1 - c0, b1 - b0);
			for (unsigned i = 0; i < n; i++) {
				char tag[32];

				snprintf(tag, sizeof(tag), "QP %u", i);
				meta_line(tag, pkt[i]);
				printf("\n");
			}
			odp_packet_free_multi(pkt, (int)n);
		}
	}
	return 0;
}

int main(int argc, char *argv[])
{
	odp_pool_param_t pp;

	if (argc < 2 || (strcmp(argv[1], "surface") &&
			 ((strcmp(argv[1], "run") && strcmp(argv[1], "batch")) || argc < 3))) {
		fprintf(stderr, "usage: %s surface | run <file> | batch <file>\n", argv[0]);
		return 2;
	}
	const int is_batch = strcmp(argv[1], "batch") == 0;

	if (odp_init_global(&inst, NULL, NULL) || odp_init_local(inst, ODP_THREAD_CONTROL))
		return 3;
	odp_pool_param_init(&pp);
	pp.type = ODP_POOL_PACKET;
	pp.pkt.len = 1856;
	pp.pkt.seg_len = 1856;
	pp.pkt.num = is_batch ? BATCH_MAX : 256;
	pool = odp_pool_create("parse_pool", &pp);
	if (pool == ODP_POOL_INVALID)
		return 3;
	if (strcmp(argv[1], "surface") == 0)
		return surface();

	FILE *f = fopen(argv[2], "r");
	static char line[8192], name[64], hex[4096], hex2[4096];
	static uint8_t frame[2048], frame2[2048];

	if (!f)
		return 4;
	if (is_batch) {
		odp_pool_t pool2 = odp_pool_create("parse_pool2", &pp);
		const int rc = pool2 == ODP_POOL_INVALID ? 3 : batch(f, pool2);

		fclose(f);
		if (rc)
			return rc;
		odp_pool_destroy(pool2);
		odp_pool_destroy(pool);
		odp_term_local();
		return odp_term_global(inst) ? 6 : 0;
	}
	while (fgets(line, sizeof(line), f)) {
		int proto, layer;
		unsigned sel, plus;

		if (sscanf(line, "C %63s %d %d %u %u %4095s", name, &proto, &layer, &sel, &plus, hex) == 6) {
			const int n = unhex(hex, frame, sizeof(frame));

			if (n <= 0)
				return 5;
			run_case(name, proto, layer, sel, plus, frame, (uint32_t)n);
		} else if (sscanf(line, "M %4095s %4095s", hex, hex2) == 2) {
			const int n = unhex(hex, frame, sizeof(frame)), m = unhex(hex2, frame2, sizeof(frame2));

			if (n <= 0 || m <= 0)
				return 5;
			multi_stop(frame, (uint32_t)n, frame2, (uint32_t)m);
			none_line(frame, (uint32_t)n);
			two_threads(frame, (uint32_t)n);
		}
	}
	fclose(f);
	uint64_t calls = 0, bounced = 0;

	odp_amd_packet_parse_stats(&calls, &bounced);
	printf("B %d\n", bounced != 0);
	odp_pool_destroy(pool);
	odp_term_local();
	return odp_term_global(inst) ? 6 : 0;
}
