/*
 * lso_driver.c -- test driver for the LSO API of the runtime
 * (odp_lso_profile_*, odp_packet_lso_request*, odp_packet_payload_offset*,
 * odp_pktout_send_lso, odp_pktio_capability_t.lso; tests/test_lso_cpu.py,
 * tests/test_gpu_lso.py).
 *
 *   lso_driver surface [<pcap>]
 *     No GPU needed.  Prints
 *       CAP <loop|pcap> <max_profiles> <max_profiles_per_pktio> <max_packet_segments>
 *           <max_segments> <max_payload_len> <max_payload_offset> <max_num_custom>
 *           <proto bits: custom ipv4 ipv6 tcp_ipv4 tcp_ipv6 sctp_ipv4 sctp_ipv6>
 *           <mod_op bits: add_segment_num add_payload_len add_payload_offset write_bits>
 *       CFG <loop|pcap> <odp_pktio_config with enable_lso>
 *       PROF <case> <1 created | 0 refused>      every accept / reject case
 *       DESTROY <case> <return value>
 *       REQ <case> <values>
 *
 *   lso_driver flow <script>
 *     One pktio; the script's lines, in order:
 *       pool <num> <len>                 the packet pool (first line)
 *       cfg <pktout bits> <pktin bits> [<pktio name>]
 *                                        open ("loop" when no name is given),
 *                                        configure and start the pktio (second line)
 *       prof ipv4 | prof custom <n> {<op> <off> <size> <m0> <m1> <m2> <v0> <v1> <v2>} x n
 *                                        create profile number 0, 1, ...: "H <1|0>"
 *       pkt <hex> <l3 | -1> [<profile> <payload_offset> <max_payload>]
 *                                        a packet for the next send, with an LSO
 *                                        request when the three values are there
 *       send none | send <profile> <payload_offset> <max_payload>
 *                                        odp_pktout_send_lso of the packets so far
 *                                        (opt NULL / given): "R <return value>"; the
 *                                        packets left with the caller are freed
 *       recv                             everything the pktio received, in order:
 *                                        "P <l3 offset> <has_error> <l3 status> <has_lso_request> <hex>"
 *       free                             "F <packets the pool can still give>"
 *       stats                            "T <LSO launches> <of them bounced> <checksum launches>"
 *
 *   lso_driver bench <packets> <len> <payload_offset> <max_payload> <reps>
 *     Times odp_pktout_send_lso of <packets> packets of <len> bytes under a
 *     custom profile (one 2-byte ADD_SEGMENT_NUM) on a loop pktio, after two
 *     warm-up calls: "B <ns of the call> <return value> <segments received>"
 *     per repetition (tools/lso_bench.py).
 *
 *   lso_driver mt <iterations>
 *     Two threads send on one loop pktio at once, <iterations> calls each of
 *     three IPv4 packets -- good, with IP options (the kernel refuses it),
 *     good -- so every call must return 1 and put the first packet's four
 *     segments on the queue.  Then everything is received and checked:
 *     "MT <calls that did not return 1> <segments received> <segments whose
 *     header checksum, IHL or payload bytes are wrong>".
 */
#define _GNU_SOURCE
#include <inttypes.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "odp_api.h"

static void custom_field(odp_lso_profile_param_t *p, int op, uint32_t off, int size)
{
	const int i = p->custom.num_custom++;

	p->custom.field[i].mod_op = (odp_lso_modify_t)op;
	p->custom.field[i].offset = off;
	p->custom.field[i].size = (uint8_t)size;
}

static void prof_case(odp_pktio_t io, const char *name, const odp_lso_profile_param_t *p)
{
	odp_lso_profile_t h = odp_lso_profile_create(io, p);

	printf("PROF %s %d\n", name, h != ODP_LSO_PROFILE_INVALID);
	if (h != ODP_LSO_PROFILE_INVALID && odp_lso_profile_destroy(h))
		printf("PROF %s destroy-failed\n", name);
}

static int surface(const char *pcap, odp_pool_t pool)
{
	const char *names[2] = { "loop", NULL };
	char src[512];
	odp_pktio_t loop = ODP_PKTIO_INVALID;

	if (pcap) {
		snprintf(src, sizeof(src), "pcap:in=%s", pcap);
		names[1] = src;
	}
	for (int k = 0; k < 2 && names[k]; k++) {
		odp_pktio_param_t pp;
		odp_pktio_capability_t c;
		odp_pktio_config_t cfg;
		const char *tag = k ? "pcap" : "loop";

		odp_pktio_param_init(&pp);
		odp_pktio_t io = odp_pktio_open(names[k], pool, &pp);

		if (io == ODP_PKTIO_INVALID || odp_pktio_capability(io, &c))
			return 4;
		printf("CAP %s %u %u %u %u %u %u %u %u%u%u%u%u%u%u %u%u%u%u\n", tag, c.lso.max_profiles,
		       c.lso.max_profiles_per_pktio, c.lso.max_packet_segments, c.lso.max_segments,
		       c.lso.max_payload_len, c.lso.max_payload_offset, c.lso.max_num_custom, c.lso.proto.custom,
		       c.lso.proto.ipv4, c.lso.proto.ipv6, c.lso.proto.tcp_ipv4, c.lso.proto.tcp_ipv6,
		       c.lso.proto.sctp_ipv4, c.lso.proto.sctp_ipv6, c.lso.mod_op.add_segment_num,
		       c.lso.mod_op.add_payload_len, c.lso.mod_op.add_payload_offset, c.lso.mod_op.write_bits);
		printf("MTU %s %u\n", tag, odp_pktio_mtu(io));
		odp_pktio_config_init(&cfg);
		cfg.enable_lso = 1;
		printf("CFG %s %d\n", tag, odp_pktio_config(io, &cfg));
		if (k == 0)
			loop = io;
		else if (odp_pktio_close(io))
			return 5;
	}
	/* ---- profile create: every accept / reject rule (odp_packet_io.c:2844-2923) */
	odp_lso_profile_param_t p;

	odp_lso_profile_param_init(&p);
	printf("INIT %d %d\n", (int)p.lso_proto, p.custom.num_custom);
	prof_case(loop, "none", &p);
	for (int proto = ODP_LSO_PROTO_CUSTOM; proto <= ODP_LSO_PROTO_SCTP_IPV6; proto++) {
		char nm[32];

		odp_lso_profile_param_init(&p);
		p.lso_proto = (odp_lso_protocol_t)proto;
		snprintf(nm, sizeof(nm), "proto%d", proto);
		prof_case(loop, nm, &p);
	}
	const struct { const char *name; int op; uint32_t off; int size; } one[] = {
		{ "segnum1", ODP_LSO_ADD_SEGMENT_NUM, 0, 1 },     { "segnum2", ODP_LSO_ADD_SEGMENT_NUM, 16, 2 },
		{ "segnum4", ODP_LSO_ADD_SEGMENT_NUM, 128, 4 },   { "segnum8", ODP_LSO_ADD_SEGMENT_NUM, 3, 8 },
		{ "segnum3", ODP_LSO_ADD_SEGMENT_NUM, 0, 3 },     { "segnum0", ODP_LSO_ADD_SEGMENT_NUM, 0, 0 },
		{ "segnum16", ODP_LSO_ADD_SEGMENT_NUM, 0, 16 },   { "offset129", ODP_LSO_ADD_SEGMENT_NUM, 129, 1 },
		{ "bits1", ODP_LSO_WRITE_BITS, 128, 1 },          { "bits2", ODP_LSO_WRITE_BITS, 0, 2 },
		{ "bits_offset129", ODP_LSO_WRITE_BITS, 129, 1 }, { "payload_len", ODP_LSO_ADD_PAYLOAD_LEN, 0, 2 },
		{ "payload_offset", ODP_LSO_ADD_PAYLOAD_OFFSET, 0, 2 }, { "op0", 0, 0, 2 }, { "op6", 6, 0, 2 },
	};

	for (unsigned i = 0; i < sizeof(one) / sizeof(one[0]); i++) {
		odp_lso_profile_param_init(&p);
		p.lso_proto = ODP_LSO_PROTO_CUSTOM;
		custom_field(&p, one[i].op, one[i].off, one[i].size);
		prof_case(loop, one[i].name, &p);
	}
	odp_lso_profile_param_init(&p);
	p.lso_proto = ODP_LSO_PROTO_CUSTOM;
	for (int i = 0; i < 8; i++)
		custom_field(&p, ODP_LSO_ADD_SEGMENT_NUM, (uint32_t)i * 8, 8);
	prof_case(loop, "custom8", &p);
	p.custom.num_custom = 9;
	prof_case(loop, "custom9", &p);
	odp_lso_profile_param_init(&p);
	p.lso_proto = ODP_LSO_PROTO_IPV4;
	p.custom.num_custom = 9;       /* read for the custom protocol only (:2857) */
	prof_case(loop, "ipv4_ignores_custom", &p);
	/* the 17th profile; destroy of a stale, a never used and the invalid handle */
	odp_lso_profile_t hs[17];
	int made = 0;

	p.custom.num_custom = 0;
	for (int i = 0; i < 17; i++) {
		hs[i] = odp_lso_profile_create(loop, &p);
		made += hs[i] != ODP_LSO_PROFILE_INVALID;
	}
	printf("PROF sixteen %d\nPROF seventeenth %d\n", made, hs[16] != ODP_LSO_PROFILE_INVALID);
	printf("DESTROY live %d\n", odp_lso_profile_destroy(hs[3]));
	printf("DESTROY stale %d\n", odp_lso_profile_destroy(hs[3]));
	printf("DESTROY invalid %d\n", odp_lso_profile_destroy(ODP_LSO_PROFILE_INVALID));
	hs[3] = odp_lso_profile_create(loop, &p);
	printf("PROF slot_reused %d\n", hs[3] != ODP_LSO_PROFILE_INVALID);
	/* ---- the per-packet request (:2952-2983, odp_packet.c:2452-2470) */
	odp_packet_t pkt = odp_packet_alloc(pool, 100);

	if (pkt == ODP_PACKET_INVALID)
		return 6;
	printf("REQ fresh %d %u\n", odp_packet_has_lso_request(pkt), odp_packet_payload_offset(pkt));
	odp_packet_lso_opt_t o = { .lso_profile = hs[5], .payload_offset = 34, .max_payload_len = 40 };

	int r = odp_packet_lso_request(pkt, &o);   /* calls sequenced: not inside one printf */

	printf("REQ ok %d %d %u\n", r, odp_packet_has_lso_request(pkt), odp_packet_payload_offset(pkt));
	odp_packet_lso_request_clr(pkt);
	printf("REQ clr %d %u\n", odp_packet_has_lso_request(pkt), odp_packet_payload_offset(pkt));
	r = odp_packet_payload_offset_set(pkt, 77);
	printf("REQ offset_set %d %u\n", r, odp_packet_payload_offset(pkt));
	r = odp_packet_payload_offset_set(pkt, 65535);     /* does not fit 16 bits beside INVALID: refused */
	printf("REQ offset_set_65535 %d %u\n", r, odp_packet_payload_offset(pkt));
	r = odp_packet_payload_offset_set(pkt, 65536 + 5);
	printf("REQ offset_set_wide %d %u\n", r, odp_packet_payload_offset(pkt));
	r = odp_packet_payload_offset_set(pkt, 65534);
	printf("REQ offset_set_65534 %d %u\n", r, odp_packet_payload_offset(pkt));
	o.payload_offset = 101;        /* past the packet's 100 bytes */
	r = odp_packet_lso_request(pkt, &o);
	printf("REQ past_packet %d %d\n", r, odp_packet_has_lso_request(pkt));
	o.payload_offset = 100;
	printf("REQ at_end %d\n", odp_packet_lso_request(pkt, &o));
	odp_packet_lso_request_clr(pkt);
	odp_packet_free(pkt);
	pkt = odp_packet_alloc(pool, 400);
	o.payload_offset = 129;
	printf("REQ offset129 %d\n", odp_packet_lso_request(pkt, &o));
	o.payload_offset = 128;
	printf("REQ offset128 %d\n", odp_packet_lso_request(pkt, &o));
	odp_packet_lso_request_clr(pkt);
	o.lso_profile = ODP_LSO_PROFILE_INVALID;
	r = odp_packet_lso_request(pkt, &o);
	printf("REQ invalid_profile %d %d\n", r, odp_packet_has_lso_request(pkt));
	odp_lso_profile_destroy(hs[7]);
	o.lso_profile = hs[7];
	printf("REQ stale_profile %d\n", odp_packet_lso_request(pkt, &o));
	o.lso_profile = hs[5];
	odp_packet_lso_request(pkt, &o);
	odp_packet_free(pkt);
	pkt = odp_packet_alloc(pool, 400);     /* the same buffer again: alloc clears the state */
	printf("REQ realloc %d %u\n", odp_packet_has_lso_request(pkt), odp_packet_payload_offset(pkt));
	/* send_lso on a pktio that is not started (where there is no GPU none
	 * starts): num <= 0, no request, and a good request -- the packet stays
	 * with the caller */
	odp_pktout_queue_t outq;

	memset(&outq, 0, sizeof(outq));
	outq.pktio = loop;
	printf("SEND num0 %d\n", odp_pktout_send_lso(outq, &pkt, 0, NULL));
	printf("SEND norequest %d\n", odp_pktout_send_lso(outq, &pkt, 1, NULL));
	o.payload_offset = 34;
	o.max_payload_len = 40;
	r = odp_packet_lso_request(pkt, &o);
	printf("SEND notstarted %d %d %d\n", r, odp_pktout_send_lso(outq, &pkt, 1, NULL),
	       odp_pktout_send_lso(outq, &pkt, 1, &o));
	printf("SEND kept %d %u\n", odp_packet_has_lso_request(pkt), odp_packet_len(pkt));
	odp_packet_free(pkt);
	return 0;
}

#define MAX_PEND 256
#define MAX_HEX (2 * 65535 + 8)

static uint32_t pool_left(odp_pool_t pool, uint32_t len)
{
	static odp_packet_t hold[65536];
	int n = 0, got;

	while (n < 65536 && (got = odp_packet_alloc_multi(pool, len, hold + n, 65536 - n > 256 ? 256 : 65536 - n)) > 0)
		n += got;
	if (n > 0)
		odp_packet_free_multi(hold, n);
	return (uint32_t)n;
}

static int flow(const char *path)
{
	FILE *f = fopen(path, "r");
	char *line = malloc(MAX_HEX + 256), *hex = malloc(MAX_HEX + 2);
	odp_pool_t pool = ODP_POOL_INVALID;
	odp_pktio_t io = ODP_PKTIO_INVALID;
	odp_pktout_queue_t outq;
	odp_pktin_queue_t inq;
	odp_lso_profile_t prof[32];
	odp_packet_t pend[MAX_PEND];
	int nprof = 0, npend = 0;
	uint32_t pool_len = 0;

	if (!f || !line || !hex)
		return 20;
	while (fgets(line, MAX_HEX + 256, f)) {
		char cmd[16] = "";
		int at = 0;

		if (sscanf(line, "%15s %n", cmd, &at) < 1)
			continue;
		const char *a = line + at;

		if (!strcmp(cmd, "pool")) {
			odp_pool_param_t p;
			uint32_t num = 0;

			sscanf(a, "%u %u", &num, &pool_len);
			odp_pool_param_init(&p);
			p.type = ODP_POOL_PACKET;
			p.pkt.len = pool_len;
			p.pkt.seg_len = pool_len;
			p.pkt.num = num;
			pool = odp_pool_create("pktio_pool", &p);
			if (pool == ODP_POOL_INVALID)
				return 21;
		} else if (!strcmp(cmd, "cfg")) {
			odp_pktio_param_t pp;
			odp_pktio_config_t cfg;
			odp_pktin_queue_param_t iq;
			odp_pktout_queue_param_t oq;
			unsigned long long po = 0, pi = 0;

			char name[512] = "loop";

			sscanf(a, "%llx %llx %511s", &po, &pi, name);
			odp_pktio_param_init(&pp);
			pp.in_mode = ODP_PKTIN_MODE_DIRECT;
			io = odp_pktio_open(name, pool, &pp);
			if (io == ODP_PKTIO_INVALID)
				return 22;
			odp_pktin_queue_param_init(&iq);
			odp_pktout_queue_param_init(&oq);
			if (odp_pktin_queue_config(io, &iq) || odp_pktout_queue_config(io, &oq))
				return 23;
			odp_pktio_config_init(&cfg);
			cfg.parser.layer = ODP_PROTO_LAYER_ALL;
			cfg.pktin.all_bits = pi;
			cfg.pktout.all_bits = po;
			cfg.enable_lso = 1;
			if (odp_pktio_config(io, &cfg) || odp_pktio_start(io) ||
			    odp_pktout_queue(io, &outq, 1) < 1 || odp_pktin_queue(io, &inq, 1) != 1)
				return 24;
		} else if (!strcmp(cmd, "prof")) {
			odp_lso_profile_param_t p;
			char kind[16] = "";
			int n = 0, used = 0;

			odp_lso_profile_param_init(&p);
			sscanf(a, "%15s %d %n", kind, &n, &used);
			a += used;
			p.lso_proto = !strcmp(kind, "ipv4") ? ODP_LSO_PROTO_IPV4 : ODP_LSO_PROTO_CUSTOM;
			for (int i = 0; i < n && i < ODP_LSO_MAX_CUSTOM; i++) {
				unsigned op, off, size, m[3], v[3];

				if (sscanf(a, "%u %u %u %u %u %u %u %u %u %n", &op, &off, &size, &m[0], &m[1], &m[2], &v[0],
					   &v[1], &v[2], &used) < 9)
					return 25;
				a += used;
				custom_field(&p, (int)op, off, (int)size);
				p.custom.field[i].write_bits.first_seg.mask[0] = (uint8_t)m[0];
				p.custom.field[i].write_bits.middle_seg.mask[0] = (uint8_t)m[1];
				p.custom.field[i].write_bits.last_seg.mask[0] = (uint8_t)m[2];
				p.custom.field[i].write_bits.first_seg.value[0] = (uint8_t)v[0];
				p.custom.field[i].write_bits.middle_seg.value[0] = (uint8_t)v[1];
				p.custom.field[i].write_bits.last_seg.value[0] = (uint8_t)v[2];
			}
			prof[nprof] = odp_lso_profile_create(io, &p);
			printf("H %d\n", prof[nprof] != ODP_LSO_PROFILE_INVALID);
			nprof++;
		} else if (!strcmp(cmd, "pkt")) {
			int l3 = -1, pi = -1;
			unsigned po = 0, mp = 0;
			const int got = sscanf(a, "%131078s %d %d %u %u", hex, &l3, &pi, &po, &mp);
			const uint32_t len = (uint32_t)strlen(hex) / 2;

			if (got < 2 || npend == MAX_PEND)
				return 26;
			odp_packet_t pkt = odp_packet_alloc(pool, len);

			if (pkt == ODP_PACKET_INVALID)
				return 27;
			uint8_t *d = odp_packet_data(pkt);

			for (uint32_t i = 0; i < len; i++) {
				unsigned b;

				sscanf(hex + 2 * i, "%2x", &b);
				d[i] = (uint8_t)b;
			}
			if (l3 >= 0)
				odp_packet_l3_offset_set(pkt, (uint32_t)l3);
			if (got == 5) {
				const odp_packet_lso_opt_t o = { .lso_profile = prof[pi], .payload_offset = po,
								 .max_payload_len = mp };

				if (odp_packet_lso_request(pkt, &o))
					return 28;
			}
			pend[npend++] = pkt;
		} else if (!strcmp(cmd, "send")) {
			int pi = -1;
			unsigned po = 0, mp = 0;
			odp_packet_lso_opt_t o;
			const int with = sscanf(a, "%d %u %u", &pi, &po, &mp) == 3;

			if (with)
				o = (odp_packet_lso_opt_t){ .lso_profile = prof[pi], .payload_offset = po, .max_payload_len = mp };
			const int r = odp_pktout_send_lso(outq, pend, npend, with ? &o : NULL);

			printf("R %d\n", r);
			for (int i = r > 0 ? r : 0; i < npend; i++)
				odp_packet_free(pend[i]);
			npend = 0;
		} else if (!strcmp(cmd, "recv")) {
			odp_packet_t pk[256];
			int idle = 0;

			while (idle < 3) {
				const int n = odp_pktin_recv(inq, pk, 256);

				for (int i = 0; i < n; i++) {
					const uint8_t *d = odp_packet_data(pk[i]);
					const uint32_t len = odp_packet_len(pk[i]);

					printf("P %u %d %d %d ", odp_packet_l3_offset(pk[i]), odp_packet_has_error(pk[i]),
					       (int)odp_packet_l3_chksum_status(pk[i]), odp_packet_has_lso_request(pk[i]));
					for (uint32_t b = 0; b < len; b++)
						printf("%02x", d[b]);
					printf("\n");
					odp_packet_free(pk[i]);
				}
				idle = (n == 0 && odp_amd_pktio_rx_idle(io) == 1) ? idle + 1 : 0;
			}
		} else if (!strcmp(cmd, "free")) {
			printf("F %u\n", pool_left(pool, pool_len));
		} else if (!strcmp(cmd, "stats")) {
			uint64_t lb = 0, lo = 0, tb = 0, to = 0;

			odp_amd_pktio_lso_stats(io, &lb, &lo);
			odp_amd_pktio_tx_stats(io, &tb, &to);
			printf("T %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", lb, lo, tb);
		}
	}
	fclose(f);
	if (io != ODP_PKTIO_INVALID) {
		odp_pktio_stop(io);
		odp_pktio_close(io);
	}
	return 0;
}

static int bench(int n, uint32_t len, uint32_t po, uint32_t mp, int reps)
{
	odp_pool_param_t p;
	odp_pktio_param_t pp;
	odp_pktio_config_t cfg;
	odp_pktout_queue_t outq;
	odp_pktin_queue_t inq;
	odp_lso_profile_param_t lp;
	odp_packet_t *pk = malloc(sizeof(*pk) * (size_t)n), rx[256];

	if (!pk || n <= 0 || len <= po || mp == 0)
		return 30;
	odp_pool_param_init(&p);
	p.type = ODP_POOL_PACKET;
	p.pkt.len = len;
	p.pkt.seg_len = len;
	p.pkt.num = (uint32_t)n * (2u + (len - po) / mp) + 64u;
	odp_pool_t pool = odp_pool_create("pktio_pool", &p);

	odp_pktio_param_init(&pp);
	pp.in_mode = ODP_PKTIN_MODE_DIRECT;
	odp_pktio_t io = pool == ODP_POOL_INVALID ? ODP_PKTIO_INVALID : odp_pktio_open("loop", pool, &pp);

	if (io == ODP_PKTIO_INVALID || odp_pktin_queue_config(io, NULL) || odp_pktout_queue_config(io, NULL))
		return 31;
	odp_pktio_config_init(&cfg);
	cfg.parser.layer = ODP_PROTO_LAYER_L2;
	cfg.enable_lso = 1;
	if (odp_pktio_config(io, &cfg) || odp_pktio_start(io) || odp_pktout_queue(io, &outq, 1) < 1 ||
	    odp_pktin_queue(io, &inq, 1) != 1)
		return 32;
	odp_lso_profile_param_init(&lp);
	lp.lso_proto = ODP_LSO_PROTO_CUSTOM;
	custom_field(&lp, ODP_LSO_ADD_SEGMENT_NUM, 16, 2);
	const odp_packet_lso_opt_t o = { .lso_profile = odp_lso_profile_create(io, &lp), .payload_offset = po,
					 .max_payload_len = mp };

	if (o.lso_profile == ODP_LSO_PROFILE_INVALID)
		return 33;
	for (int r = -2; r < reps; r++) {
		if (odp_packet_alloc_multi(pool, len, pk, n) != n)
			return 34;
		for (int i = 0; i < n; i++)
			memset(odp_packet_data(pk[i]), 0x40 + (i & 63), len);
		const odp_time_t t0 = odp_time_local();
		const int sent = odp_pktout_send_lso(outq, pk, n, &o);
		const uint64_t ns = odp_time_diff_ns(odp_time_local(), t0);
		long got = 0;
		int idle = 0;

		for (int i = sent > 0 ? sent : 0; i < n; i++)
			odp_packet_free(pk[i]);
		while (idle < 3) {
			const int k = odp_pktin_recv(inq, rx, 256);

			if (k > 0)
				odp_packet_free_multi(rx, k);
			got += k > 0 ? k : 0;
			idle = (k == 0 && odp_amd_pktio_rx_idle(io) == 1) ? idle + 1 : 0;
		}
		if (r >= 0)
			printf("B %" PRIu64 " %d %ld\n", ns, sent, got);
	}
	odp_pktio_stop(io);
	odp_pktio_close(io);
	free(pk);
	return 0;
}

#define MT_LEN (34u + 3u * 64u + 9u)

typedef struct mt_arg {
	odp_instance_t inst;
	odp_pool_t pool;
	odp_pktout_queue_t outq;
	odp_packet_lso_opt_t opt;
	int iters, tag, bad;
} mt_arg_t;

static void *mt_main(void *arg)
{
	mt_arg_t *t = arg;

	if (odp_init_local(t->inst, ODP_THREAD_WORKER)) {
		t->bad = -1;
		return NULL;
	}
	for (int it = 0; it < t->iters; it++) {
		odp_packet_t pk[3];

		if (odp_packet_alloc_multi(t->pool, MT_LEN, pk, 3) != 3) {
			t->bad = -1;
			break;
		}
		for (int i = 0; i < 3; i++) {
			uint8_t *d = odp_packet_data(pk[i]);

			memset(d, t->tag, MT_LEN);
			d[14] = i == 1 ? 0x46 : 0x45;
			d[20] = d[21] = 0;
			odp_packet_l3_offset_set(pk[i], 14);
		}
		const int r = odp_pktout_send_lso(t->outq, pk, 3, &t->opt);

		t->bad += r != 1;
		for (int i = r > 0 ? r : 0; i < 3; i++)
			odp_packet_free(pk[i]);
	}
	odp_term_local();
	return NULL;
}

static int mt(odp_instance_t inst, int iters)
{
	odp_pool_param_t p;
	odp_pktio_param_t pp;
	odp_pktio_config_t cfg;
	odp_pktin_queue_t inq;
	odp_lso_profile_param_t lp;
	mt_arg_t t[2];
	pthread_t th[2];
	odp_packet_t rx[256];

	odp_pool_param_init(&p);
	p.type = ODP_POOL_PACKET;
	p.pkt.len = 512;
	p.pkt.seg_len = 512;
	p.pkt.num = (uint32_t)iters * 8u + 256u;
	odp_pool_t pool = odp_pool_create("pktio_pool", &p);

	odp_pktio_param_init(&pp);
	pp.in_mode = ODP_PKTIN_MODE_DIRECT;
	odp_pktio_t io = pool == ODP_POOL_INVALID ? ODP_PKTIO_INVALID : odp_pktio_open("loop", pool, &pp);

	if (io == ODP_PKTIO_INVALID || odp_pktin_queue_config(io, NULL) || odp_pktout_queue_config(io, NULL))
		return 40;
	odp_pktio_config_init(&cfg);
	cfg.enable_lso = 1;
	if (odp_pktio_config(io, &cfg) || odp_pktio_start(io) || odp_pktin_queue(io, &inq, 1) != 1)
		return 41;
	odp_lso_profile_param_init(&lp);
	lp.lso_proto = ODP_LSO_PROTO_IPV4;
	for (int k = 0; k < 2; k++) {
		memset(&t[k], 0, sizeof(t[k]));
		t[k].inst = inst;
		t[k].pool = pool;
		t[k].iters = iters;
		t[k].tag = 0x51 + k;
		t[k].opt = (odp_packet_lso_opt_t){ .lso_profile = odp_lso_profile_create(io, &lp),
						   .payload_offset = 34, .max_payload_len = 64 };
		if (t[k].opt.lso_profile == ODP_LSO_PROFILE_INVALID || odp_pktout_queue(io, &t[k].outq, 1) < 1)
			return 42;
	}
	for (int k = 0; k < 2; k++)
		if (pthread_create(&th[k], NULL, mt_main, &t[k]))
			return 43;
	for (int k = 0; k < 2; k++)
		pthread_join(th[k], NULL);
	if (t[0].bad < 0 || t[1].bad < 0)
		return 44;
	long got = 0, wrong = 0;
	int idle = 0;

	while (idle < 3) {
		const int n = odp_pktin_recv(inq, rx, 256);

		for (int i = 0; i < n; i++) {
			const uint8_t *d = odp_packet_data(rx[i]);
			const uint32_t len = odp_packet_len(rx[i]);
			uint32_t sum = 0;
			int ok = len > 34 && len <= 34 + 64 && d[14] == 0x45 && (d[0] == 0x51 || d[0] == 0x52);

			for (uint32_t b = 14; ok && b < 34; b += 2)
				sum += (uint32_t)d[b] << 8 | d[b + 1];
			sum = (sum & 0xffffu) + (sum >> 16);
			sum = (sum & 0xffffu) + (sum >> 16);
			ok = ok && sum == 0xffffu;
			for (uint32_t b = 34; ok && b < len; b++)
				ok = d[b] == d[0];
			wrong += !ok;
		}
		if (n > 0)
			odp_packet_free_multi(rx, n);
		got += n > 0 ? n : 0;
		idle = (n == 0 && odp_amd_pktio_rx_idle(io) == 1) ? idle + 1 : 0;
	}
	printf("MT %d %ld %ld\n", t[0].bad + t[1].bad, got, wrong);
	odp_pktio_stop(io);
	odp_pktio_close(io);
	return 0;
}

int main(int argc, char *argv[])
{
	odp_instance_t inst;

	if (argc < 2) {
		fprintf(stderr, "usage: %s surface [<pcap>] | flow <script> | mt <iterations> | bench <n> <len> <off> <payload> <reps>\n",
			argv[0]);
		return 2;
	}
	if (odp_init_global(&inst, NULL, NULL) || odp_init_local(inst, ODP_THREAD_CONTROL))
		return 3;
	odp_schedule_config(NULL);
	if (strcmp(argv[1], "surface") == 0) {
		odp_pool_param_t p;

		odp_pool_param_init(&p);
		p.type = ODP_POOL_PACKET;
		p.pkt.len = 1856;
		p.pkt.seg_len = 1856;
		p.pkt.num = 64;
		odp_pool_t pool = odp_pool_create("pktio_pool", &p);

		return pool == ODP_POOL_INVALID ? 3 : surface(argc > 2 ? argv[2] : NULL, pool);
	}
	if (strcmp(argv[1], "mt") == 0 && argc > 2)
		return mt(inst, atoi(argv[2]));
	if (strcmp(argv[1], "bench") == 0 && argc > 6)
		return bench(atoi(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), (uint32_t)atoi(argv[5]),
			     atoi(argv[6]));
	return argc > 2 ? flow(argv[2]) : 2;
}
