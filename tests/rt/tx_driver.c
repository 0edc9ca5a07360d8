/*
 * tx_driver.c -- test driver for the pktout checksum insertion of the loop
 * pktio (odp_pktio_capability / odp_pktio_config pktout bits,
 * odp_packet_l3_chksum_insert / odp_packet_l4_chksum_insert,
 * odp_pktout_send).  Test infrastructure only.
 *
 * usage: tx_driver surface <pcap>
 *     The API surface, no GPU needed.  Output lines:
 *       CAP <loop|pcap> <capability.config.pktout.all_bits hex>
 *       CFG <loop|pcap> <bits hex> <odp_pktio_config return>
 *       OVR ok        both override setters were called on a packet
 *
 *        tx_driver loop <pcap> <pktout bits> <pktin bits> <ovr>
 *     Round trip: the frames of <pcap> (read through a parse-less pcap pktio)
 *     get their l3 / l4 offsets set, are sent into a loop pktio configured
 *     with the pktout / pktin option bits, and received again.
 *     <ovr>: 0 none; 1 odp_packet_l4_chksum_insert(pkt, 0) on every odd
 *     packet; 2 odp_packet_l3/l4_chksum_insert(pkt, 1) on every packet;
 *     3 odp_packet_l4_chksum_insert(pkt, 0) on every packet, and the received
 *     packets are sent and received a second time as they came back (a
 *     received packet carries no override).
 *     Output lines, in arrival order:
 *       P <l3 status> <l4 status> <has_error> <hex frame>   (0 unknown 1 bad 2 ok)
 *       S <in_packets> <in_errors>
 *       T <sends that ran the kernel> <of them through the bounce buffer>
 *     TX_COUNT_ONLY=1: no P lines; "R <packets> <send ns>" (time in
 *     odp_pktout_send, tools/tx_bench.py).
 */
#define _GNU_SOURCE
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "odp_api.h"

static odp_pool_t mkpool(const char *name)
{
	odp_pool_param_t p;

	odp_pool_param_init(&p);
	p.type = ODP_POOL_PACKET;
	p.pkt.len = 1856;
	p.pkt.seg_len = 1856;
	p.pkt.num = getenv("TX_POOL_NUM") ? (uint32_t)atoi(getenv("TX_POOL_NUM")) : 4096;
	return odp_pool_create(name, &p);
}

/* l3 / l4 of a well-formed Ethernet frame: tags skipped, IPv4 IHL, IPv6 fixed header */
static void set_offsets(odp_packet_t pkt)
{
	const uint8_t *d = odp_packet_data(pkt);
	const uint32_t len = odp_packet_len(pkt);
	uint32_t o = 12;

	if (len < 14)
		return;
	uint32_t et = (uint32_t)d[o] << 8 | d[o + 1];

	while ((et == 0x8100 || et == 0x88A8) && o + 6 <= len) {
		o += 4;
		et = (uint32_t)d[o] << 8 | d[o + 1];
	}
	const uint32_t l3 = o + 2;

	if (l3 >= len)
		return;
	odp_packet_l3_offset_set(pkt, l3);
	if (et == 0x0800 && l3 + 4u * (d[l3] & 15u) < len)
		odp_packet_l4_offset_set(pkt, l3 + 4u * (d[l3] & 15u));
	else if (et == 0x86DD && l3 + 40 < len)
		odp_packet_l4_offset_set(pkt, l3 + 40);
}

static int surface(const char *pcap, odp_pool_t pool)
{
	const char *names[2] = { "loop", NULL };
	char src[512];

	snprintf(src, sizeof(src), "pcap:in=%s", pcap);
	names[1] = src;
	for (int k = 0; k < 2; k++) {
		odp_pktio_param_t pp;
		odp_pktio_capability_t capa;
		odp_pktio_config_t cfg;
		const char *tag = k ? "pcap" : "loop";

		odp_pktio_param_init(&pp);
		odp_pktio_t io = odp_pktio_open(names[k], pool, &pp);

		if (io == ODP_PKTIO_INVALID || odp_pktio_capability(io, &capa))
			return 4;
		printf("CAP %s 0x%" PRIx64 "\n", tag, (uint64_t)capa.config.pktout.all_bits);
		/* the eight checksum bits, each default alone, and a bit past them */
		const uint64_t tries[] = { 0x1FE, 0x20, 0x40, 0x80, 0x100, 0x1E, 0x200, 0x01, 0x1FF };

		for (unsigned t = 0; t < sizeof(tries) / sizeof(tries[0]); t++) {
			odp_pktio_config_init(&cfg);
			cfg.pktout.all_bits = tries[t];
			printf("CFG %s 0x%" PRIx64 " %d\n", tag, tries[t], odp_pktio_config(io, &cfg));
		}
		odp_pktio_config_init(&cfg);
		if (odp_pktio_config(io, &cfg) || odp_pktio_close(io))
			return 5;
	}
	odp_packet_t pkt = odp_packet_alloc(pool, 64);

	if (pkt == ODP_PACKET_INVALID)
		return 6;
	odp_packet_l3_chksum_insert(pkt, 1);
	odp_packet_l4_chksum_insert(pkt, 0);
	odp_packet_free(pkt);
	printf("OVR ok\n");
	return 0;
}

int main(int argc, char *argv[])
{
	odp_instance_t inst;

	if (argc < 3) {
		fprintf(stderr, "usage: %s surface <pcap> | loop <pcap> <pktout> <pktin> <ovr>\n", argv[0]);
		return 2;
	}
	if (odp_init_global(&inst, NULL, NULL) || odp_init_local(inst, ODP_THREAD_CONTROL))
		return 3;
	odp_schedule_config(NULL);
	odp_pool_t pool = mkpool("pktio_pool");

	if (pool == ODP_POOL_INVALID)
		return 3;
	if (strcmp(argv[1], "surface") == 0)
		return surface(argv[2], pool);
	if (argc < 6)
		return 2;
	const uint64_t pktout = strtoull(argv[3], NULL, 0), pktin = strtoull(argv[4], NULL, 0);
	const int ovr = atoi(argv[5]);
	const int count_only = getenv("TX_COUNT_ONLY") != NULL;
	odp_pktio_param_t pp;
	odp_pktio_config_t cfg;
	odp_pktin_queue_param_t iq;
	odp_pktout_queue_param_t oq;

	odp_pktio_param_init(&pp);
	pp.in_mode = ODP_PKTIN_MODE_DIRECT;
	odp_pktio_t io = odp_pktio_open("loop", pool, &pp);

	if (io == ODP_PKTIO_INVALID)
		return 4;
	odp_pktin_queue_param_init(&iq);
	odp_pktout_queue_param_init(&oq);
	if (odp_pktin_queue_config(io, &iq) || odp_pktout_queue_config(io, &oq))
		return 5;
	odp_pktio_config_init(&cfg);
	cfg.parser.layer = ODP_PROTO_LAYER_ALL;
	cfg.pktin.all_bits = pktin;
	cfg.pktout.all_bits = pktout;
	if (odp_pktio_config(io, &cfg))
		return 6;
	if (odp_pktio_start(io))
		return 8;

	/* the source frames through a parse-less pcap pktio */
	char src[512];
	odp_pktio_param_t sp;
	odp_pktio_config_t sc;
	odp_pktin_queue_t sinq, inq;
	odp_pktout_queue_t outq;
	odp_packet_t pk[256];
	int n;
	long sent = 0;
	uint64_t send_ns = 0;

	snprintf(src, sizeof(src), "pcap:in=%s", argv[2]);
	odp_pktio_param_init(&sp);
	odp_pktio_t sio = odp_pktio_open(src, pool, &sp);

	if (sio == ODP_PKTIO_INVALID || odp_pktin_queue_config(sio, NULL))
		return 9;
	odp_pktio_promisc_mode_set(sio, 1);
	odp_pktio_config_init(&sc);
	sc.parser.layer = ODP_PROTO_LAYER_NONE;
	odp_pktio_config(sio, &sc);
	if (odp_pktio_start(sio) || odp_pktin_queue(sio, &sinq, 1) != 1 ||
	    odp_pktout_queue(io, &outq, 1) < 1 || odp_pktin_queue(io, &inq, 1) != 1)
		return 9;
	while ((n = odp_pktin_recv(sinq, pk, 256)) > 0) {
		for (int i = 0; i < n; i++) {
			set_offsets(pk[i]);
			if ((ovr == 1 && ((sent + i) & 1)) || ovr == 3)
				odp_packet_l4_chksum_insert(pk[i], 0);
			if (ovr == 2) {
				odp_packet_l3_chksum_insert(pk[i], 1);
				odp_packet_l4_chksum_insert(pk[i], 1);
			}
		}
		odp_time_t t0 = odp_time_local();

		if (odp_pktout_send(outq, pk, n) != n)
			return 10;
		send_ns += odp_time_diff_ns(odp_time_local(), t0);
		sent += n;
	}
	odp_pktio_stop(sio);
	odp_pktio_close(sio);

	int idle = 0;
	long got = 0;

	if (ovr == 3) {
		/* receive everything, send it again untouched */
		odp_packet_t *held = malloc(sizeof(*held) * (size_t)(sent + 1));
		long nh = 0;

		while (held && idle < 3) {
			n = odp_pktin_recv(inq, pk, 256);
			for (int i = 0; i < n && nh < sent; i++)
				held[nh++] = pk[i];
			idle = (n == 0 && odp_amd_pktio_rx_idle(io) == 1) ? idle + 1 : 0;
		}
		if (!held || nh != sent)
			return 12;
		for (long i = 0; i < nh; i += 256) {
			const int k = nh - i < 256 ? (int)(nh - i) : 256;

			if (odp_pktout_send(outq, held + i, k) != k)
				return 10;
		}
		free(held);
		idle = 0;
	}
	while (idle < 3) {
		n = odp_pktin_recv(inq, pk, 256);
		for (int i = 0; i < n; i++) {
			if (!count_only) {
				const uint8_t *d = odp_packet_data(pk[i]);
				const uint32_t len = odp_packet_len(pk[i]);

				printf("P %d %d %d ", (int)odp_packet_l3_chksum_status(pk[i]),
				       (int)odp_packet_l4_chksum_status(pk[i]), odp_packet_has_error(pk[i]));
				for (uint32_t b = 0; b < len; b++)
					printf("%02x", d[b]);
				printf("\n");
			}
			odp_packet_free(pk[i]);
		}
		got += n > 0 ? n : 0;
		idle = (n == 0 && odp_amd_pktio_rx_idle(io) == 1) ? idle + 1 : 0;
	}
	if (count_only)
		printf("R %ld %" PRIu64 "\n", got, send_ns);
	odp_pktio_stats_t st;

	odp_pktio_stats(io, &st);
	printf("S %" PRIu64 " %" PRIu64 "\n", st.in_packets, st.in_errors);
	uint64_t tx_bursts = 0, tx_bounced = 0;

	odp_amd_pktio_tx_stats(io, &tx_bursts, &tx_bounced);
	printf("T %" PRIu64 " %" PRIu64 "\n", tx_bursts, tx_bounced);
	odp_pktio_stop(io);
	odp_pktio_close(io);
	return sent == got ? 0 : 11;
}
