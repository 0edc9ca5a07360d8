/* vecfill_driver -- the chain classify -> pool plan -> pool move -> run plan ->
 * vector take / fill / enqueue through the public API only, on the runtime's
 * own packets, vectors and queues, printed in rx_driver's format so that
 * tests/test_gpu_vecfill_driver.py can hold it equal to what the receive path
 * (rx_driver over the same capture and rules) delivers.  The control plane,
 * the pools and the printing are rx_driver's own code (included below); the
 * pktio is opened and started but never received from.
 *
 * usage: vecfill_driver <pcap:in=FILE> <rules> <frames file> <burst> <cos_pools 0|1>
 *   cos_pools 1 gives every CoS a pool of its own (at most 15 CoS then: the
 *   pool plan tells 16 pools apart).
 *   frames file: uint32 n, then per frame uint16 length and its bytes (the
 *   capture's frames, in order).  RX_PKTV as for rx_driver.
 * output: rx_driver's V / P / S / Q lines (S from the run plan's counters), and
 *   F <pool> <free> <num>      per pool after everything was freed
 *   C <vectors> <lost> <holes> <refused> <events>   the fill's counters
 */
#define main rx_driver_main
#include "rx_driver.c"
#undef main

#include <errno.h>

#include "odp_cls_api.h"
#include "mi_cls.h"

#define DIE(code, ...)                                  \
	do {                                            \
		fprintf(stderr, __VA_ARGS__);           \
		fprintf(stderr, "\n");                  \
		return code;                            \
	} while (0)

static void *zalloc(size_t bytes)
{
	void *p = aligned_alloc(64, (bytes + 63) & ~(size_t)63);

	if (p)
		memset(p, 0, (bytes + 63) & ~(size_t)63);
	return p;
}

/* the events a pool can still give: taken and put back */
static uint32_t pool_free_count(odp_pool_t pool, uint32_t num, int vectors)
{
	void **h = malloc(sizeof(void *) * (num + 1));
	uint32_t n = 0;

	if (!h)
		return 0;
	if (vectors) {
		while (n <= num && (h[n] = (void *)odp_packet_vector_alloc(pool)) != (void *)ODP_PACKET_VECTOR_INVALID)
			n++;
		for (uint32_t i = 0; i < n; i++)
			odp_packet_vector_free((odp_packet_vector_t)h[i]);
	} else {
		const int k = odp_packet_alloc_multi(pool, 64, (odp_packet_t *)h, (int)num + 1);

		n = k > 0 ? (uint32_t)k : 0;
		if (n)
			odp_packet_free_multi((odp_packet_t *)h, (int)n);
	}
	free(h);
	return n;
}

int main(int argc, char *argv[])
{
	odp_instance_t inst;
	odp_pktio_param_t pp;
	odp_pktin_queue_param_t iq;
	odp_pktout_queue_param_t oq;
	odp_pktio_config_t cfg;

	if (argc < 6)
		DIE(2, "usage: %s <pcap:in=FILE> <rules> <frames file> <burst> <cos_pools>", argv[0]);
	const uint32_t burst = (uint32_t)atoi(argv[4]);

	if (odp_init_global(&inst, NULL, NULL) || odp_init_local(inst, ODP_THREAD_CONTROL))
		return 3;
	odp_schedule_config(NULL);
	odp_pool_t pool = mkpool("pktio_pool");
	uint32_t pktv_num = 0;

	if (getenv("RX_PKTV")) {
		odp_pool_param_t vp;
		unsigned mx = 0, num = 0;

		sscanf(getenv("RX_PKTV"), "%u,%u", &mx, &num);
		odp_pool_param_init(&vp);
		vp.type = ODP_POOL_VECTOR;
		vp.vector.num = num;
		vp.vector.max_size = mx;
		pktv_pool = odp_pool_create("pktv_pool", &vp);
		pktv_max = mx;
		pktv_num = num;
		if (pktv_pool == ODP_POOL_INVALID)
			return 12;
	}
	odp_pktio_param_init(&pp);
	pp.in_mode = ODP_PKTIN_MODE_DIRECT;
	odp_pktio_t pktio = odp_pktio_open(argv[1], pool, &pp);

	if (pktio == ODP_PKTIO_INVALID)
		return 4;
	odp_pktin_queue_param_init(&iq);
	iq.classifier_enable = 1;
	odp_pktout_queue_param_init(&oq);
	if (odp_pktin_queue_config(pktio, &iq) || odp_pktout_queue_config(pktio, &oq))
		return 5;
	odp_pktio_promisc_mode_set(pktio, 1);
	odp_pktio_config_init(&cfg);
	cfg.parser.layer = ODP_PROTO_LAYER_ALL;
	if (odp_pktio_config(pktio, &cfg))
		return 6;
	FILE *f = fopen(argv[2], "r");

	if (!f)
		return 7;
	replay(f, pktio, atoi(argv[5]));
	fclose(f);
	if (odp_pktio_start(pktio))
		return 8;

	/* ---- the frames ---------------------------------------------------- */
	uint32_t n = 0;
	size_t bytes = 0;

	f = fopen(argv[3], "rb");
	if (!f || fread(&n, 4, 1, f) != 1 || n == 0)
		DIE(9, "no frames");
	uint8_t *pkts = zalloc((size_t)n * 2048 + 64);
	uint32_t *off = zalloc(4 * (size_t)n);
	uint16_t *len = zalloc(2 * (size_t)n);

	for (uint32_t i = 0; i < n; i++) {
		if (fread(&len[i], 2, 1, f) != 1 || len[i] > 1856 || fread(pkts + bytes, 1, len[i], f) != len[i])
			DIE(9, "bad frames file at %u", i);
		off[i] = (uint32_t)bytes;
		bytes += len[i];
	}
	fclose(f);

	/* ---- classify -------------------------------------------------------- */
	mi_cls_result_t *res = zalloc(sizeof(*res) * n), *res2 = zalloc(sizeof(*res) * n);
	int rc = odp_amd_cls_classify_host(pktio, pkts, bytes, off, len, n, res, 0);

	if (rc)
		DIE(20, "classify: %d", rc);

	/* ---- the three tables ------------------------------------------------ */
	static mi_cls_enq_tab_t etab;
	static mi_cls_pool_tab_t ptab;
	static mi_cls_run_tab_t rtab;
	static odp_queue_t queues[MI_CLS_ENQ_DST_MAX];
	odp_pool_t pools[MI_CLS_POOL_SLOTS], vpools[MI_CLS_RUN_VSLOTS];
	uint32_t ndst = 0, npool = 0, nvp = 0;
	uint64_t gen = 0;

	if ((rc = odp_amd_cls_enqtab_fill(&etab, queues, &ndst, &gen)) ||
	    (rc = odp_amd_cls_pooltab_fill(pktio, &ptab, pools, &npool, &gen)) ||
	    (rc = odp_amd_cls_runtab_fill(&rtab, vpools, &nvp, &gen)))
		DIE(21, "tables: %d", rc);

	/* ---- pool plan: the need first, then with the packets at hand -------- */
	uint32_t have[MI_CLS_POOL_SLOTS], base[MI_CLS_POOL_SLOTS] = { 0 };
	uint32_t *dec = zalloc(4 * (size_t)n), *idx = zalloc(4 * (size_t)n);
	static mi_cls_pool_out_t pout;

	for (uint32_t k = 0; k < MI_CLS_POOL_SLOTS; k++)
		have[k] = 0xFFFFFFFFu;
	rc = odp_amd_cls_pool_plan_host(pktio, res, len, NULL, n, &ptab, have, base, res2, dec, idx, &pout);
	if (rc)
		DIE(22, "pool plan (need): %d", rc);
	uint32_t ngot = 0, meta_off = 0, dfm = 0;
	uint64_t alo = 0, abytes = 0;

	if ((rc = odp_amd_cls_pool_move_geom(&meta_off, &dfm, &alo, &abytes)))
		DIE(23, "pool move geom: %d (pools not page-locked?)", rc);
	uint64_t *got = zalloc(8 * ((size_t)n + 1));
	uint32_t headroom = 0;

	for (uint32_t k = 0; k < MI_CLS_POOL_SLOTS; k++) {
		base[k] = ngot;
		have[k] = 0;
		if (k >= npool || pout.need[k] == 0)
			continue;
		const int t = odp_packet_alloc_multi(pools[k], 64, (odp_packet_t *)(void *)(got + ngot), (int)pout.need[k]);

		have[k] = t > 0 ? (uint32_t)t : 0;
		if (have[k])
			headroom = odp_packet_headroom((odp_packet_t)(uintptr_t)got[ngot]);
		for (uint32_t i = 0; i < have[k]; i++)
			got[ngot + i] += meta_off;      /* the line's address */
		ngot += have[k];
	}
	rc = odp_amd_cls_pool_plan_host(pktio, res, len, NULL, n, &ptab, have, base, res2, dec, idx, &pout);
	if (rc)
		DIE(22, "pool plan: %d", rc);

	/* ---- pool move ------------------------------------------------------- */
	uint64_t *ent = zalloc(8 * (size_t)n);
	static mi_cls_move_out_t mout;
	mi_cls_move_args_t ma;

	memset(&ma, 0, sizeof(ma));
	ma.pkts = pkts;
	ma.pkts_bytes = bytes;
	ma.off = off;
	ma.len = len;
	ma.res = res2;
	ma.dec = dec;
	ma.idx = idx;
	ma.got = got;
	ma.n = n;
	ma.ngot = ngot;
	ma.tab = &etab;
	ma.dst_queue = (const uint64_t *)(const void *)queues;
	ma.input = (uint64_t)(uintptr_t)pktio;
	ma.headroom = headroom;
	ma.data_from_meta = dfm;
	ma.arena_lo = alo;
	ma.arena_bytes = abytes;
	ma.ent = ent;
	ma.out = &mout;
	if ((rc = odp_amd_cls_pool_move_host(pktio, &ma)) || mout.refused)
		DIE(24, "pool move: %d refused %llu", rc, (unsigned long long)mout.refused);

	/* ---- run plan -------------------------------------------------------- */
	uint32_t *seq = zalloc(4 * (size_t)n);
	mi_cls_run_t *runs = zalloc(sizeof(*runs) * n);
	static mi_cls_run_out_t rout;

	rc = odp_amd_cls_enq_runs_host(pktio, res2, len, n, &etab, &rtab, burst, seq, runs, n, &rout);
	if (rc || rout.nruns > n)
		DIE(25, "run plan: %d", rc);

	/* ---- vectors: take, fill, enqueue ------------------------------------ */
	mi_cls_vec_args_t va;
	static mi_cls_vec_out_t vout;
	uint64_t *vgot = zalloc(8 * ((size_t)rout.vectors + 1));
	uint64_t *ev = zalloc(8 * (size_t)n), *lost = zalloc(8 * (size_t)n);
	mi_cls_evrun_t *evr = zalloc(sizeof(*evr) * n);
	uint64_t vlo = 0, vbytes = 0;

	memset(&va, 0, sizeof(va));
	if ((rc = odp_amd_cls_vec_geom(&va.size_off, &va.tbl_off, &vlo, &vbytes)) && rout.vectors)
		DIE(26, "vec geom: %d (vector pools not page-locked?)", rc);
	const int nvgot = odp_amd_cls_vec_take(vpools, nvp, rout.vec_need, vgot, (uint32_t)rout.vectors, va.vbase,
					       va.vhave, va.vcap);

	if (nvgot < 0)
		DIE(27, "vec take: %d", nvgot);
	va.seq = seq;
	va.runs = runs;
	va.run_out = &rout;
	va.ent = ent;
	va.vgot = vgot;
	va.n = n;
	va.run_cap = n;
	va.nvgot = (uint32_t)nvgot;
	va.ent_to_handle = meta_off;
	va.rtab = &rtab;
	va.varena_lo = vlo;
	va.varena_bytes = vbytes;
	va.ev = ev;
	va.evr = evr;
	va.lost = lost;
	va.out = &vout;
	if (vbytes == 0) {   /* no vector pool at all: any range the device reaches, never written */
		va.varena_lo = alo;
		va.varena_bytes = abytes;
	}
	if ((rc = odp_amd_cls_vec_fill_host(pktio, &va)) || vout.truncated)
		DIE(28, "vec fill: %d", rc);
	const int64_t events = odp_amd_cls_vec_enq(runs, evr, (uint32_t)rout.nruns, ev, lost, (uint32_t)vout.lost, queues,
						   ndst, &rtab, vpools, nvp, vgot, va.vbase, va.vhave, &vout, seq,
						   ent, meta_off);

	if (events < 0)
		DIE(29, "vec enq: %lld", (long long)events);
	/* the records that are not delivered, and the packets taken and not used */
	for (uint32_t p = (uint32_t)rout.delivered; p < n; p++)
		if (ent[seq[p]])
			odp_packet_free((odp_packet_t)(uintptr_t)(ent[seq[p]] - meta_off));
	for (uint32_t k = 0; k < npool; k++)
		for (uint32_t i = base[k] + pout.used[k]; i < base[k] + have[k]; i++)
			odp_packet_free((odp_packet_t)(uintptr_t)(got[i] - meta_off));

	/* ---- what the queues hold -------------------------------------------- */
	for (;;) {
		odp_event_t e[64];
		odp_queue_t from;
		const int m = odp_schedule_multi(&from, ODP_SCHED_NO_WAIT, e, 64);

		if (m <= 0)
			break;
		for (int i = 0; i < m; i++)
			print_ev(qname(from), e[i]);
	}
	printf("S %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rout.packets, rout.in_errors, rout.in_discards,
	       rout.octets);
	for (int c = 0; c < ncos; c++) {
		odp_queue_t qs[32];
		uint32_t nq = odp_cls_cos_queues(cos_h[c], qs, 32);

		for (uint32_t s = 0; s < nq && s < 32; s++) {
			odp_cls_queue_stats_t qs_;

			if (odp_cls_queue_stats(cos_h[c], qs[s], &qs_) == 0)
				printf("Q %s %u %" PRIu64 " %" PRIu64 "\n", cos_name[c], s, qs_.packets, qs_.discards);
		}
	}
	printf("C %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRId64 "\n", vout.vectors, vout.lost, vout.holes,
	       vout.refused, events);
	for (uint32_t k = 0; k < npool; k++) {
		odp_pool_info_t info;

		if (odp_pool_info(pools[k], &info) == 0)
			printf("F %s %u %u\n", info.name, pool_free_count(pools[k], info.params.pkt.num, 0),
			       info.params.pkt.num);
	}
	if (pktv_pool != ODP_POOL_INVALID)
		printf("F pktv_pool %u %u\n", pool_free_count(pktv_pool, pktv_num, 1), pktv_num);
	odp_pktio_stop(pktio);
	odp_pktio_close(pktio);
	return 0;
}
