/* runtab_driver -- odp_amd_cls_runtab_fill against a control plane made through
 * the public API: a plain CoS, two packet-vector CoS on one vector pool, one on
 * another, a hash CoS whose queues have event aggregators, a drop CoS; then a
 * vector CoS on each of further pools until the table's 16 slots are full, and
 * one more.  Needs no device.  Prints, for tests/test_enq_runs_cpu.py:
 *
 *   fill <rc> nslots <n> gen_ok <0|1> stamp_new <0|1>
 *   cos <name> <index> mode <m> vmax <v> vslot <s>      per created CoS
 *   slot <k> <pool name>                                  per slot
 *   unused_modes <count of nonzero modes at other indexes>
 *   full <rc of the fill with 16 pools> nslots <n>
 *   over <rc of the fill with 17 pools>
 *   bad <rc with a NULL table> <rc with NULL pools>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "odp_api.h"
#include "odp_cls_api.h"
#include "mi_cls.h"

static odp_pool_t vec_pool(const char *name, uint32_t max_size)
{
	odp_pool_param_t p;

	odp_pool_param_init(&p);
	p.type = ODP_POOL_VECTOR;
	p.vector.num = 16;
	p.vector.max_size = max_size;
	return odp_pool_create(name, &p);
}

static odp_cos_t mkcos(const char *name, int drop, uint32_t nq, odp_pool_t vpool, uint32_t vmax,
		       const odp_event_aggr_config_t *aggr)
{
	odp_cls_cos_param_t cp;
	odp_queue_param_t qp;

	odp_cls_cos_param_init(&cp);
	odp_queue_param_init(&qp);
	qp.type = ODP_QUEUE_TYPE_SCHED;
	cp.action = drop ? ODP_COS_ACTION_DROP : ODP_COS_ACTION_ENQUEUE;
	cp.num_queue = nq;
	if (vpool != ODP_POOL_INVALID) {
		cp.vector.enable = true;
		cp.vector.pool = vpool;
		cp.vector.max_size = vmax;
	}
	if (nq > 1) {
		if (aggr) {
			qp.num_aggr = 1;
			qp.aggr = aggr;
		}
		cp.queue_param = qp;
		cp.hash_proto.all_bits = 0x5;
	} else if (!drop) {
		cp.queue = odp_queue_create(name, &qp);
	}
	return odp_cls_cos_create(name, &cp);
}

int main(void)
{
	odp_instance_t inst;
	static mi_cls_run_tab_t tab, tab2;
	odp_pool_t vp[MI_CLS_RUN_VSLOTS];
	uint32_t ns = 99;
	uint64_t gen = 0;

	if (odp_init_global(&inst, NULL, NULL) || odp_init_local(inst, ODP_THREAD_CONTROL))
		return 3;
	odp_schedule_config(NULL);
	const odp_pool_t pa = vec_pool("vpoolA", 64), pb = vec_pool("vpoolB", 64);
	odp_pool_param_t ep;
	odp_event_aggr_config_t aggr;

	odp_pool_param_init(&ep);
	ep.type = ODP_POOL_EVENT_VECTOR;
	ep.event_vector.num = 16;
	ep.event_vector.max_size = 8;
	const odp_pool_t evv = odp_pool_create("evv_pool", &ep);

	if (pa == ODP_POOL_INVALID || pb == ODP_POOL_INVALID || evv == ODP_POOL_INVALID)
		return 4;
	memset(&aggr, 0, sizeof(aggr));
	aggr.pool = evv;
	aggr.max_size = 8;
	aggr.max_tmo_ns = 1000;
	aggr.event_type = ODP_EVENT_PACKET;

	const char *names[] = { "plain", "vecA", "aggr", "vecA2", "vecB", "drop" };
	odp_cos_t cos[6];

	cos[0] = mkcos(names[0], 0, 1, ODP_POOL_INVALID, 0, NULL);
	cos[1] = mkcos(names[1], 0, 1, pa, 8, NULL);
	cos[2] = mkcos(names[2], 0, 4, ODP_POOL_INVALID, 0, &aggr);
	cos[3] = mkcos(names[3], 0, 1, pa, 3, NULL);
	cos[4] = mkcos(names[4], 0, 4, pb, 64, NULL);
	cos[5] = mkcos(names[5], 1, 1, ODP_POOL_INVALID, 0, NULL);
	for (int i = 0; i < 6; i++)
		if (cos[i] == ODP_COS_INVALID)
			return 5;

	int rc = odp_amd_cls_runtab_fill(&tab, vp, &ns, &gen);
	uint32_t ns2 = 0;
	uint64_t gen2 = 0;
	odp_pool_t vp2[MI_CLS_RUN_VSLOTS];

	odp_amd_cls_runtab_fill(&tab2, vp2, &ns2, &gen2);
	printf("fill %d nslots %u gen_ok %d stamp_new %d\n", rc, ns, gen == odp_amd_cls_generation() && gen2 == gen,
	       tab2.stamp != tab.stamp && tab.stamp != 0);

	int used[256] = { 0 }, other = 0;

	for (int i = 0; i < 6; i++) {
		const uint32_t x = (uint32_t)odp_cos_to_u64(cos[i]) - 1u;   /* cos_t.index */

		used[x & 255u] = 1;
		printf("cos %s %u mode %u vmax %u vslot %u\n", names[i], x, tab.mode[x], tab.vmax[x], tab.vslot[x]);
	}
	for (uint32_t k = 0; k < ns && k < MI_CLS_RUN_VSLOTS; k++)
		printf("slot %u %s\n", k, vp[k] == pa ? "vpoolA" : vp[k] == pb ? "vpoolB" : "?");
	for (int i = 0; i < 256; i++)
		other += !used[i] && (tab.mode[i] || tab.vmax[i] || tab.vslot[i]);
	printf("unused_modes %d\n", other);

	/* a CoS on each of 14 more pools fills the slots; the 17th pool does not fit */
	for (int k = 0; k < 15; k++) {
		char nm[32];

		snprintf(nm, sizeof(nm), "vpoolX%d", k);
		const odp_pool_t p = vec_pool(nm, 4);

		if (p == ODP_POOL_INVALID || mkcos(nm, 0, 1, p, 4, NULL) == ODP_COS_INVALID)
			return 6;
		if (k == 13) {
			rc = odp_amd_cls_runtab_fill(&tab, vp, &ns, &gen);
			printf("full %d nslots %u\n", rc, ns);
		}
	}
	printf("over %d\n", odp_amd_cls_runtab_fill(&tab, vp, &ns, &gen));
	printf("bad %d %d\n", odp_amd_cls_runtab_fill(NULL, vp, &ns, &gen),
	       odp_amd_cls_runtab_fill(&tab, NULL, &ns, &gen));
	return 0;
}
