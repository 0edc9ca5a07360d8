/* pooltab_driver -- odp_amd_cls_pooltab_fill and odp_amd_cls_pool_own against a
 * control plane made through the public API: a loop pktio on its own pool, a
 * CoS without a pool, two CoS on one pool of their own, one on another, one on
 * the pktio's pool by name, a drop CoS with a pool; one more CoS on a new pool; then
 * a CoS on each of further pools until the table's 16 slots are full, and one more.
 * Needs no device.  Prints, for tests/test_pool_plan_cpu.py:
 *
 *   fill <rc> nslot <n> gen_ok <0|1> stamp_new <0|1>
 *   cos <name> <index> slot <s>                           per created CoS
 *   slot <k> <pool name> cap <slot_cap>                   per slot
 *   unused <count of slots at other CoS indexes>
 *   own <rc> <own of: a pktio-pool packet, a poolA packet, a poolB packet,
 *             a packet of a pool without a slot, ODP_PACKET_INVALID>
 *   regen <1 if the generation moved> nslot <n> late <slot> cap <slot_cap>
 *   full <rc of the fill with 16 pools> nslot <n>
 *   over <rc of the fill with 17 pools>
 *   bad <rc with a NULL table> <rc with NULL pools> <rc with no such pktio>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "odp_api.h"
#include "odp_cls_api.h"
#include "mi_cls.h"

static odp_pool_t pkt_pool(const char *name, uint32_t len)
{
	odp_pool_param_t p;

	odp_pool_param_init(&p);
	p.type = ODP_POOL_PACKET;
	p.pkt.num = 8;
	p.pkt.len = len;
	return odp_pool_create(name, &p);
}

static odp_cos_t mkcos(const char *name, int drop, odp_pool_t pool)
{
	odp_cls_cos_param_t cp;
	odp_queue_param_t qp;

	odp_cls_cos_param_init(&cp);
	odp_queue_param_init(&qp);
	qp.type = ODP_QUEUE_TYPE_SCHED;
	cp.action = drop ? ODP_COS_ACTION_DROP : ODP_COS_ACTION_ENQUEUE;
	cp.pool = pool;
	if (!drop)
		cp.queue = odp_queue_create(name, &qp);
	return odp_cls_cos_create(name, &cp);
}

static uint32_t cos_index(odp_cos_t c)
{
	return ((uint32_t)odp_cos_to_u64(c) - 1u) & 255u;   /* cos_t.index */
}

int main(void)
{
	odp_instance_t inst;
	static mi_cls_pool_tab_t tab, tab2;
	odp_pool_t pools[MI_CLS_POOL_SLOTS], pools2[MI_CLS_POOL_SLOTS];
	uint32_t ns = 99, ns2 = 0;
	uint64_t gen = 0, gen2 = 0;

	if (odp_init_global(&inst, NULL, NULL) || odp_init_local(inst, ODP_THREAD_CONTROL))
		return 3;
	odp_schedule_config(NULL);
	const odp_pool_t pio = pkt_pool("pio", 1500), pa = pkt_pool("poolA", 200), pb = pkt_pool("poolB", 9000),
			 pz = pkt_pool("poolZ", 300);

	if (pio == ODP_POOL_INVALID || pa == ODP_POOL_INVALID || pb == ODP_POOL_INVALID || pz == ODP_POOL_INVALID)
		return 4;
	const odp_pktio_t io = odp_pktio_open("loop", pio, NULL);

	if (io == ODP_PKTIO_INVALID)
		return 5;
	const char *names[] = { "plain", "a1", "b1", "a2", "named", "drop" };
	odp_cos_t cos[6];

	cos[0] = mkcos(names[0], 0, ODP_POOL_INVALID);
	cos[1] = mkcos(names[1], 0, pa);
	cos[2] = mkcos(names[2], 0, pb);
	cos[3] = mkcos(names[3], 0, pa);
	cos[4] = mkcos(names[4], 0, pio);
	cos[5] = mkcos(names[5], 1, pb);
	for (int i = 0; i < 6; i++)
		if (cos[i] == ODP_COS_INVALID)
			return 6;

	int rc = odp_amd_cls_pooltab_fill(io, &tab, pools, &ns, &gen);

	odp_amd_cls_pooltab_fill(io, &tab2, pools2, &ns2, &gen2);
	printf("fill %d nslot %u gen_ok %d stamp_new %d\n", rc, ns, gen == odp_amd_cls_generation() && gen2 == gen,
	       tab2.stamp != tab.stamp && tab.stamp != 0 && tab.nslot == ns);

	int used[256] = { 0 }, other = 0;

	for (int i = 0; i < 6; i++) {
		const uint32_t x = cos_index(cos[i]);

		used[x] = 1;
		printf("cos %s %u slot %u\n", names[i], x, tab.cos_slot[x]);
	}
	for (uint32_t k = 0; k < ns && k < MI_CLS_POOL_SLOTS; k++)
		printf("slot %u %s cap %u\n", k,
		       pools[k] == pio ? "pio" : pools[k] == pa ? "poolA" : pools[k] == pb ? "poolB" : "?", tab.slot_cap[k]);
	for (int i = 0; i < 256; i++)
		other += !used[i] && tab.cos_slot[i] != 0xFF;
	printf("unused %d\n", other);

	odp_packet_t pk[5] = { odp_packet_alloc(pio, 64), odp_packet_alloc(pa, 64), odp_packet_alloc(pb, 64),
			       odp_packet_alloc(pz, 64), ODP_PACKET_INVALID };
	uint8_t own[5] = { 9, 9, 9, 9, 9 };

	for (int i = 0; i < 4; i++)
		if (pk[i] == ODP_PACKET_INVALID)
			return 7;
	rc = odp_amd_cls_pool_own(pk, 5, pools, ns, own);
	printf("own %d %u %u %u %u %u\n", rc, own[0], own[1], own[2], own[3], own[4]);
	odp_packet_free_multi(pk, 4);

	/* the control plane changes: the generation moves and the next table follows */
	const odp_cos_t late = mkcos("late", 0, pz);

	if (late == ODP_COS_INVALID)
		return 8;
	rc = odp_amd_cls_pooltab_fill(io, &tab2, pools2, &ns2, &gen2);
	printf("regen %d nslot %u late %u cap %u\n", rc == 0 && gen2 != gen && gen2 == odp_amd_cls_generation(), ns2,
	       tab2.cos_slot[cos_index(late)], tab2.slot_cap[3]);

	/* a CoS on each of 12 more pools fills the slots; the 17th pool does not fit */
	for (int k = 0; k < 13; k++) {
		char nm[32];

		snprintf(nm, sizeof(nm), "poolX%d", k);
		const odp_pool_t p = pkt_pool(nm, 128);

		if (p == ODP_POOL_INVALID || mkcos(nm, 0, p) == ODP_COS_INVALID)
			return 9;
		if (k == 11) {
			rc = odp_amd_cls_pooltab_fill(io, &tab, pools, &ns, &gen);
			printf("full %d nslot %u\n", rc, ns);
		}
	}
	printf("over %d\n", odp_amd_cls_pooltab_fill(io, &tab, pools, &ns, &gen));
	printf("bad %d %d %d\n", odp_amd_cls_pooltab_fill(io, NULL, pools, &ns, &gen),
	       odp_amd_cls_pooltab_fill(io, &tab, NULL, &ns, &gen),
	       odp_amd_cls_pooltab_fill((odp_pktio_t)(uintptr_t)63, &tab, pools, &ns, &gen));
	return 0;
}
