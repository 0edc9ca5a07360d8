/*
 * ref_loop_shim.c -- runs the reference's OWN transmit code of the loop pktio
 * behind a C ABI: loopback_fix_checksums / check_proto (the decision and the
 * calls of odp_packet.c's _odp_packet_{ipv4,udp,tcp,sctp}_chksum_insert) and
 * get_dest_queue (the pktin flow hash).  Those functions are `static` in
 * pktio/loop.c, so this unit includes that file from the reference tree when
 * it is compiled (oracle/Makefile; the include below is all of it that is
 * here).  The copy of the rest of loop.c that comes with it (open, send,
 * receive, the ops table) is never called; the symbols it leaves undefined
 * get stand-ins that end the run.
 *
 *   *** TEST INFRASTRUCTURE -- NOT PART OF THE PRODUCT ***
 *
 * This file is this project's text.
 */
#include <pktio/loop.c>

#include "ref_shim.h"

#include <odp/api/plat/event_vector_inline_types.h>

#include <string.h>

/* the descriptor's bits (include/mi_cls.h MI_CLS_TXF_*) */
#define F_L3_SET 0x01u
#define F_L3 0x02u
#define F_L4_SET 0x04u
#define F_L4 0x08u
#define F_UDP 0x10u
#define F_TCP 0x20u
#define F_IPV4 0x40u
#define F_IPV6 0x80u

_Static_assert(sizeof(ref_tx_desc_t) == 8, "descriptor is 8 bytes");
_Static_assert(MAX_QUEUES >= 64, "the six moduli need 64 loop queues");

/* ============================================================ stand-ins */
/* What the rest of loop.c refers to.  Nothing that ref_tx_* calls reaches
 * any of it. */
const _odp_queue_api_fn_t *_odp_queue_api;
odp_global_data_ro_t odp_global_ro;
const _odp_event_vector_inline_offset_t _odp_event_vector_inline;

int _odp_ipsec_try_inline(odp_packet_t *pkt)
{
	(void)pkt;
	UNREACHED();
}

odp_time_t _odp_time_cur(void)
{
	UNREACHED();
}

int odp_queue_capability(odp_queue_capability_t *capa)
{
	(void)capa;
	UNREACHED();
}

odp_queue_t odp_queue_aggr(odp_queue_t queue, uint32_t aggr_index)
{
	(void)queue;
	(void)aggr_index;
	UNREACHED();
}

void odp_pktio_config_init(odp_pktio_config_t *config)
{
	(void)config;
	UNREACHED();
}

odp_packet_vector_t odp_packet_vector_alloc(odp_pool_t pool)
{
	(void)pool;
	UNREACHED();
}

void odp_event_free(odp_event_t event)
{
	(void)event;
	UNREACHED();
}

void odp_event_free_multi(const odp_event_t event[], int num)
{
	(void)event;
	(void)num;
	UNREACHED();
}

/* ============================================================== ref_tx_* */
static void set_offsets(odp_packet_hdr_t *hdr, uint32_t l3, uint32_t l4)
{
	hdr->p.l3_offset = l3 == 0xFFFF ? ODP_PACKET_OFFSET_INVALID : l3;
	hdr->p.l4_offset = l4 == 0xFFFF ? ODP_PACKET_OFFSET_INVALID : l4;
}

/* loopback_fix_checksums on the fake packet: the offsets and the four
 * override flags from the descriptor, pktout_cfg.all_bits = pktout_opt, every
 * capability bit set.  out_frame receives the len bytes of the frame as the
 * reference leaves them.  0 done, -1 no memory. */
int ref_tx_fix_checksums(const uint8_t *frame, uint32_t len, uint32_t l3, uint32_t l4, uint32_t flags,
			 uint32_t pktout_opt, uint8_t *out_frame)
{
	odp_pktout_config_opt_t cfg, capa;
	uint8_t *data;
	odp_packet_hdr_t *hdr = ref_fake_packet(frame, len, &data);

	if (!hdr)
		return -1;
	set_offsets(hdr, l3, l4);
	hdr->p.flags.l3_chksum_set = (flags & F_L3_SET) != 0;
	hdr->p.flags.l3_chksum = (flags & F_L3) != 0;
	hdr->p.flags.l4_chksum_set = (flags & F_L4_SET) != 0;
	hdr->p.flags.l4_chksum = (flags & F_L4) != 0;
	cfg.all_bits = pktout_opt;
	capa.all_bits = 0;
	capa.bit.ipv4_chksum = capa.bit.udp_chksum = capa.bit.tcp_chksum = capa.bit.sctp_chksum = 1;
	capa.bit.ipv4_chksum_ena = capa.bit.udp_chksum_ena = capa.bit.tcp_chksum_ena = 1;
	capa.bit.sctp_chksum_ena = 1;
	loopback_fix_checksums(packet_handle(hdr), &cfg, &capa);
	memcpy(out_frame, data, len);
	free(data);
	return 0;
}

/* get_dest_queue on the fake packet, over a pkt_loop_t whose queue i is the
 * handle i + 1: returns the index of the queue it picked, -1 no memory. */
int ref_tx_dest_queue(const uint8_t *frame, uint32_t len, uint32_t l3, uint32_t l4, uint32_t meta_flags,
		      uint32_t hash_proto, uint32_t num_qs, int index)
{
	static pkt_loop_t loop;
	uint8_t *data;
	odp_packet_hdr_t *hdr;
	odp_queue_t q;
	uint32_t i;

	if (num_qs == 0 || num_qs > MAX_QUEUES)
		return -2;
	hdr = ref_fake_packet(frame, len, &data);
	if (!hdr)
		return -1;
	set_offsets(hdr, l3, l4);
	hdr->p.input_flags.udp = (meta_flags & F_UDP) != 0;
	hdr->p.input_flags.tcp = (meta_flags & F_TCP) != 0;
	hdr->p.input_flags.ipv4 = (meta_flags & F_IPV4) != 0;
	hdr->p.input_flags.ipv6 = (meta_flags & F_IPV6) != 0;
	for (i = 0; i < MAX_QUEUES; i++)
		loop.loopqs[i].queue = (odp_queue_t)(uintptr_t)(i + 1);
	loop.hash.all_bits = hash_proto;
	loop.num_qs = num_qs;
	loop.num_conf_qs = num_qs;
	q = get_dest_queue(&loop, packet_handle(hdr), index);
	free(data);
	return (int)((uintptr_t)q - 1);
}

/* ------------------------------------------------- the same over a batch */
int ref_tx_fix_checksums_batch(const uint8_t *buf, const uint32_t *off, const uint16_t *len,
			       const ref_tx_desc_t *desc, uint32_t n, uint32_t pktout_opt, uint8_t *out_buf)
{
	uint32_t i;

	for (i = 0; i < n; i++)
		if (ref_tx_fix_checksums(buf + off[i], len[i], desc[i].l3, desc[i].l4, desc[i].flags,
					 pktout_opt, out_buf + off[i]))
			return -1;
	return 0;
}

/* res[6 i + k]: the queue of packet i with num_qs = the k-th of these six
 * pairwise coprime moduli, none above the loop pktio's 64 queues, whose
 * product exceeds 2^32 */
static const uint32_t tx_mod[REF_TX_NMOD] = { 64, 63, 61, 59, 55, 53 };

int ref_tx_dest_queue_batch(const uint8_t *buf, const uint32_t *off, const uint16_t *len,
			    const ref_tx_desc_t *desc, uint32_t n, uint32_t hash_proto, int index,
			    uint8_t *res)
{
	uint32_t i, k;

	for (i = 0; i < n; i++)
		for (k = 0; k < REF_TX_NMOD; k++) {
			int q = ref_tx_dest_queue(buf + off[i], len[i], desc[i].l3, desc[i].l4, desc[i].flags,
						  hash_proto, tx_mod[k], index);

			if (q < 0)
				return q;
			res[REF_TX_NMOD * i + k] = (uint8_t)q;
		}
	return 0;
}
