/*
 * ref_shim.h -- what the two shim units of oracle/_ref/libodp_ref.so share
 * (ref_shim.c: receive side and stand-ins; ref_loop_shim.c: transmit side).
 *
 *   *** TEST INFRASTRUCTURE -- NOT PART OF THE PRODUCT ***
 */
#ifndef REF_SHIM_H
#define REF_SHIM_H

#include <odp_api.h>
#include <odp_packet_internal.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

/* A call that the tested paths can never make ends the run: returning
 * something made up would hide a wrong shim. */
#define UNREACHED() do { fprintf(stderr, "ref_shim: %s called\n", __func__); abort(); } while (0)

#define TAIL_ZEROS 256   /* "bytes at or beyond frame_len read as zero" */

/* A packet header over a private copy of the frame followed by TAIL_ZEROS
 * zero bytes: one segment, no pool behind it.  free(*data) when done. */
odp_packet_hdr_t *ref_fake_packet(const uint8_t *frame, uint32_t len, uint8_t **data);

/* the 8-byte descriptor of include/mi_cls.h (mi_cls_tx_desc_t) */
typedef struct {
	uint16_t l3, l4;
	uint8_t  flags;
	uint8_t  rsv[3];
} ref_tx_desc_t;

#define REF_TX_NMOD 6   /* the moduli of ref_tx_dest_queue_batch */

int ref_tx_fix_checksums(const uint8_t *frame, uint32_t len, uint32_t l3, uint32_t l4, uint32_t flags,
			 uint32_t pktout_opt, uint8_t *out_frame);
int ref_tx_dest_queue(const uint8_t *frame, uint32_t len, uint32_t l3, uint32_t l4, uint32_t meta_flags,
		      uint32_t hash_proto, uint32_t num_qs, int index);
int ref_tx_fix_checksums_batch(const uint8_t *buf, const uint32_t *off, const uint16_t *len,
			       const ref_tx_desc_t *desc, uint32_t n, uint32_t pktout_opt, uint8_t *out_buf);
int ref_tx_dest_queue_batch(const uint8_t *buf, const uint32_t *off, const uint16_t *len,
			    const ref_tx_desc_t *desc, uint32_t n, uint32_t hash_proto, int index,
			    uint8_t *res);

#endif
