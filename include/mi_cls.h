/*
 * mi_cls.h -- thin C ABI between the (C) ODP host side and the hand-written
 * gfx950 HIP kernels of the MI355X packet parse + PMR classify path.
 *
 * This ABI is the device-side, batch form of the two per-packet internal
 * calls that every linux-generic pktio driver's .recv op makes
 * (pktio_if_ops_t.recv, platform/linux-generic/include/odp_packet_io_internal.h:222;
 * loop driver: platform/linux-generic/pktio/loop.c:253-384):
 *
 *   _odp_packet_parse_common()   platform/linux-generic/include/odp_parse_internal.h:80-112
 *   _odp_cls_classify_packet()   platform/linux-generic/odp_classification.c:1742-1771
 *
 * One call of mi_cls_classify() replaces the per-packet pair for a whole
 * batch of contiguous packets already resident in device memory.  All
 * pointers are plain device pointers; the caller owns every buffer.  Every
 * entry point returns 0 on success or a negative errno.
 *
 * Threading: one mi_cls_ctx_t per GPU; calls on one context are
 * serialised by the caller (mirrors the reference's lock-free data plane
 * reading rule tables that the control plane snapshots, odp_classification.c:1373).
 */
#ifndef MI_CLS_H_
#define MI_CLS_H_

#ifndef __HIPCC_RTC__
#include <stddef.h>
#endif
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Per-packet result record (16 bytes, written by the kernel).
 * Mirrors the packet-header fields the reference fills in
 * (odp_packet_hdr_t.p / .cos / .dst_queue / .cls_mark,
 *  platform/linux-generic/include/odp_packet_internal.h:55-70,112,116,139):
 *   in_flags  - low 32 bits of packet_parser_t.input_flags.all (bits >= 32
 *               are never set by this path; layout: packet_inline_types.h:60-107)
 *   err       - flags.all.error, 7 bits: snap_len, ip, l3_chksum, tcp, udp,
 *               sctp, l4_chksum (packet_inline_types.h:152-165)
 *   outcome   - MI_CLS_OUT_* below (the 0 / 1 / -1 return protocol of
 *               _odp_packet_parse_common and _odp_cls_classify_packet)
 *   cos       - CoS index (cos_t.index, the slot number), 0xFF when none
 *   hops      - number of PMR matches on the CoS descent (diagnostic)
 *   queue     - queue slot inside the CoS: 0 for a single-queue CoS, the
 *               Toeplitz hash slot for a hash-queue CoS (get_dest_queue,
 *               odp_classification.c:395-405); the host maps (cos, slot) to
 *               the odp_queue_t handle
 *   mark      - hdr->cls_mark (valid when in_flags bit 0, cls_mark, is set)
 *   l3/l4     - packet_parser_t.l3_offset / l4_offset (0xFFFF = invalid);
 *               l2_offset is always 0 on this path and is not stored.
 * ---------------------------------------------------------------------- */
typedef struct mi_cls_result {
	uint32_t in_flags;
	uint8_t  err;
	uint8_t  outcome;
	uint8_t  cos;
	uint8_t  hops;
	uint16_t queue;
	uint16_t mark;
	uint16_t l3_offset;
	uint16_t l4_offset;
} mi_cls_result_t;

enum {
	MI_CLS_OUT_ENQ        = 0, /* classify returned 0: enqueue to (cos, queue)        */
	MI_CLS_OUT_COS_DROP   = 1, /* classify returned 1: CoS action DROP (silent drop)   */
	MI_CLS_OUT_DISCARD    = 2, /* classify returned -1: no CoS (in_discards++)         */
	MI_CLS_OUT_PARSE_DROP = 3, /* parse returned -1: truncated L4 header (in_errors++) */
	MI_CLS_OUT_LOOP       = 4  /* CoS graph cycle: the reference never returns here    */
};

/* ------------------------------------------------------------------------
 * Compiled rule table ("snapshot" of the control-plane CoS/PMR tables,
 * platform/linux-generic/include/odp_classification_datamodel.h:126-206).
 * One contiguous, position-independent little-endian blob of 32-bit words:
 *   mi_tbl_hdr_t | mi_cos_t[num_cos] | mi_rule_t[num_rules] | mi_term_t[num_terms]
 * Rules of a CoS are stored contiguously in cos->pmr[] order (the order the
 * reference scans them, match_pmr_cos, odp_classification.c:1631), with
 * entries whose linked CoS is invalid already removed (:1635-1636).
 * ---------------------------------------------------------------------- */
#define MI_CLS_TBL_MAGIC   0x534C434Du /* "MCLS" */
#define MI_CLS_TBL_VERSION 1u

typedef struct mi_tbl_hdr {
	uint32_t magic;
	uint32_t version;
	uint32_t total_bytes;
	uint32_t num_cos;       /* CoS slots described (= max slot used + 1)          */
	uint32_t num_rules;
	uint32_t num_terms;
	int32_t  default_cos;   /* slot, -1 = none (classifier_t.default_cos)         */
	int32_t  error_cos;     /* slot, -1 = none (classifier_t.error_cos)           */
	uint32_t default_valid; /* default_cos->valid at snapshot time (:1712)        */
	uint32_t used_kinds;    /* bit per MI_K_* present anywhere in the table       */
	uint32_t max_hops;      /* descent bound (cycle guard)                        */
	uint32_t cos_off;       /* byte offsets of the three arrays from the header   */
	uint32_t rule_off;
	uint32_t term_off;
	uint32_t generation;    /* control-plane generation this snapshot reflects    */
	uint32_t rsv;
} mi_tbl_hdr_t;

typedef struct mi_cos {
	uint32_t rule_begin;
	uint32_t num_rules;
	uint8_t  action;        /* 0 enqueue, 1 drop (odp_cos_action_t)              */
	uint8_t  num_queue;     /* 1..32                                             */
	uint8_t  hash_proto;    /* cos_t.hash_proto: bit0 ipv4, 1 ipv6, 2 udp, 3 tcp */
	uint8_t  index;         /* cos_t.index                                       */
	uint32_t valid;
} mi_cos_t;

typedef struct mi_rule {
	uint32_t term_begin;
	uint16_t num_terms;     /* 0..8; 0 matches everything                       */
	uint16_t mark;
	uint32_t dst_cos;       /* linked CoS slot                                  */
	uint32_t rsv;
} mi_rule_t;

/* Compiled term kinds (one per verify_pmr_<term>, odp_classification.c:931-1357) */
enum {
	MI_K_LEN = 0,      /* frame_len (host order) & mask == value                 */
	MI_K_ETH0,         /* raw bytes at l2+12, gate eth                           */
	MI_K_ETHX,         /* raw bytes at l2+16 / +20 (qinq), gate vlan|qinq        */
	MI_K_VID0,         /* raw tci at l2+14 & be16(0x0fff), gate eth&vlan         */
	MI_K_VIDX,         /* raw tci at l2+14 / +18, & be16(0x0fff), gate vlan|qinq */
	MI_K_PCP0,         /* tci>>13 (host order), gate eth&vlan                    */
	MI_K_DMAC,         /* 6 raw bytes at l2, gate eth                            */
	MI_K_PROTO,        /* ipv4 proto / ipv6 fixed next_hdr, gate ipv4|ipv6       */
	MI_K_DSCP,         /* tos>>2 / (vtf&0x0fc00000)>>22, gate ipv4|ipv6          */
	MI_K_UDP_DPORT,
	MI_K_TCP_DPORT,
	MI_K_UDP_SPORT,
	MI_K_TCP_SPORT,
	MI_K_SIP,
	MI_K_DIP,
	MI_K_SIP6,
	MI_K_DIP6,
	MI_K_SPI,          /* l4+4 (AH) / l4+0 (ESP)                                 */
	MI_K_NEVER,        /* LD_VNI: accepted at create, never matches (:1250)      */
	MI_K_CUSTOM_FRAME, /* bytes at offset, gate len > offset+size                */
	MI_K_CUSTOM_L3,    /* bytes at l3+offset, gate l2 & l3 valid & len > ...     */
	MI_K_ALWAYS,       /* INNER_HDR_OFF: always passes (:1504)                   */
	MI_K_COUNT
};

typedef struct mi_term {
	uint8_t  kind;          /* MI_K_*                                            */
	uint8_t  size;          /* val_sz                                            */
	uint16_t rsv0;
	uint32_t offset;        /* custom offset                                     */
	uint32_t rsv1[2];
	uint32_t mask[4];       /* little-endian packing of the mask bytes           */
	uint32_t value[4];      /* pre-masked value bytes (pmr_create_term, :757)    */
} mi_term_t;

/* ------------------------------------------------------------------------
 * Context and entry points
 * ---------------------------------------------------------------------- */
typedef struct mi_cls_ctx mi_cls_ctx_t;

/* Number of visible HIP devices (>= 0), or a negative errno. */
int mi_cls_device_count(void);

/* Create a classification context bound to HIP device `device`. */
int mi_cls_ctx_create(int device, mi_cls_ctx_t **ctx);
int mi_cls_ctx_destroy(mi_cls_ctx_t *ctx);

/* Upload a compiled rule table (host memory, mi_tbl_hdr_t blob) to the
 * context's device copy, stream-ordered on `stream` (hipStream_t, NULL =
 * default stream).  Validates the blob; -EINVAL on a malformed table. */
int mi_cls_rules_load(mi_cls_ctx_t *ctx, const void *tbl, size_t bytes, void *stream);

/* Parse + classify n packets.
 *   pkts_dev  packed packet bytes; each packet starts at pkts_dev + off_dev[i]
 *             (any alignment).  Loads are 16-B pieces at frame-relative
 *             offsets, so the buffer must be readable up to
 *             off_dev[i] + round_up(len_dev[i], 16) for every packet: when
 *             off_dev[i] is not a multiple of 16 that is up to 15 bytes past
 *             the next 16-byte boundary after the packet (a batch whose
 *             allocation ends right after its last frame needs 16 B of slack).
 *   off_dev   uint32 byte offsets, len_dev uint16 frame lengths (FCS stripped)
 *   out_dev   n result records
 *   n         at most MI_CLS_MAX_BATCH: the kernels address the records
 *             through a buffer descriptor, whose byte range is 32 bits wide
 *             (-EINVAL above it)
 * Stream-ordered on `stream`; returns after the launch is enqueued. */
#define MI_CLS_MAX_BATCH ((1u << 28) - 1u)
int mi_cls_classify(mi_cls_ctx_t *ctx, const uint8_t *pkts_dev, const uint32_t *off_dev,
		    const uint16_t *len_dev, uint32_t n, mi_cls_result_t *out_dev,
		    void *stream);

/* Host-memory batch (the pktio receive path, loop.c:253-384 / pcap.c:280-401):
 * classifies n frames packed at pkts_host (offsets relative to it, every
 * frame inside `bytes`), writes the n records to out_host and waits.
 * When pkts_host, off_host, len_host and out_host are all page-locked
 * (mi_cls_host_alloc, hipHostMalloc, hipHostRegister) the kernel reads the
 * frames' header windows and the descriptors in place and writes the records
 * in place (zero copy: only the bytes it touches cross the host link);
 * otherwise the frames and descriptors are copied to the context's device
 * staging buffers on its own stream and the records copied back. */
int mi_cls_classify_host(mi_cls_ctx_t *ctx, const uint8_t *pkts_host, size_t bytes,
			 const uint32_t *off_host, const uint16_t *len_host, uint32_t n,
			 mi_cls_result_t *out_host);

/* Pipelined form of mi_cls_classify_host: enqueue the batch on the context's
 * stream and return a ticket (0 for n == 0); mi_cls_classify_host_wait(ticket)
 * returns once its records are in out_host.  The caller leaves all four
 * buffers untouched in between.  Up to 8 batches may be in flight; batches
 * complete in submission order.  A rule load waits for the batches in
 * flight, which classify under the rules they were submitted with.
 * Replaces nothing in the reference (its receive burst parses
 * synchronously, pktio/loop.c:253-384): it lets the runtime overlap one
 * burst's classification with delivering the previous one. */
int mi_cls_classify_host_submit(mi_cls_ctx_t *ctx, const uint8_t *pkts_host, size_t bytes,
				const uint32_t *off_host, const uint16_t *len_host, uint32_t n,
				mi_cls_result_t *out_host, uint64_t *ticket);
int mi_cls_classify_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* Program-specialised kernel of the loaded rules.  A program whose default
 * CoS has a classification block and whose rules do not form a CoS tree
 * gets a kernel with that block compiled in as constants (hipRTC, in the
 * background after mi_cls_rules_load; launches use the generic kernel until
 * it is ready -- the records are the same either way).  Blocks until the
 * compilation of the loaded program's kernel has ended: 0 = the specialised
 * kernel is in use, 1 = none (no such block, a CoS tree, disabled by
 * MI_CLS_JIT=0, or it failed to compile), -EINVAL = no rules loaded. */
int mi_cls_spec_wait(mi_cls_ctx_t *ctx);

/* Host-only (no device needed): compile the specialised kernel of a
 * compiled table's program for block shape nw (4, 12, 16) synchronously
 * (the tree form for CoS trees, which the data path does not use).
 * 0 compiled, 1 the default CoS has no classification block, < 0 error
 * (-ENOEXEC: the compile failed).  Tests use it to check the embedded
 * kernel sources build. */
int mi_cls_spec_compile(const void *tbl, size_t bytes, int nw);

/* State of the specialised-kernel compiler (host only): *running = compiler
 * processes alive (at most 1: one compile at a time), *queued = 1 if a
 * request waits to start (a newer request replaces it), *cached = distinct
 * programs kept (at most 64; later programs run the generic kernels).
 * Returns 1 while the compile thread is active, else 0. */
int mi_cls_spec_pending(uint32_t *running, uint32_t *queued, uint32_t *cached);

/* The kernel instantiation the context's last mi_cls_classify (or
 * mi_cls_parse: see there) launched
 * (diagnostics: bench lines and fault records name it).  info[0] waves per
 * block, [1] 1 if the hot region was in LDS, [2] 1 if the per-lane CoS-tree
 * rounds were compiled in (DIV), [3] flat engine + 1 (0: not a flat
 * kernel), [4] 1 if program-specialised, [5] 1 if the pktin-option kernel
 * (CK), [6] grid (blocks).  All zero before the first launch.  Returns the
 * number of words written (min(n, MI_CLS_LAUNCH_INFO_WORDS)) or -EINVAL. */
#define MI_CLS_LAUNCH_INFO_WORDS 7
int mi_cls_last_launch(const mi_cls_ctx_t *ctx, uint32_t *info, uint32_t n);

/* ------------------------------------------------------------------------
 * Multi-GPU: one host batch over several devices.
 * The batch shards with no exchange step: mi_cls_shard cuts it into
 * contiguous slices balanced by the bytes the kernel reads per packet
 * (min(len,128) + 6 B descriptor + 16 B record); each slice is staged,
 * classified and copied back on its own context and stream, all devices in
 * flight at once; the records land at their packets' positions in `out`, so
 * the result is the single-device result and per-queue arrival order is the
 * one the reference's _odp_cls_enq runs see
 * (platform/linux-generic/include/odp_classification_internal.h:208-236).
 * Replaces running the per-burst loopback_recv (pktio/loop.c:253-384) once
 * per device.
 * ---------------------------------------------------------------------- */
typedef struct mi_cls_group mi_cls_group_t;

/* begin[0..nshards]: slice k is packets [begin[k], begin[k+1]). */
int mi_cls_shard(const uint16_t *len, uint32_t n, uint32_t nshards, uint32_t *begin);

/* One context per entry of devices[] (an id may repeat: several contexts on
 * one device). */
int mi_cls_group_create(const int *devices, uint32_t n, mi_cls_group_t **group);
int mi_cls_group_destroy(mi_cls_group_t *group);
uint32_t mi_cls_group_size(const mi_cls_group_t *group);
mi_cls_ctx_t *mi_cls_group_ctx(mi_cls_group_t *group, uint32_t i);
/* The rule table replicated to every device (synchronous). */
int mi_cls_group_rules_load(mi_cls_group_t *group, const void *tbl, size_t bytes);
int mi_cls_group_pktin_opt_set(mi_cls_group_t *group, uint64_t opt);
/* As mi_cls_classify_host, sharded over the group's devices; returns when
 * every record is in out_host.  Pinned input (mi_cls_host_alloc) lets the
 * devices' copies overlap. */
int mi_cls_group_classify_host(mi_cls_group_t *group, const uint8_t *pkts_host, size_t bytes,
			       const uint32_t *off_host, const uint16_t *len_host, uint32_t n,
			       mi_cls_result_t *out_host);

/* Pipelined form of mi_cls_group_classify_host (the multi-GPU receive
 * path's submit / wait, as mi_cls_classify_host_submit for one context):
 * every device's slice is put in flight and a ticket returned;
 * mi_cls_group_classify_host_wait(ticket) returns once all records are in
 * out_host.  Batch, descriptors and records must be page-locked
 * (mi_cls_host_alloc) to be read and written in place; otherwise the batch
 * is classified synchronously and *ticket is 0 (done).  Up to 8 batches in
 * flight, completed in submission order.  Replaces running the receive
 * burst (pktio/loop.c:253-384) once per device, synchronously. */
int mi_cls_group_classify_host_submit(mi_cls_group_t *group, const uint8_t *pkts_host, size_t bytes,
				      const uint32_t *off_host, const uint16_t *len_host, uint32_t n,
				      mi_cls_result_t *out_host, uint64_t *ticket);
int mi_cls_group_classify_host_wait(mi_cls_group_t *group, uint64_t ticket);

/* pktin parse options for the following classify calls on this context:
 * odp_pktin_config_opt_t.all_bits (include/odp_rt.h; reference
 * include/odp/api/spec/packet_io.h odp_pktin_config_opt_t).  Bits 2-5
 * validate the IPv4 header / UDP / TCP / SCTP checksums (odp_parse.c:134-141,
 * 298-313, odp_packet.c:2065-2138: l3/l4_chksum_done in in_flags bits 30/31,
 * l3/l4_chksum_err in err bits 2/6), bits 6-10 drop packets with IPv4 /
 * IPv6 / UDP / TCP / SCTP errors (MI_CLS_OUT_PARSE_DROP).  0 (the default)
 * is the plain parse.  Replaces the `opt` argument of
 * _odp_packet_parse_common (include/odp_parse_internal.h:80-112). */
int mi_cls_pktin_opt_set(mi_cls_ctx_t *ctx, uint64_t opt);

/* Largest batch the context's caller will classify per call (0: unknown,
 * the default).  Only a performance hint for the kernel's block shape:
 * batches of a few thousand packets (receive bursts) spread over more CUs
 * in 4-wave blocks, large batches use one 16-wave block per CU sharing a
 * tile queue.  Results never depend on it; the program-specialised kernel
 * is rebuilt for the shape it implies.  No reference counterpart (the
 * reference classifies one packet per call, pktio/loop.c:283-339). */
int mi_cls_batch_hint(mi_cls_ctx_t *ctx, uint32_t max_batch);

/* ------------------------------------------------------------------------
 * pktout checksum insertion: the transmit half of the checksum offloads
 * (reference pktio/loop.c:386-472 loopback_fix_checksums, odp_packet.c:
 * 1888-2063 _odp_packet_{ipv4,udp,tcp,sctp}_chksum_insert).  Per packet the
 * IPv4 header checksum, the UDP or TCP checksum, or the SCTP CRC-32C is
 * computed and written into the frame.  Nothing is parsed: l3 / l4 are the
 * packet's offsets as its metadata has them (0xFFFF: invalid).
 *   IP version from frame[l3] >> 4: 4 with len - l3 >= 20 (protocol
 *   frame[l3 + 9], 255 when MF or the fragment offset is set), 6 with
 *   len - l3 >= 40 (next header frame[l3 + 6], no extension-header walk);
 *   anything else: nothing is written.
 *   A checksum is inserted when the packet is of its protocol and
 *   (<l>_chksum_set ? <l>_chksum : the pktout_opt bit): IPv4 under the L3
 *   pair, UDP (17) / TCP (6) / SCTP (132) under the L4 pair.  pktout_opt is
 *   odp_pktout_config_opt_t.all_bits >> 1 (all_bits without ts_ena, its bit
 *   0): bits 4-7 ipv4 / udp / tcp / sctp _chksum (the _ena bits 0-3 are not
 *   consulted, as in loop.c).
 *   IPv4: over the 4 IHL header bytes, stored at l3 + 10; not when IHL < 5
 *   or the header ends past the frame.  UDP / TCP: pseudo header from the
 *   addresses as stored, the protocol, and the UDP length field as stored
 *   (TCP: len - l4), then [l4, len); UDP 0 is stored as 0xFFFF; UDP at
 *   l4 + 6, TCP at l4 + 16 (the reference stores TCP at l4 + 6, odp_packet.c:
 *   1988: a deviation).  SCTP: CRC-32C, init ~0, over [l4, len) with the
 *   field zero, complemented, little-endian at l4 + 8.
 *   Contract for the L4 checksums: l4 valid, l4 - l3 even and at least 20
 *   (IPv4) / 40 (IPv6), the checksum field wholly inside the frame; a packet
 *   that violates it is left unchanged for that protocol.  No byte outside
 *   [off, off + len) is stored.  Two descriptors naming one frame: undefined.
 * ---------------------------------------------------------------------- */
typedef struct mi_cls_tx_desc {
	uint16_t l3, l4;        /* offsets from the frame start, 0xFFFF invalid     */
	uint8_t  flags;         /* MI_CLS_TXF_*                                     */
	uint8_t  rsv[3];
} mi_cls_tx_desc_t;     /* 8 B */

#define MI_CLS_TXF_L3_SET 0x01u  /* l3_chksum_set: the L3 override is valid       */
#define MI_CLS_TXF_L3     0x02u  /* l3_chksum: insert (1) / do not insert (0)     */
#define MI_CLS_TXF_L4_SET 0x04u  /* l4_chksum_set                                 */
#define MI_CLS_TXF_L4     0x08u  /* l4_chksum                                     */
/* the packet's metadata flags (odp_packet_has_udp() ...), read by mi_cls_tx_hash
 * only: the checksum entries ignore them */
#define MI_CLS_TXF_UDP    0x10u
#define MI_CLS_TXF_TCP    0x20u
#define MI_CLS_TXF_IPV4   0x40u
#define MI_CLS_TXF_IPV6   0x80u

/* done[i]: the checksums written into packet i */
#define MI_CLS_TX_IPV4 1u
#define MI_CLS_TX_UDP  2u
#define MI_CLS_TX_TCP  4u
#define MI_CLS_TX_SCTP 8u

/* Insert into n packets in device memory: the batch contract of
 * mi_cls_classify (offsets, any alignment, the readable tail up to each
 * frame's 16-B rounding); desc_dev 8-byte aligned; done_dev (n bytes) may be
 * NULL.  The context needs no rules.  Stream-ordered on `stream`; returns
 * after the launch is enqueued.  n == 0: 0.  No device: -ENODEV. */
int mi_cls_chksum_insert(mi_cls_ctx_t *ctx, uint8_t *pkts_dev, const uint32_t *off_dev,
			 const uint16_t *len_dev, const mi_cls_tx_desc_t *desc_dev, uint32_t n,
			 uint64_t pktout_opt, uint8_t *done_dev, void *stream);

/* Host-memory batch (the pktio send path): inserts into the n frames packed
 * at pkts_host (every frame inside `bytes`) and waits.  When pkts_host,
 * off_host, len_host, desc_host (and done_host, if given) are page-locked
 * (mi_cls_host_alloc) and every frame's 16-B rounding lies inside `bytes`
 * the kernel works on the frames in place; otherwise the batch goes through
 * the context's staging buffers and the frames are copied back.  The submit
 * form returns a ticket of the context's ring (mi_cls_classify_host_submit:
 * 0 for n == 0, up to 8 batches in flight, buffers untouched until the
 * wait). */
int mi_cls_chksum_insert_host(mi_cls_ctx_t *ctx, uint8_t *pkts_host, size_t bytes,
			      const uint32_t *off_host, const uint16_t *len_host,
			      const mi_cls_tx_desc_t *desc_host, uint32_t n, uint64_t pktout_opt,
			      uint8_t *done_host);
int mi_cls_chksum_insert_host_submit(mi_cls_ctx_t *ctx, uint8_t *pkts_host, size_t bytes,
				     const uint32_t *off_host, const uint16_t *len_host,
				     const mi_cls_tx_desc_t *desc_host, uint32_t n, uint64_t pktout_opt,
				     uint8_t *done_host, uint64_t *ticket);
int mi_cls_chksum_insert_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* ------------------------------------------------------------------------
 * The pktin flow hash of the loop pktio (reference pktio/loop.c:479-530
 * get_dest_queue), a step of the transmit kernel: per packet
 * odp_hash_crc32c(string, n, 0) -- the raw reflected CRC-32C, no final
 * inversion -- into hash_out[i]; the modulo by the queue count is the
 * caller's.  The string is decided by the packet's metadata alone, the
 * MI_CLS_TXF_UDP / TCP / IPV4 / IPV6 bits of its descriptor and l3 / l4 (the
 * frame is not parsed), under hash_proto = odp_pktin_hash_proto_t.all_bits
 * (bit 0 ipv4_udp, 1 ipv4_tcp, 2 ipv4, 3 ipv6_udp, 4 ipv6_tcp, 5 ipv6;
 * 1..63):
 *   l4 valid: (ipv4_udp | ipv6_udp) and TXF_UDP: the 4 bytes at l4 when
 *   l4 + 8 <= len; else (ipv4_tcp | ipv6_tcp) and TXF_TCP: the 4 bytes at l4
 *   when l4 + 20 <= len.  A UDP packet whose header does not fit appends
 *   nothing (the TCP branch is not tried).
 *   l3 valid: ipv4 and TXF_IPV4: the 8 bytes at l3 + 12 when l3 + 20 <= len;
 *   else ipv6 and TXF_IPV6: the 32 bytes at l3 + 8 when l3 + 40 <= len.
 *   The empty string hashes to 0.
 * chksum != 0: the same launch also inserts the checksums, exactly as
 * mi_cls_chksum_insert with this pktout_opt, these descriptors and `done`,
 * and the hash is of the frame as the insertion leaves it (the reference
 * fixes the checksums, then picks the queue: loop.c:581-582).  That matters
 * only where the metadata contradicts the bytes and puts a checksum field
 * into the string: TXF_IPV6 on an IPv4 frame, an l4 inside the IPv4 header.
 * chksum == 0 (no default and no override of the call asks for a checksum):
 * the hash alone; no frame byte is written, pktout_opt is not read and done,
 * where given, is zeroed.  hash_out: n words, required.  Otherwise the
 * arguments, the batch contract, the host forms (in place when every array,
 * hash_out too, is page-locked; else staged, hash_out copied back with done
 * and -- chksum != 0 only -- the frames), the tickets and the error codes
 * are those of mi_cls_chksum_insert*.
 * ---------------------------------------------------------------------- */
int mi_cls_tx_hash(mi_cls_ctx_t *ctx, uint8_t *pkts_dev, const uint32_t *off_dev,
		   const uint16_t *len_dev, const mi_cls_tx_desc_t *desc_dev, uint32_t n,
		   uint64_t pktout_opt, uint8_t *done_dev, uint32_t hash_proto, uint32_t *hash_out_dev,
		   int chksum, void *stream);
int mi_cls_tx_hash_host(mi_cls_ctx_t *ctx, uint8_t *pkts_host, size_t bytes,
			const uint32_t *off_host, const uint16_t *len_host,
			const mi_cls_tx_desc_t *desc_host, uint32_t n, uint64_t pktout_opt,
			uint8_t *done_host, uint32_t hash_proto, uint32_t *hash_out_host, int chksum);
int mi_cls_tx_hash_host_submit(mi_cls_ctx_t *ctx, uint8_t *pkts_host, size_t bytes,
			       const uint32_t *off_host, const uint16_t *len_host,
			       const mi_cls_tx_desc_t *desc_host, uint32_t n, uint64_t pktout_opt,
			       uint8_t *done_host, uint32_t hash_proto, uint32_t *hash_out_host,
			       int chksum, uint64_t *ticket);
int mi_cls_tx_hash_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* ------------------------------------------------------------------------
 * The parse on its own: odp_packet_parse() / odp_packet_parse_multi() for a
 * batch (reference odp_packet.c:2140-2229 over odp_parse.c:23-105 _odp_parse_eth
 * and :362-488 _odp_packet_parse_common_l3_l4, then odp_packet.c:2065-2138
 * _odp_packet_l4_chksum).  No rule program takes part and the context needs
 * no rules.  Per call:
 *   proto       where the parse starts: an Ethernet header, or an IPv4 / IPv6
 *               header (then no L2 flag is set and l3_offset is 0);
 *   last_layer  where it stops: L2 (the return at odp_parse.c:372-375: L2
 *               flags and the snap-length error, l4_offset invalid), L3 (:412:
 *               also the L3 flags, the IP and IPv4-checksum errors and
 *               l4_offset as the L3 parsers set it), L4 or ALL (the same);
 *   chksums     odp_proto_chksums_t.all_chksum: bit 0 ipv4, 1 udp, 2 tcp, 3
 *               sctp -- the checksums to validate (no drop rules).
 * The caller folds a packet's parse offset into the batch: off[i] is the
 * byte where parsing starts and len[i] = frame_len - offset (every length
 * odp_parse.c tests is relative to that); any alignment.  The batch contract
 * of mi_cls_classify holds (readable up to each frame's 16-B rounding).
 * The record: in_flags, err, l3_offset / l4_offset relative to the parse
 * start (0xFFFF invalid); outcome MI_CLS_OUT_ENQ where odp_packet_parse
 * returns 0, MI_CLS_OUT_PARSE_DROP where it returns -1 (an error bit left
 * after the layer cut, or a truncated TCP / UDP / SCTP header at layer >= L4,
 * which sets none); cos, hops, queue, mark 0.
 * ---------------------------------------------------------------------- */
#define MI_CLS_PROTO_ETH  1u   /* odp_proto_t */
#define MI_CLS_PROTO_IPV4 2u
#define MI_CLS_PROTO_IPV6 3u
#define MI_CLS_LAYER_L2   1u   /* odp_proto_layer_t */
#define MI_CLS_LAYER_L3   2u
#define MI_CLS_LAYER_L4   3u
#define MI_CLS_LAYER_ALL  4u
#define MI_CLS_CHKSUM_IPV4 1u  /* odp_proto_chksums_t.all_chksum */
#define MI_CLS_CHKSUM_UDP  2u
#define MI_CLS_CHKSUM_TCP  4u
#define MI_CLS_CHKSUM_SCTP 8u

typedef struct mi_cls_parse_param {
	uint32_t proto;         /* MI_CLS_PROTO_*                                   */
	uint32_t last_layer;    /* MI_CLS_LAYER_*                                   */
	uint32_t chksums;       /* MI_CLS_CHKSUM_* bits (others ignored)            */
} mi_cls_parse_param_t;

/* Parse n packets in device memory; out_dev 16-byte aligned.  Stream-ordered
 * on `stream`; returns after the launch is enqueued.  n == 0: 0.  proto or
 * last_layer out of range: -EINVAL.  No device: -ENODEV.  mi_cls_last_launch
 * reports this launch too: info[0] 4, [1]-[4] 0, [5] 1 when checksum code
 * ran, [6] the grid. */
int mi_cls_parse(mi_cls_ctx_t *ctx, const uint8_t *pkts_dev, const uint32_t *off_dev,
		 const uint16_t *len_dev, uint32_t n, const mi_cls_parse_param_t *param,
		 mi_cls_result_t *out_dev, void *stream);

/* Host-memory batch, with the semantics of mi_cls_chksum_insert_host and its
 * submit / wait forms: pkts_host, off_host, len_host and out_host page-locked
 * (mi_cls_host_alloc) and every frame's 16-B rounding inside `bytes`: read
 * and written in place; otherwise through the context's staging buffers
 * (nothing is copied back but the records: a parse writes no frame byte).
 * Tickets come from the context's ring. */
int mi_cls_parse_host(mi_cls_ctx_t *ctx, const uint8_t *pkts_host, size_t bytes,
		      const uint32_t *off_host, const uint16_t *len_host, uint32_t n,
		      const mi_cls_parse_param_t *param, mi_cls_result_t *out_host);
int mi_cls_parse_host_submit(mi_cls_ctx_t *ctx, const uint8_t *pkts_host, size_t bytes,
			     const uint32_t *off_host, const uint16_t *len_host, uint32_t n,
			     const mi_cls_parse_param_t *param, mi_cls_result_t *out_host,
			     uint64_t *ticket);
int mi_cls_parse_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* ------------------------------------------------------------------------
 * LSO: large send offload segmentation of a batch (reference
 * odp_packet_io.c:3089-3152 _odp_lso_num_packets, :3154-3251
 * _odp_lso_create_packets, :2985-3018 lso_update_ipv4, :3020-3087
 * lso_update_custom).  A source packet of `len` bytes with a header of
 * hdr_len bytes is cut into nseg segments: each is the header followed by
 * seg_payload bytes of the payload (the last one by what is left), and its
 * header is then edited by the packet's profile:
 *   IPv4    tot_len = (uint16_t)(seg_len - l3); fragment word = the stored one
 *           + (k * seg_payload) / 8 in 16 bits, MF added for k < nseg - 1;
 *           the header checksum recomputed over 20 bytes at l3 + 10.  A header
 *           whose IHL is not 5 fails the packet (MI_CLS_LSO_ST_IHL).
 *   custom  up to 8 fields in order, a later one seeing what an earlier one
 *           wrote: ADD_SEGMENT_NUM adds k to a big-endian 1/2/4/8-byte field
 *           (wrapping), WRITE_BITS sets (b & ~mask) | (value & mask) in one
 *           byte with the first (k == 0) / last (k == nseg - 1) / middle pair.
 *           A field that reaches past the packet's shortest (last) segment
 *           fails the packet (MI_CLS_LSO_ST_FIELD).
 * A failed packet's segments are not written; st[i] tells.
 * ---------------------------------------------------------------------- */
#define MI_CLS_LSO_MAX_SEGMENTS 64u        /* PKTIO_LSO_MAX_SEGMENTS            */
#define MI_CLS_LSO_MAX_PAYLOAD_OFFSET 128u /* PKTIO_LSO_MAX_PAYLOAD_OFFSET      */
#define MI_CLS_LSO_PROFILES 16u            /* PKTIO_LSO_PROFILES                */
#define MI_CLS_LSO_MAX_CUSTOM 8u           /* ODP_LSO_MAX_CUSTOM                */
#define MI_CLS_LSO_PROTO_CUSTOM 1u         /* odp_lso_protocol_t                */
#define MI_CLS_LSO_PROTO_IPV4 2u
#define MI_CLS_LSO_ADD_SEGMENT_NUM 1u      /* odp_lso_modify_t                  */
#define MI_CLS_LSO_WRITE_BITS 5u
#define MI_CLS_LSO_L3_INVALID 0xFFFFu

/* st[i] */
#define MI_CLS_LSO_ST_OK 0u
#define MI_CLS_LSO_ST_IHL 1u    /* IPv4 profile: IHL != 5                          */
#define MI_CLS_LSO_ST_FIELD 2u  /* custom field past a segment's end               */
#define MI_CLS_LSO_ST_DESC 3u   /* descriptor the kernel refuses (device form only:
				 * the host forms reject it before the launch)   */

typedef struct mi_cls_lso_field {
	uint8_t mod_op;         /* MI_CLS_LSO_ADD_SEGMENT_NUM / _WRITE_BITS          */
	uint8_t offset;         /* from the frame start, <= 128                      */
	uint8_t size;           /* 1, 2, 4, 8 (WRITE_BITS: 1)                        */
	uint8_t rsv;
	uint8_t mask[3];        /* WRITE_BITS: first, middle, last segment           */
	uint8_t value[3];
	uint8_t rsv2[2];
} mi_cls_lso_field_t;   /* 12 B */

typedef struct mi_cls_lso_profile {
	uint8_t proto;          /* MI_CLS_LSO_PROTO_*                                */
	uint8_t num_custom;     /* <= 8                                              */
	uint8_t rsv[2];
	mi_cls_lso_field_t field[8];
} mi_cls_lso_profile_t; /* 100 B */

/* One source packet (16 B, 16-byte aligned). */
typedef struct mi_cls_lso_desc {
	uint16_t hdr_len;       /* payload offset, <= 128                            */
	uint16_t seg_payload;   /* payload bytes per full segment (mi_cls_lso_plan)  */
	uint16_t l3;            /* IPv4 profile: the IP header's offset              */
	uint8_t  profile;       /* index into the profile table                      */
	uint8_t  nseg;          /* 2..64                                             */
	uint32_t first_seg;     /* its first entry of the segment table              */
	uint32_t rsv;
} mi_cls_lso_desc_t;

/* One segment: where it goes and whose it is (segment k of source `src` is
 * entry desc[src].first_seg + k). */
typedef struct mi_cls_lso_seg {
	uint32_t off;           /* byte offset in the destination buffer             */
	uint32_t src;           /* index of its source packet                        */
} mi_cls_lso_seg_t;     /* 8 B */

/* Host-only (no device needed): the segmentation plan of one packet,
 * _odp_lso_num_packets (odp_packet_io.c:3089-3152).  proto MI_CLS_LSO_PROTO_*,
 * l3 the packet's L3 offset (MI_CLS_LSO_L3_INVALID: none; read for IPv4 only).
 * Returns the number of segments (1: the packet goes out as it is;
 * *seg_payload = max_payload, *left_over = 0) or -EINVAL.  Deviation: a
 * payload length of 0 (max_payload 0, or IPv4 with max_payload < 8), on which
 * the reference divides by zero, is -EINVAL. */
int mi_cls_lso_plan(uint32_t len, uint32_t hdr_len, uint32_t max_payload, uint32_t proto, uint32_t l3,
		    uint32_t *seg_payload, uint32_t *left_over);

/* Segment n source packets in device memory into nsegs segments.  src_dev /
 * off_dev / len_dev under the batch contract of mi_cls_classify (the kernel
 * reads no byte outside [off, off + len)); desc_dev 16-byte and seg_dev
 * 8-byte aligned; dst_dev may be src_dev, no segment overlapping a source
 * frame or another segment; st_dev n bytes.  Exactly the bytes
 * [seg.off, seg.off + seg_len) of every segment are written.  The profile
 * table (nprof <= 16, host memory) travels by value with the launch.
 * Stream-ordered on `stream`.  n == 0 or nsegs == 0: 0.  No device: -ENODEV.
 * nprof > 16, a profile's protocol, num_custom, a field's mod_op, offset or
 * size out of range: -EINVAL before any launch (the host forms check the
 * descriptors the same way: profile index, nseg 2..64, hdr_len, the segment
 * table and every source and segment inside its buffer).
 * mi_cls_last_launch: info[0] 64 + the waves per block (68), [1]-[5] 0, [6]
 * the grid. */
int mi_cls_lso_segment(mi_cls_ctx_t *ctx, const uint8_t *src_dev, const uint32_t *off_dev,
		       const uint16_t *len_dev, const mi_cls_lso_desc_t *desc_dev, uint32_t n,
		       uint8_t *dst_dev, const mi_cls_lso_seg_t *seg_dev, uint32_t nsegs,
		       const mi_cls_lso_profile_t *prof, uint32_t nprof, uint8_t *st_dev, void *stream);

/* Host-memory batch, with the semantics of mi_cls_chksum_insert_host and its
 * submit / wait forms.  src_host (src_bytes) and dst_host (dst_bytes) are
 * either one buffer (equal pointers and sizes) or two that do not overlap.
 * All of src, dst, off, len, desc, seg and st page-locked (mi_cls_host_alloc):
 * worked on in place; otherwise through the context's staging buffers, and
 * only the destination segments (and st) are copied back. */
int mi_cls_lso_segment_host(mi_cls_ctx_t *ctx, const uint8_t *src_host, size_t src_bytes,
			    const uint32_t *off_host, const uint16_t *len_host,
			    const mi_cls_lso_desc_t *desc_host, uint32_t n, uint8_t *dst_host,
			    size_t dst_bytes, const mi_cls_lso_seg_t *seg_host, uint32_t nsegs,
			    const mi_cls_lso_profile_t *prof, uint32_t nprof, uint8_t *st_host);
int mi_cls_lso_segment_host_submit(mi_cls_ctx_t *ctx, const uint8_t *src_host, size_t src_bytes,
				   const uint32_t *off_host, const uint16_t *len_host,
				   const mi_cls_lso_desc_t *desc_host, uint32_t n, uint8_t *dst_host,
				   size_t dst_bytes, const mi_cls_lso_seg_t *seg_host, uint32_t nsegs,
				   const mi_cls_lso_profile_t *prof, uint32_t nprof, uint8_t *st_host,
				   uint64_t *ticket);
int mi_cls_lso_segment_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* ------------------------------------------------------------------------
 * Receive delivery on the GPU: the host steps of loopback_recv /
 * pcapif_recv_pkt after classification (pktio/loop.c:308-373, pcap.c:
 * 330-352) for packets whose headers and buffers are in page-locked host
 * memory the device addresses at the host's addresses: each packet's
 * metadata (_odp_packet_parse_common's result at the pktio's parser layer,
 * hdr->cos / cls_mark / dst_queue of _odp_cls_classify_packet, input pktio)
 * written into its header, its frame copied into its buffer (pcap frames,
 * pool switch, _odp_pktio_packet_to_pool), and the stable group-by-queue
 * permutation of _odp_cls_enq's runs (include/odp_classification_internal.h:
 * 208-236: each queue receives its packets in arrival order).
 * ---------------------------------------------------------------------- */

/* The receive-path fields of a packet header (the runtime's packet header
 * embeds this block; odp_packet_hdr_t.p / cos / cls_mark / dst_queue /
 * input, platform/linux-generic/include/odp_packet_internal.h:55-70,112-139). */
typedef struct mi_cls_pkt_meta {
	uint32_t data_off;      /* headroom                                        */
	uint32_t len;
	uint64_t in_flags;      /* packet_parser_t.input_flags                      */
	uint8_t  err;           /* flags.all.error                                  */
	uint8_t  cos;           /* 0xFF none                                        */
	uint16_t cls_mark;
	uint16_t l2, l3, l4;
	uint16_t rsv0;
	uint32_t rsv1;
	uint64_t dst_queue;     /* odp_queue_t                                      */
	uint64_t input;         /* odp_pktio_t                                      */
	uint64_t user_ptr;
	uint64_t rsv2;
} mi_cls_pkt_meta_t;    /* 64 B: one cache line of the header, written whole */

/* One delivered packet (host-written, 48 B). */
typedef struct mi_cls_dlv {
	uint64_t meta;          /* address of its mi_cls_pkt_meta_t (64-B aligned)   */
	uint64_t dst_queue;     /* queue written into meta when the classifier is on */
	uint64_t user_ptr;      /* kept user pointer (not MI_CLS_DLV_FRESH)          */
	uint32_t src;           /* frame offset from the batch base (MI_CLS_DLV_COPY) */
	uint32_t rec;           /* index of its record                              */
	uint16_t len;           /* frame length                                     */
	uint8_t  flags;         /* MI_CLS_DLV_*                                     */
	uint8_t  qid;           /* queue group 0..MI_CLS_DLV_GROUPS-1, 0xFF none    */
	uint32_t data_off;      /* the packet's headroom (kept: not MI_CLS_DLV_FRESH) */
	uint64_t rsv;
} mi_cls_dlv_t;

#define MI_CLS_DLV_FRESH 0x01u  /* newly allocated: initialise every field     */
#define MI_CLS_DLV_COPY  0x02u  /* copy the frame into meta + data_from_meta    */
#define MI_CLS_DLV_CLS   0x04u  /* classifier on: cos / cls_mark / dst_queue    */
#define MI_CLS_DLV_GROUPS 64
/* Entries one delivery groups at most: a burst with more entries must give
 * every entry qid 0xFF (mi_cls_deliver_submit rejects it otherwise). */
#define MI_CLS_DLV_GROUP_MAX 8192
/* An entry index, a group's count and a frame's rank each travel in 16 bits:
 * gcnt bits 0-15, the rank in dec bits 16-31, the kernels' 16-bit LDS arrays
 * (s_perm / s_rank in mi_cls_kd.hip). */
#ifdef __cplusplus
static_assert(MI_CLS_DLV_GROUP_MAX <= 0xFFFF, "a burst's indexes, counts and ranks fit 16 bits");
#else
_Static_assert(MI_CLS_DLV_GROUP_MAX <= 0xFFFF, "a burst's indexes, counts and ranks fit 16 bits");
#endif

typedef struct mi_cls_dlv_args {
	const uint8_t *base;    /* the classified batch's base (host VA)           */
	const mi_cls_result_t *res;   /* its records                              */
	const mi_cls_dlv_t *dlv;
	uint32_t n;             /* entries of dlv                                   */
	uint32_t layer;         /* parser layer (ODP_PROTO_LAYER_L2..ALL = 1..4)    */
	uint64_t input;         /* odp_pktio_t written into meta                    */
	uint32_t headroom;      /* data_off of fresh packets                        */
	uint32_t data_from_meta;/* bytes from a meta block to the packet's data     */
	uint32_t *perm;         /* out: entry indexes grouped by qid (stable)       */
	uint32_t *gcnt;         /* out: MI_CLS_DLV_GROUPS entry counts per qid       */
} mi_cls_dlv_args_t;

/* Submit the delivery of a classified burst on the context's stream (after
 * its classification) and return a ticket for mi_cls_classify_host_wait.
 * Every pointer is host memory the device reads and writes in place
 * (mi_cls_host_alloc); entries with qid 0xFF are left out of perm.  More
 * than MI_CLS_DLV_GROUP_MAX entries with a queue group: -E2BIG. */
int mi_cls_deliver_submit(mi_cls_ctx_t *ctx, const mi_cls_dlv_args_t *args, uint64_t *ticket);

/* ------------------------------------------------------------------------
 * The receive chain: classification, the per-frame decisions and the
 * delivery of one burst submitted at once, with no host step between them.
 * The host's per-frame decide step of mi_cls_deliver_submit (parse drop,
 * CoS drop / discard, destination pool, too long for the pool, queue group)
 * runs on the device from a per-generation table of the control plane
 * (mi_cls_rxtab_t: CoS -> pool slot, queues, queue groups), and each frame
 * takes its packet from packets the host took from the pools before the
 * submit (pool slot k: got[got_base[k] .. + have[k]), used in arrival order).
 * A burst whose frames need more packets of a slot than were taken reports
 * `short_pool` and is delivered again by the host (nothing it would deliver
 * differently has been enqueued).  Reference steps: loop.c:308-373,
 * pcap.c:330-352, include/odp_packet_io_internal.h:352-371,
 * odp_classification.c:1742-1771, include/odp_classification_internal.h:
 * 142-236.
 * ---------------------------------------------------------------------- */
#define MI_CLS_RX_POOLS 16
#define MI_CLS_RX_QENT 1024
#define MI_CLS_RXT_CLS   0x1u   /* classifier on                               */
#define MI_CLS_RXT_GROUP 0x2u   /* every CoS enqueues plainly to <= 64 queues:   */
				/* group by queue (qg) for one enqueue per queue */
typedef struct mi_cls_rxtab {
	uint32_t flags;               /* MI_CLS_RXT_*                               */
	uint32_t npool;               /* pool slots (slot 0: the pktio's pool)      */
	uint32_t pool_cap[MI_CLS_RX_POOLS];   /* data capacity of each slot's packets */
	uint8_t  rt_slot[64];         /* runtime pool index -> slot + 1 (0: none)   */
	uint8_t  cos_pool[256];       /* CoS index -> pool slot                     */
	uint8_t  cos_nq[256];         /* queues of the CoS                          */
	uint16_t cos_q0[256];         /* its first entry of qh / qg                 */
	uint8_t  rt_pinned[64];       /* runtime pool index -> 1: page-locked pool   */
	uint64_t qh[MI_CLS_RX_QENT];  /* odp_queue_t per (CoS, queue slot)          */
	uint8_t  qg[MI_CLS_RX_QENT];  /* its queue group 0..63 (MI_CLS_RXT_GROUP)   */
	uint64_t stamp;               /* new value whenever the table is rewritten: */
				      /* the device keeps a copy per stamp          */
} mi_cls_rxtab_t;

typedef struct mi_cls_rx_out {
	uint64_t in_errors, in_discards, packets, octets;
	uint32_t used[MI_CLS_RX_POOLS];   /* packets taken of each slot              */
	uint32_t need[MI_CLS_RX_POOLS];   /* frames that wanted a packet of the slot */
	uint32_t short_pool;          /* 1: a slot had too few packets (host redo)  */
	uint32_t not_in_place;        /* loop staging (stage): a packet outside the  */
				      /* page-locked arena (host redo)              */
	uint32_t rsv[2];
} mi_cls_rx_out_t;

/* Frame decision word (dec[i]): fate in bits 0-1, pool slot in bits 2-6,
 * queue group in bits 8-14 (0x7F none), rank among the slot's frames in
 * bits 16-31. */
#define MI_CLS_RXF_DROP    0u   /* parse drop or CoS drop: nothing delivered  */
#define MI_CLS_RXF_DISCARD 1u   /* counted in in_discards                      */
#define MI_CLS_RXF_FRESH   2u   /* a packet of its slot (frame copied)         */
#define MI_CLS_RXF_INPLACE 3u   /* a loop packet received in its own buffer    */

typedef struct mi_cls_rxc_args {
	const uint8_t *base;          /* the burst's frames (soff[i] from here)     */
	const uint32_t *soff;
	const uint16_t *slen;
	mi_cls_result_t *res;         /* records (every frame's, when the ticket is done) */
	uint32_t n;                   /* frames (<= MI_CLS_DLV_GROUP_MAX)           */
	uint32_t layer;               /* parser layer (ODP_PROTO_LAYER_L2..ALL)     */
	uint64_t input;               /* odp_pktio_t written into meta              */
	uint32_t headroom;            /* data_off of fresh packets                  */
	uint32_t data_from_meta;      /* bytes from a meta block to its data        */
	const mi_cls_rxtab_t *tab;
	const uint64_t *got;          /* packets taken per slot (odp_packet_t)      */
	uint32_t got_base[MI_CLS_RX_POOLS], have[MI_CLS_RX_POOLS];
	const uint64_t *pk;           /* loop: each frame's packet, else NULL       */
	const uint8_t *ppool;         /* loop: its runtime pool index + 1           */
	const uint16_t *pdoff;        /* loop: its headroom                         */
	uint32_t meta_off;            /* bytes from a packet handle to its meta     */
	uint32_t stage;               /* loop: the device builds soff / slen / ppool */
				      /* from the packets' headers (pk) first       */
	uint16_t head_off;            /* stage: offset of a header's buffer pointer */
	uint16_t pool_off;            /* stage: offset of its u16 pool index        */
	/* outputs */
	uint32_t *dec;                /* per frame: decision word                   */
	uint64_t *ent;                /* per frame: the delivered packet (0: none)  */
	uint32_t *perm;               /* frames grouped by queue group (stable)     */
	uint32_t *gcnt;               /* MI_CLS_DLV_GROUPS: the group's frame count in
				       * bits 0-15 (MI_CLS_DLV_GROUP_MAX <= 0xFFFF); bit
				       * 24 set when they all have one CoS, its index
				       * in bits 16-23 (mi_cls_result_t.cos is 8 bits:
				       * the 256 CoS of mi_cls_rxtab_t.cos_pool)   */
	mi_cls_rx_out_t *out;
} mi_cls_rxc_args_t;

/* Submit a host batch's classification (as mi_cls_classify_host_submit)
 * followed by the decisions and the delivery of args; one ticket for all
 * (mi_cls_classify_host_wait).  Every pointer of args is page-locked host
 * memory the device addresses in place; res / soff / slen / base are the
 * classification's.  -EINVAL: not so, or n too large. */
int mi_cls_rx_chain_submit(mi_cls_ctx_t *ctx, const uint8_t *pkts, size_t bytes,
			   const mi_cls_rxc_args_t *args, uint64_t *ticket);

/* ------------------------------------------------------------------------
 * The enqueue plan: what a pktio driver does with a classified batch's
 * records, one packet at a time, before its packets are on their queues
 * (reference pktio/loop.c:311-312, 324-325, 352-355, 380-381: the counters;
 * include/odp_classification_internal.h:208-236 _odp_cls_enq: runs of equal
 * destination enqueued in arrival order), for a batch of any size and up to
 * MI_CLS_ENQ_DST_MAX destination queues.  No pools, no packet handles: every
 * enqueued record is delivered.  The CoS pool switch and the frames it leaves
 * without a packet are the pool plan's (mi_cls_pool_plan, below): plan its
 * res_out.  Per record, in arrival order:
 *   in_errors    err != 0, or outcome MI_CLS_OUT_PARSE_DROP;
 *   in_discards  outcome MI_CLS_OUT_DISCARD or MI_CLS_OUT_LOOP;
 *   delivered    outcome MI_CLS_OUT_ENQ whose (cos, queue) the table maps:
 *                queue < cos_nq[cos], cos_q0[cos] + queue < MI_CLS_ENQ_ENT and
 *                the entry's id < ndst; it goes to that destination id;
 *   stale        outcome MI_CLS_OUT_ENQ that the table does not map (the
 *                records are of other rules than the table): not delivered;
 *   packets / octets  delivered records with err == 0, and their len summed.
 * perm[n] is a permutation of 0 .. n-1: the delivered records grouped by
 * destination id ascending, arrival order inside a group, then every record
 * that is not delivered as one last group, in arrival order (one free call).
 * gbeg[ndst + 2]: group g is perm[gbeg[g] .. gbeg[g+1]); group ndst is the
 * not-delivered one; gbeg[0] == 0, gbeg[ndst + 1] == n.
 * Multi-GPU: there is no mi_cls_group_* form.  Shards planned per device
 * concatenate in shard order: a queue's packets of shard k precede those of
 * shard k + 1, which is arrival order (mi_cls_shard cuts contiguous slices).
 * ---------------------------------------------------------------------- */
#define MI_CLS_ENQ_ENT 8192      /* (CoS, queue slot) entries: 255 CoS x 32 hash queues fit */
#define MI_CLS_ENQ_DST_MAX 8192  /* destination ids                                          */
/* The kernels' shape: a block of 16 waves ranks MI_CLS_ENQ_TILE records at a
 * time and walks a contiguous run of tiles; at most MI_CLS_ENQ_GRID blocks
 * (grid = min(MI_CLS_ENQ_GRID, tiles); a batch of more tiles gives each block
 * ceil(tiles / grid) of them).  Destination ids are grouped in stable passes of
 * MI_CLS_ENQ_DIGIT bits: one pass when ndst + 1 <= 1 << MI_CLS_ENQ_DIGIT, else
 * two. */
#define MI_CLS_ENQ_TILE 1024
#define MI_CLS_ENQ_GRID 256
#define MI_CLS_ENQ_DIGIT 8

typedef struct mi_cls_enq_tab {
	uint32_t ndst;                    /* destination ids in use (<= MI_CLS_ENQ_DST_MAX) */
	uint32_t rsv;
	uint8_t  cos_nq[256];             /* CoS index -> its queues (0: none: drop CoS,
					   * invalid CoS)                                  */
	uint16_t cos_q0[256];             /* its first entry of ent_dst                     */
	uint16_t ent_dst[MI_CLS_ENQ_ENT]; /* (CoS, queue slot) -> destination id; entries
					   * of one odp_queue_t share an id                */
	uint64_t stamp;                   /* new value whenever the table is rewritten: the
					   * device keeps the copy of the last stamp        */
} mi_cls_enq_tab_t;

typedef struct mi_cls_enq_out {
	uint64_t in_errors, in_discards, packets, octets;
	uint64_t delivered;               /* records in groups 0 .. ndst-1                  */
	uint64_t stale;                   /* enqueue records the table does not map         */
} mi_cls_enq_out_t;

/* Plan n records in device memory.  res_dev / len_dev: the records and frame
 * lengths (the len_dev of mi_cls_classify); perm_dev n words, gbeg_dev
 * tab->ndst + 2 words, out_dev one mi_cls_enq_out_t (8-byte aligned): all
 * written whole, no input value of theirs is read.  tab is host memory, read
 * during the call.  The context needs no rules.  Stream-ordered on `stream`
 * (after mi_cls_classify on the same stream the records never leave the
 * device); returns after the launches are enqueued.  The scratch (11 B per
 * record) is the context's, grown by 1.5x and kept; a call on another stream
 * than the previous plan's is ordered after it.  n == 0: gbeg and out are
 * zeroed (res / len / perm may be NULL).  -EINVAL: a NULL array, or a NULL
 * context where there is a device; -ENODEV: no device; -E2BIG: tab->ndst >
 * MI_CLS_ENQ_DST_MAX.  mi_cls_last_launch: info[0] 128 + the waves per block
 * (144), [1] the digit passes (1, 2; 0 for n == 0), [2]-[5] 0, [6] the grid. */
int mi_cls_enq_plan(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_dev, const uint16_t *len_dev,
		    uint32_t n, const mi_cls_enq_tab_t *tab, uint32_t *perm_dev, uint32_t *gbeg_dev,
		    mi_cls_enq_out_t *out_dev, void *stream);

/* Host-memory batch, with the semantics of mi_cls_chksum_insert_host and its
 * submit / wait forms: res, len, perm, gbeg and out all page-locked
 * (mi_cls_host_alloc): read and written in place; otherwise the records and
 * lengths go through the context's staging buffers and perm, gbeg and out are
 * copied back.  Tickets come from the context's ring (the buffers stay
 * untouched until the wait; tab may change after the submit returns). */
int mi_cls_enq_plan_host(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_host, const uint16_t *len_host,
			 uint32_t n, const mi_cls_enq_tab_t *tab, uint32_t *perm_host,
			 uint32_t *gbeg_host, mi_cls_enq_out_t *out_host);
int mi_cls_enq_plan_host_submit(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_host,
				const uint16_t *len_host, uint32_t n, const mi_cls_enq_tab_t *tab,
				uint32_t *perm_host, uint32_t *gbeg_host, mi_cls_enq_out_t *out_host,
				uint64_t *ticket);
int mi_cls_enq_plan_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* ------------------------------------------------------------------------
 * The run plan: the per-run form of the enqueue plan, for CoS with packet
 * vectors or an event aggregator, whose deliveries follow the reference's
 * runs (include/odp_classification_internal.h:83-236 _odp_cls_enq,
 * _odp_cos_enq, _odp_cos_vector_enq) and not the queue groups.  Delivered,
 * stale, the destination id and the six counters are those of the enqueue
 * plan above, under the same mi_cls_enq_tab_t.  Per record i, in arrival
 * order, with burst(i) = i / burst (burst == 0: the whole batch is one burst):
 *   run head     a delivered record with no earlier delivered record in its
 *                burst, or whose latest earlier delivered record of its burst
 *                differs from it in (destination id, cos).  Records that are
 *                not delivered end no run; a burst's end does.  Entries that
 *                share a destination id do not break a run; the same queue
 *                under another CoS does, and so does the same CoS with
 *                another id;
 *   run          a head and the delivered records up to the next head.
 * seq[n] is a permutation of 0 .. n-1: the delivered records in arrival
 * order, then every other record in arrival order (one free call).
 * runs[]: the runs in arrival order, run r = seq[first .. first + count):
 *   plain        count < 2, or the CoS's mode has no MI_CLS_RUN_VEC: one
 *                enqueue of `count` packets -- to the queue's aggregator when
 *                flags has MI_CLS_RUN_AGGR (the CoS's bit); nvec = 0;
 *   vectors      otherwise: flags = MI_CLS_RUN_VEC, nvec = ceil(count /
 *                vmax[cos]) packet vectors of the pool of vslot[cos], all of
 *                vmax packets but the last.
 * out: the six counters, nruns (the true number of runs, also when it exceeds
 * run_cap), vectors (nvec summed over all nruns runs) and vec_need[s] (nvec
 * summed over the runs of the CoS with vslot s): a driver takes each pool's
 * vectors with one call.
 * ---------------------------------------------------------------------- */
#define MI_CLS_RUN_AGGR 0x1u     /* mode bit 0: the reference's vector.use_aggr     */
#define MI_CLS_RUN_VEC 0x2u      /* mode bit 1: not vector.use_std_enq              */
#define MI_CLS_RUN_VSLOTS 16     /* vector pools a table tells apart                */
/* The kernels' shape: a block of 16 waves walks a contiguous run of tiles of
 * MI_CLS_RUN_TILE records; at most MI_CLS_RUN_GRID blocks (grid = min(
 * MI_CLS_RUN_GRID, tiles); a batch of more tiles gives each block ceil(tiles /
 * grid) of them). */
#define MI_CLS_RUN_TILE 1024
#define MI_CLS_RUN_GRID 256

typedef struct mi_cls_run_tab {
	uint8_t  mode[256];               /* CoS index -> MI_CLS_RUN_AGGR | MI_CLS_RUN_VEC  */
	uint16_t vmax[256];               /* packets per vector (>= 1 for a VEC CoS)        */
	uint8_t  vslot[256];              /* its vector pool's slot (< MI_CLS_RUN_VSLOTS)   */
	uint64_t stamp;                   /* as mi_cls_enq_tab_t.stamp                      */
} mi_cls_run_tab_t;

typedef struct mi_cls_run {
	uint32_t first;                   /* index into seq                                 */
	uint32_t count;                   /* packets (can exceed 65535)                     */
	uint16_t dst;                     /* destination id                                 */
	uint8_t  cos;
	uint8_t  flags;                   /* MI_CLS_RUN_AGGR (plain run) or MI_CLS_RUN_VEC  */
	uint32_t nvec;
} mi_cls_run_t;

typedef struct mi_cls_run_out {
	uint64_t in_errors, in_discards, packets, octets, delivered, stale; /* mi_cls_enq_out_t */
	uint64_t nruns;
	uint64_t vectors;
	uint64_t vec_need[MI_CLS_RUN_VSLOTS];
} mi_cls_run_out_t;

/* Plan the runs of n records in device memory.  res_dev / len_dev as for
 * mi_cls_enq_plan; seq_dev n words, runs_dev run_cap entries (16-byte
 * aligned), out_dev one mi_cls_run_out_t (8-byte aligned).  seq, runs[0 ..
 * min(nruns, run_cap)) and out are written whole and no input value of theirs
 * is read; nothing past runs[min(nruns, run_cap)) is touched (a truncated
 * plan still has the true nruns: call again with room).  tab and rtab are host
 * memory, read and checked during the call.  Stream-ordered on `stream`;
 * returns after the launches are enqueued.  The scratch (12 B per record) is
 * the context's, grown by 1.5x and kept; a call on another stream than the
 * previous run plan's is ordered after it.  n == 0: out is zeroed (res / len
 * / seq / runs may be NULL).  -EINVAL: a NULL table or array (runs may be NULL
 * when run_cap == 0), a NULL context where there is a device, or a CoS with
 * MI_CLS_RUN_VEC whose vmax is 0 or whose vslot is >= MI_CLS_RUN_VSLOTS;
 * -ENODEV: no device; -E2BIG: tab->ndst > MI_CLS_ENQ_DST_MAX.
 * mi_cls_last_launch: info[0] 192 + the waves per block (208), [1] the
 * launches (5; 1 for n == 0), [2]-[5] 0, [6] the grid. */
int mi_cls_enq_runs(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_dev, const uint16_t *len_dev,
		    uint32_t n, const mi_cls_enq_tab_t *tab, const mi_cls_run_tab_t *rtab, uint32_t burst,
		    uint32_t *seq_dev, mi_cls_run_t *runs_dev, uint32_t run_cap, mi_cls_run_out_t *out_dev,
		    void *stream);

/* Host-memory batch, as mi_cls_enq_plan_host and its submit / wait forms:
 * res, len, seq, runs and out all page-locked: read and written in place;
 * otherwise the records and lengths go through the context's staging buffers
 * and seq, runs and out are copied back (the run_cap entries of runs go up
 * first, so that those past nruns come back as they were). */
int mi_cls_enq_runs_host(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_host, const uint16_t *len_host,
			 uint32_t n, const mi_cls_enq_tab_t *tab, const mi_cls_run_tab_t *rtab,
			 uint32_t burst, uint32_t *seq_host, mi_cls_run_t *runs_host, uint32_t run_cap,
			 mi_cls_run_out_t *out_host);
int mi_cls_enq_runs_host_submit(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_host,
				const uint16_t *len_host, uint32_t n, const mi_cls_enq_tab_t *tab,
				const mi_cls_run_tab_t *rtab, uint32_t burst, uint32_t *seq_host,
				mi_cls_run_t *runs_host, uint32_t run_cap, mi_cls_run_out_t *out_host,
				uint64_t *ticket);
int mi_cls_enq_runs_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* ------------------------------------------------------------------------
 * The pool plan: the first thing a pktio driver does with a classified
 * packet, before it counts and enqueues it: the move into its CoS's pool
 * (reference include/odp_packet_io_internal.h:352-371
 * _odp_pktio_packet_to_pool, called at pktio/loop.c:332-337), for a batch of
 * any size and up to MI_CLS_POOL_SLOTS pools.  A frame that gets no packet --
 * its pool ran short, or it is longer than the pool's packets -- is freed and
 * counted in in_discards by the reference and reaches no queue.  Per record i,
 * in arrival order, with slot = cos_slot[cos]; the fates are tested in this
 * order:
 *   NONE      outcome is not MI_CLS_OUT_ENQ, or the CoS has no slot (cos_slot
 *             0xFF or >= nslot: the enqueue plan's "stale"): takes no packet;
 *   INPLACE   own[i] == slot + 1: the frame already sits in a packet of that
 *             pool and stays there.  own is for loop-style drivers whose
 *             frames are packets: own[i] is that packet's slot + 1, 0 for
 *             none (a value above nslot selects nothing); own == NULL: no
 *             frame has a packet (pcap frames).  An INPLACE frame is never
 *             TOO_LONG: the reference compares the pools before it allocates;
 *   TOO_LONG  len[i] > slot_cap[slot]: the allocation fails.  It takes no rank;
 *   FRESH     rank < have[slot], where rank is the number of earlier records
 *             of the slot that are FRESH or SHORT: takes packet base[slot] +
 *             rank of the caller's array;
 *   SHORT     rank >= have[slot]: the pool ran short.
 * dec[i] = fate | slot << 4 (slot 0 for NONE).  idx[i] = base[slot] + rank for
 * FRESH, 0xFFFFFFFF for every other fate: the caller keeps every packet it
 * took in one array, slot k's at base[k] .. base[k] + have[k]; afterwards
 * those from base[k] + used[k] on go back to the pool.  res_out[i] is res[i]
 * with outcome replaced by MI_CLS_OUT_DISCARD for TOO_LONG and SHORT and no
 * other byte changed, so the plans compose: mi_cls_enq_plan or
 * mi_cls_enq_runs over res_out gives the deliveries, the free list and the
 * counters of the reference's loop with the pool switch in it -- a loser is
 * one more in_discards (loop.c:335), is in no queue group, run or vector, and
 * keeps its in_errors count.  have[k] == 0xFFFFFFFF asks for the need alone:
 * nothing is SHORT and the caller reads need[].
 * This is the reference's packet-by-packet loop under "no packet returns to a
 * pool during the batch", the assumption of the receive path's buckets too:
 * frames of one pool get packets in arrival order, so a short pool leaves the
 * same frames without one as frame-by-frame allocation from have[k] free
 * packets would.
 * Multi-GPU: there is no mi_cls_group_* form.  A shard's ranks start at zero,
 * so the caller gives each shard its own have / base (its part of the packets).
 * ---------------------------------------------------------------------- */
#define MI_CLS_POOL_SLOTS 16
/* The kernels' shape: a block of 16 waves walks a contiguous run of tiles of
 * MI_CLS_POOL_TILE records; at most MI_CLS_POOL_GRID blocks (grid = min(
 * MI_CLS_POOL_GRID, tiles); a batch of more tiles gives each block ceil(tiles /
 * grid) of them). */
#define MI_CLS_POOL_TILE 1024
#define MI_CLS_POOL_GRID 256

typedef struct mi_cls_pool_tab {
	uint32_t nslot;                        /* slots in use, <= MI_CLS_POOL_SLOTS          */
	uint32_t rsv;
	uint32_t slot_cap[MI_CLS_POOL_SLOTS];  /* longest frame a packet of the slot can hold */
	uint8_t  cos_slot[256];                /* CoS index -> slot; 0xFF: none               */
	uint64_t stamp;                        /* as mi_cls_enq_tab_t.stamp                   */
} mi_cls_pool_tab_t;

#define MI_CLS_PF_NONE     0u  /* takes no packet: not MI_CLS_OUT_ENQ, or a CoS without a slot
				  (cos_slot 0xFF or >= nslot: the enqueue plan's "stale")     */
#define MI_CLS_PF_INPLACE  1u  /* own[i] == slot + 1: the packet stays where it is            */
#define MI_CLS_PF_FRESH    2u  /* takes packet idx[i] of the caller's array                   */
#define MI_CLS_PF_TOO_LONG 3u  /* len[i] > slot_cap[slot]: the allocation fails               */
#define MI_CLS_PF_SHORT    4u  /* its rank >= have[slot]: the pool ran short                  */

typedef struct mi_cls_pool_out {
	uint64_t inplace, fresh, too_long, shorted;   /* records of each fate          */
	uint32_t need[MI_CLS_POOL_SLOTS];              /* FRESH + SHORT of the slot     */
	uint32_t used[MI_CLS_POOL_SLOTS];              /* FRESH = min(need, have)       */
} mi_cls_pool_out_t;

/* Plan the packets of n records in device memory.  res_dev / len_dev as for
 * mi_cls_enq_plan (res_dev 16-byte aligned, as mi_cls_classify writes it);
 * own_dev n bytes or NULL; res_out_dev n records (16-byte aligned; res_dev
 * itself, in place, or an array disjoint from it), dec_dev and idx_dev n words,
 * out_dev one mi_cls_pool_out_t (8-byte aligned): all written whole, no input
 * value of theirs is read.  tab, have and base are host memory, read during
 * the call.  The context needs no rules.  Stream-ordered on `stream`; returns
 * after the launches are enqueued.  The scratch is the context's (of fixed
 * size on this path; the staged host form's 9 B per record are grown by 1.5x
 * and kept); a call on another stream than the previous pool plan's is ordered
 * after it.  n == 0: out is zeroed (the arrays may be NULL).  -EINVAL: a NULL
 * table, have, base, out or (n > 0) array other than own; tab->nslot >
 * MI_CLS_POOL_SLOTS; n > MI_CLS_MAX_BATCH; base[k] + min(have[k], n) past
 * 0xFFFFFFFE for a slot k < nslot; a misaligned res, res_out or out; a NULL
 * context where there is a device.  -ENODEV: no device.
 * mi_cls_last_launch: info[0] 256 + the waves per block (272), [1] the
 * launches (3; 1 for n == 0), [2]-[5] 0, [6] the grid. */
int mi_cls_pool_plan(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_dev, const uint16_t *len_dev,
		     const uint8_t *own_dev /* may be NULL */, uint32_t n,
		     const mi_cls_pool_tab_t *tab,
		     const uint32_t have[MI_CLS_POOL_SLOTS], const uint32_t base[MI_CLS_POOL_SLOTS],
		     mi_cls_result_t *res_out_dev, uint32_t *dec_dev, uint32_t *idx_dev,
		     mi_cls_pool_out_t *out_dev, void *stream);

/* Host-memory batch, as mi_cls_enq_plan_host and its submit / wait forms:
 * res, len, own (if given), res_out, dec, idx and out all page-locked: read
 * and written in place; otherwise the records, lengths and own go through the
 * context's staging buffers and res_out, dec, idx and out are copied back. */
int mi_cls_pool_plan_host(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_host, const uint16_t *len_host,
			  const uint8_t *own_host, uint32_t n, const mi_cls_pool_tab_t *tab,
			  const uint32_t have[MI_CLS_POOL_SLOTS], const uint32_t base[MI_CLS_POOL_SLOTS],
			  mi_cls_result_t *res_out_host, uint32_t *dec_host, uint32_t *idx_host,
			  mi_cls_pool_out_t *out_host);
int mi_cls_pool_plan_host_submit(mi_cls_ctx_t *ctx, const mi_cls_result_t *res_host,
				 const uint16_t *len_host, const uint8_t *own_host, uint32_t n,
				 const mi_cls_pool_tab_t *tab, const uint32_t have[MI_CLS_POOL_SLOTS],
				 const uint32_t base[MI_CLS_POOL_SLOTS], mi_cls_result_t *res_out_host,
				 uint32_t *dec_host, uint32_t *idx_host, mi_cls_pool_out_t *out_host,
				 uint64_t *ticket);
int mi_cls_pool_plan_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* ------------------------------------------------------------------------
 * The pool move: the steps of the reference's receive loop that touch packet
 * memory, for a batch the pool plan has decided: packet_parse_reset plus the
 * parse and classification result written into the header (pktio/loop.c:
 * 308-342) and the copy half of _odp_pktio_packet_to_pool (include/
 * odp_packet_io_internal.h:352-371).  With it the chain classify -> pool plan
 * -> pool move -> enqueue plan (or run plan) runs on one stream and the host
 * reads back ent[] and the counters.  The classifier is on, so the parser
 * layer is ALL: no layer cut.  Per record i, fate = dec[i] & 15:
 *   FRESH    the packet is got[idx[i]] (the address of its mi_cls_pkt_meta_t
 *            line).  All 64 bytes of the line are written: data_off =
 *            headroom, len, in_flags, err, cos, cls_mark, l2 = 0, l3, l4,
 *            input, every reserved word 0; dst_queue = dst_queue[id] when tab
 *            maps the record's (cos, queue) by the enqueue plan's "delivered"
 *            rule (outcome MI_CLS_OUT_ENQ, queue < cos_nq[cos], cos_q0[cos] +
 *            queue < MI_CLS_ENQ_ENT, the entry's id < ndst), else 0; user_ptr
 *            = that of pk[i]'s line when pk is given and pk[i] != 0 (what
 *            odp_packet_copy carries), else 0.  The frame pkts[off[i] ..
 *            off[i] + len[i]) is copied to line + data_from_meta in 16-byte
 *            pieces: [0, len) is the frame, [len, round_up(len, 16)) is
 *            unspecified, nothing at or past that is touched; len 0 writes
 *            the line alone;
 *   INPLACE  the packet is pk[i].  The line is written the same way, but
 *            data_off and user_ptr keep the values read from it; no frame
 *            byte is written;
 *   other    ent[i] = 0, nothing else written.
 * ent[i] is the line's address of the packet that holds frame i afterwards,
 * or 0.  out: moved (FRESH records done), inplace (INPLACE records done),
 * bytes (the sum of len over the moved records) and refused.
 * Guards: no caller data can make the device touch memory outside pkts[0 ..
 * pkts_bytes) and [arena_lo, arena_lo + arena_bytes), the one range every
 * packet lies in.  A FRESH or INPLACE record is refused -- ent[i] = 0, nothing
 * of it written, counted in refused -- when
 *   its frame reaches past pkts_bytes (a frame needs [off, off + len) alone:
 *   no slack behind it);
 *   FRESH: idx[i] >= ngot; its packet's address is 0 or not 64-byte aligned;
 *   [line, line + data_from_meta + round_up(len, 16)) is not inside the arena;
 *   or pk[i] != 0 is not the address of a 64-byte line inside the arena;
 *   INPLACE: pk is NULL; pk[i] is 0 or not 64-byte aligned; [line, line + 64)
 *   is not inside the arena.
 * Two records that name one packet, a packet that overlaps pkts where a FRESH
 * record reads it, and arrays that overlap the arena's packets are undefined
 * behaviour (inside the two ranges).
 * Multi-GPU: there is no mi_cls_group_* form.
 * ---------------------------------------------------------------------- */
/* The kernel's shape: a wave takes tiles of MI_CLS_MOVE_TILE records (one per
 * lane), dealt statically over at most MI_CLS_MOVE_GRID blocks (of 4 waves:
 * wave w of W takes tiles w, w + W, ...); a tile's frames are copied in rounds
 * of at most MI_CLS_MOVE_ROUND bytes, whose loads are all issued before the
 * first store. */
#define MI_CLS_MOVE_TILE 64
#define MI_CLS_MOVE_GRID 512
#define MI_CLS_MOVE_ROUND 8192

typedef struct mi_cls_move_out {
	uint64_t moved, inplace, bytes, refused;
} mi_cls_move_out_t;

typedef struct mi_cls_move_args {
	const uint8_t *pkts;           /* the classification's frames ...               */
	uint64_t pkts_bytes;           /* ... their buffer's size, < 2^32 ...           */
	const uint32_t *off;           /* ... and arrays, at any alignment              */
	const uint16_t *len;
	const mi_cls_result_t *res;    /* the pool plan's res_out (16-byte aligned)     */
	const uint32_t *dec, *idx;     /* the pool plan's outputs                       */
	const uint64_t *got;           /* ngot line addresses of the packets taken, as
					* the pool plan's base / have lay them out      */
	const uint64_t *pk;            /* each frame's own packet's line, 0: none; NULL:
					* no frame has one (pcap-style frames)          */
	uint32_t n, ngot;
	const mi_cls_enq_tab_t *tab;   /* host memory, read during the call             */
	const uint64_t *dst_queue;     /* tab->ndst odp_queue_t by destination id; host
					* memory; part of the table: refreshed with it  */
	uint64_t input;                /* odp_pktio_t                                   */
	uint32_t headroom;             /* data_off of a fresh packet                    */
	uint32_t data_from_meta;       /* bytes from a line to a fresh packet's data: a
					* multiple of 16, at least 64                   */
	uint64_t arena_lo, arena_bytes;
	uint64_t *ent;                 /* out: n line addresses                         */
	mi_cls_move_out_t *out;        /* out (8-byte aligned)                          */
} mi_cls_move_args_t;

/* Move n records in device memory (or host memory the device addresses).  ent
 * and out are written whole, no input value of theirs is read.  args, tab and
 * dst_queue are host memory, read during the call; the table's device copy is
 * refreshed when tab's address or stamp differs from the last call's.  The
 * context needs no rules.  Stream-ordered on `stream`; returns after the
 * launches are enqueued; a call on another stream than the previous move's is
 * ordered after it.  n == 0: out is zeroed (the arrays may be NULL).
 * -EINVAL: NULL args, table, dst_queue (with ndst > 0), out or (n > 0) array
 * other than pk; got NULL with ngot > 0; a misaligned res (16), ent, got, pk or
 * out (8); data_from_meta below 64 or no multiple of 16; n > MI_CLS_MAX_BATCH;
 * pkts_bytes >= 2^32; arena_lo + arena_bytes past 2^64; a NULL context where
 * there is a device.  -E2BIG: tab->ndst > MI_CLS_ENQ_DST_MAX.  -ENODEV: no
 * device.  mi_cls_last_launch: info[0] 320 + the waves per block (324), [1]
 * the launches (2; 1 for n == 0), [2]-[5] 0, [6] the grid. */
int mi_cls_pool_move(mi_cls_ctx_t *ctx, const mi_cls_move_args_t *args, void *stream);

/* Host-memory batch, as mi_cls_pool_plan_host and its submit / wait forms.
 * The packets are always worked on in place: -EINVAL unless
 * mi_cls_host_mapped holds for both ends of the arena.  pkts, off, len, res,
 * dec, idx, got, pk (if given), ent and out all page-locked: read and written
 * in place; otherwise the frames, off, len, res, dec, idx, got and pk go
 * through the context's staging buffers and ent and out are copied back. */
int mi_cls_pool_move_host(mi_cls_ctx_t *ctx, const mi_cls_move_args_t *args);
int mi_cls_pool_move_host_submit(mi_cls_ctx_t *ctx, const mi_cls_move_args_t *args, uint64_t *ticket);
int mi_cls_pool_move_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* ------------------------------------------------------------------------
 * The vector fill: the host half of the reference's _odp_cos_vector_enq
 * (include/odp_classification_internal.h:83-137) for a batch the run plan has
 * cut: every run's event array, ready for one odp_queue_enq_multi, and the
 * packet vectors of the runs that have some, filled.  With it the chain
 * classify -> pool plan -> pool move -> run plan -> vector fill runs on one
 * stream; nruns and the delivered count are read on the device from the run
 * plan's out, so there is no host round trip between the plan and the fill.
 * Inputs: the run plan's seq[n], runs[run_cap] and out, the pool move's ent[n],
 * the vectors taken for the batch (vgot[nvgot], slot s's at vbase[s] ..
 * vbase[s] + vhave[s]) and the run table.
 *   handle       hnd(i) = ent[i] - ent_to_handle when ent[i] != 0, else 0
 *                (ent_to_handle: the distance from a packet handle to its
 *                metadata line).  A delivered record whose ent is 0 is one the
 *                move refused: it is written as handle 0 wherever it lands,
 *                and every handle 0 written to ev, a table or lost is counted
 *                in holes.
 * Per run r < nruns, in run order, with s = vslot[cos], vm = vmax[cos],
 * rank_s(r) = the sum of nvec over the earlier MI_CLS_RUN_VEC runs of slot s,
 * ev_first(r) = the sum over the earlier runs of (count for a plain run, nvec
 * for a vector run): ev needs at most n entries and no entry's place depends
 * on a pool running short:
 *   plain run    (flags has no MI_CLS_RUN_VEC) its events are its packets:
 *                ev[ev_first + o] = hnd(seq[first + o]) for o < count;
 *                ev_count = pk_enq = count;
 *   vector run   it gets g = clamp(vhave[s] - rank_s(r), 0, nvec) vectors,
 *                vgot[vbase[s] + rank_s(r) + k] for k < g: the reference's
 *                allocate-until-it-fails loop under "no vector returns to a
 *                pool during the batch" (the pool plan's assumption): the run
 *                at which a pool runs out gets what is left, later runs of the
 *                pool none.  Vector k: size = min(vm, count - k * vm), tbl[j] =
 *                hnd(seq[first + k * vm + j]); ev[ev_first + k] = the vector
 *                (its vgot value) for k < g, 0 for g <= k < nvec; ev_count =
 *                g; pk_enq = min(count, g * vm).  The packets seq[first +
 *                pk_enq .. first + count) are lost: their handles are appended
 *                to lost[] in no specified order (a free list; the reference
 *                leaks them).  They reach no queue: queue discards.
 * evr[r] = { ev_first, ev_count, pk_enq, vfirst }, vfirst the index in vgot of
 * the run's first vector, 0xFFFFFFFF for a plain run or g == 0; written for
 * r < nruns only.  ev is written in [0, ev_span) only, lost in [0, out->lost).
 * out: events (ev_count summed), ev_span (the event places: ev_first + its
 * share of the last run), vectors (filled), in_vectors (the packets in them),
 * lost, holes, refused, truncated, vec_used[s] = min(the slot's nvec sum,
 * vhave[s]): the vectors from vbase[s] + vec_used[s] on go back to the pool.
 * out->nruns > run_cap of the run plan: the plan was truncated, and the fill
 * writes nothing but its own out: truncated = 1, every other field 0.
 * Guards: no caller data can make the device touch memory outside the arrays
 * and [varena_lo, varena_lo + varena_bytes), the one range every vector lies
 * in.  A vector is refused -- nothing of it written, its ev entry 0, counted
 * in refused; its packets stay reachable through ent and are in no count --
 * when its index is >= nvgot, its address is 0 or not 8-byte aligned, or [v, v
 * + tbl_off + 8 * size) is not inside the arena.  seq values are checked
 * against n before use, first + count is clamped to min(out->delivered, n),
 * and an ev or lost place at or past n is not written.  ev, evr and lost must
 * not alias the inputs; vectors that overlap each other or the arrays are
 * undefined behaviour (inside the ranges).
 * Multi-GPU: there is no mi_cls_group_* form.  A shard's ranks start at zero,
 * so the caller gives each shard its own vhave / vbase (its part of the
 * vectors).
 * ---------------------------------------------------------------------- */
/* The kernels' shape: a block of 16 waves walks a contiguous run of tiles of
 * MI_CLS_VEC_TILE runs (count, place) or delivered places (fill); at most
 * MI_CLS_VEC_GRID blocks (grid = min(MI_CLS_VEC_GRID, tiles)). */
#define MI_CLS_VEC_TILE 1024
#define MI_CLS_VEC_GRID 256

typedef struct mi_cls_evrun {
	uint32_t ev_first;             /* the run's first place in ev                   */
	uint32_t ev_count;             /* events to enqueue from there                  */
	uint32_t pk_enq;               /* packets they carry; count - pk_enq are lost   */
	uint32_t vfirst;               /* index in vgot of its first vector, 0xFFFFFFFF */
} mi_cls_evrun_t;

typedef struct mi_cls_vec_out {
	uint64_t events, ev_span, vectors, in_vectors, lost, holes, refused, truncated;
	uint64_t vec_used[MI_CLS_RUN_VSLOTS];
} mi_cls_vec_out_t;

typedef struct mi_cls_vec_args {
	const uint32_t *seq;           /* the run plan's seq[n] ...                     */
	const mi_cls_run_t *runs;      /* ... runs[run_cap] (16-byte aligned) ...       */
	const mi_cls_run_out_t *run_out; /* ... and out, read on the device             */
	const uint64_t *ent;           /* the pool move's ent[n]                        */
	const uint64_t *vgot;          /* nvgot vector handles (their addresses)        */
	uint32_t n, run_cap, nvgot;
	uint32_t size_off, tbl_off;    /* a vector's size word and table, from its handle */
	uint32_t rsv;
	uint64_t ent_to_handle;
	const mi_cls_run_tab_t *rtab;  /* host memory, read during the call             */
	uint32_t vbase[MI_CLS_RUN_VSLOTS], vhave[MI_CLS_RUN_VSLOTS];
	uint32_t vcap[MI_CLS_RUN_VSLOTS];   /* each slot's pool's max_size              */
	uint64_t varena_lo, varena_bytes;
	uint64_t *ev;                  /* out: n entries                                */
	mi_cls_evrun_t *evr;           /* out: run_cap entries (16-byte aligned)        */
	uint64_t *lost;                /* out: n entries                                */
	mi_cls_vec_out_t *out;         /* out (8-byte aligned)                          */
} mi_cls_vec_args_t;

/* Fill the vectors and event arrays of a planned batch in device memory (or
 * host memory the device addresses).  ev[0 .. ev_span), evr[0 .. nruns),
 * lost[0 .. out->lost) and out are written whole, no input value of theirs is
 * read and nothing past those ends is touched.  args and rtab are host memory,
 * read during the call; the run table's device copy is refreshed when rtab's
 * address or stamp differs from the last call's, and the fixed scratch is the
 * context's (16 B per run of run_cap more, grown by 1.5x and kept).  The
 * context needs no rules.  Stream-ordered on `stream`; returns after the
 * launches are enqueued; a call on another stream than the previous fill's is
 * ordered after it by an event.  n == 0: out is zeroed (the arrays may be
 * NULL).  -EINVAL: NULL args, table, out or (n > 0) array (runs and evr may be
 * NULL when run_cap == 0, vgot when nvgot == 0); a misaligned runs or evr
 * (16), ent, vgot, ev, lost or out (8); size_off no multiple of 4 or size_off
 * + 4 > tbl_off; tbl_off no multiple of 8; a MI_CLS_RUN_VEC CoS whose vmax is
 * 0 or exceeds vcap[vslot] or whose vslot is >= MI_CLS_RUN_VSLOTS; vbase[s] +
 * vhave[s] past nvgot; varena_lo + varena_bytes past 2^64; n >
 * MI_CLS_MAX_BATCH; a NULL context where there is a device.  -ENODEV: no
 * device.  mi_cls_last_launch: info[0] 384 + the waves per block (400), [1]
 * the launches (4; 1 for n == 0), [2]-[5] 0, [6] the grid of the fill launch. */
int mi_cls_vec_fill(mi_cls_ctx_t *ctx, const mi_cls_vec_args_t *args, void *stream);

/* Host-memory batch, as mi_cls_pool_move_host and its submit / wait forms.
 * The vectors are always worked on in place: -EINVAL unless
 * mi_cls_host_mapped holds for both ends of the vector arena (n > 0).  seq,
 * runs, run_out, ent, vgot, ev, evr, lost and out all page-locked: read and
 * written in place; otherwise seq, runs, run_out, ent and vgot are staged up
 * and ev, evr, lost and out are copied back (ev, evr and lost go up first, so
 * that the entries the fill leaves alone come back as they were). */
int mi_cls_vec_fill_host(mi_cls_ctx_t *ctx, const mi_cls_vec_args_t *args);
int mi_cls_vec_fill_host_submit(mi_cls_ctx_t *ctx, const mi_cls_vec_args_t *args, uint64_t *ticket);
int mi_cls_vec_fill_host_wait(mi_cls_ctx_t *ctx, uint64_t ticket);

/* 1 if p lies in page-locked host memory that the device addresses at the
 * same address (the receive delivery's requirement), else 0. */
int mi_cls_host_mapped(const void *p);

/* Pinned (page-locked) host memory for staging; NULL on failure. */
void *mi_cls_host_alloc(size_t bytes);
void mi_cls_host_free(void *p);

/* Per-CoS packet counters with the reference's per-hop counting rule
 * (odp_classification.c:1646-1647, 1721-1723): when enabled, each
 * mi_cls_classify() adds into a device array of num_cos uint64 counters
 * for CoS slots whose stats are enabled (stats_mask bit per slot, up to 256).
 * mi_cls_stats_read copies the counters to host memory (synchronous). */
int mi_cls_stats_enable(mi_cls_ctx_t *ctx, const uint32_t stats_mask[8]);
int mi_cls_stats_read(mi_cls_ctx_t *ctx, uint64_t *host_counters, uint32_t num);
int mi_cls_stats_reset(mi_cls_ctx_t *ctx);

/* Host-only (no device needed): assemble a compiled table into the private
 * device encoding and describe it.  info[0] total 32-bit words, [1] words of
 * the per-lane "hot" region (copied to LDS when it fits), [2] CoS with a
 * classification block, [3..6] blocks per engine (direct, candidate,
 * bitmap, wide bitmap), [7] 1 if some rule leads to a CoS with rules,
 * [8] single-candidate blocks, [9] (when n >= 10) 0 if the program is not
 * flat (decided on the default CoS in one round), else its engine + 1,
 * [10] (n >= 11) CoS whose rules need a chain of blocks (more key classes
 * than one block holds; [2..8] count their first blocks).
 * n >= 9.  Used by tests and tools to check engine selection on the CPU. */
int mi_cls_program_info(const void *tbl, size_t bytes, uint32_t *info, uint32_t n);

/* Last error string for the context (static storage, never NULL). */
const char *mi_cls_strerror(int err);

#ifdef __cplusplus
}
#endif

#endif /* MI_CLS_H_ */
