// mi_cls_parse_dev.h -- device side of mi_cls_parse (include/mi_cls.h): the
// parse of a batch on its own, without a rule program -- odp_packet_parse()
// for packets that did not come from a pktio.
//
// What it replaces (reference, platform/linux-generic/):
//   odp_packet.c:2140-2229   odp_packet_parse / odp_packet_parse_multi
//   odp_parse.c:23-105       _odp_parse_eth (start protocol ETH only)
//   odp_parse.c:362-488      _odp_packet_parse_common_l3_l4 with its `layer`
//                            returns (:372-375 L2, :412 L3)
//   odp_packet.c:2065-2138   _odp_packet_l4_chksum (layer >= L4)
//
// Shape: the receive kernels' -- one wavefront per 64-packet tile, one packet
// per lane, 4-wave blocks of persistent waves striding over the tiles, the
// next tile's header windows in flight while this one is parsed -- without
// their rule program, descent, statistics and hot region.  The helpers are
// mi_cls_dev.h's: load_window / store_window / zero_tail stage the first 64
// (96) bytes of every frame in the wave's dword-major LDS window, parse_fast
// parses the lanes it covers and parse_packet the rest, l4_chksum runs the
// wave-cooperative sums and CRCs.
//
// Per launch (wave-uniform): the start protocol (template START), the last
// layer and the checksum selection (ParseArgs).  The caller folds a packet's
// parse offset into its descriptor (off = the byte parsing starts at, len =
// frame_len - offset: everything in odp_parse.c is relative to that), so
// parse starts have any alignment.
//   START ETH: parse_fast, whose L3 at 2 (mod 4) is relative to the parse
//   start, not to memory, so it holds at any offset.
//   START IPV4 / IPV6: every lane takes parse_packet<START> (L3 at byte 0 of
//   the window; parse_fast's selects are built on Ethernet's layouts).
//   Layer: the parse runs whole and the record keeps what the reference has
//   set at its return for the layer (flags and error bits by the step that
//   sets them, l4 invalid at L2); below L4 no wave enters the checksum
//   rounds, and the host picks the instantiation without checksum code when
//   the layer leaves none of the selection to do.
#pragma once
#include "mi_cls_dev.h"

// input_flags / error bits by the parser step that sets them
// (_odp_parse_eth; parse_ipv4 / parse_ipv6 and the L3 switch)
#define PRS_L2_FLAGS (F_L2 | F_ETH | F_ETH_BCAST | F_ETH_MCAST | F_JUMBO | F_VLAN | F_QINQ)
#define PRS_L3_FLAGS (PRS_L2_FLAGS | F_L3 | F_ARP | F_IPV4 | F_IPV6 | F_IP_BCAST | F_IP_MCAST | \
		      F_IPFRAG | F_IPOPT | F_L3CK_DONE)
#define PRS_L2_ERR E_SNAP
#define PRS_L3_ERR (E_SNAP | E_IP | E_L3CK)

template <uint32_t START, bool CK>
__global__ __launch_bounds__(PRS_NW * WAVE, MIN_WAVES_PER_EU) void mi_cls_parse_kernel(ParseArgs a)
{
	__shared__ uint32_t s_win[PRS_NW * RS * WROWS];
	__shared__ uint32_t s_l4[256];
	// CRC-32C slicing tables and piece shifts (checksum selections)
	__shared__ uint32_t s_crc[CK ? CRC_WORDS : 1];

	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint32_t wave = threadIdx.x >> 6;
	uint32_t *W = s_win + wave * RS * WROWS;
	const uint32_t nt = (a.n + WAVE - 1) / WAVE;
	// tiles of this wave: blockIdx.x + G (wave + PRS_NW i), i = 0, 1, ..: the
	// grid's tiles in flight are one contiguous stretch of the batch
	const uint32_t t0 = blockIdx.x + gridDim.x * wave, stride = gridDim.x * PRS_NW;
	const uint32_t layer = a.layer;
	const uint32_t opt = CK ? a.opt : 0u;

	uint32_t tile = t0, nx = t0 + stride;
	uint32_t d_off = 0, d_len = 0, n_off = 0, n_len = 0;
	{
		const uint32_t p0 = tile * WAVE + lane, p1 = nx * WAVE + lane;
		if (tile < nt && p0 < a.n) {
			d_off = ld_desc(a.off + p0);
			d_len = ld_desc(a.len + p0);
		}
		if (nx < nt && p1 < a.n) {
			n_off = ld_desc(a.off + p1);
			n_len = ld_desc(a.len + p1);
		}
	}
	const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
		(void *)a.pkts, (short)0, (int)OOB_OFF, 0x00020000);
	u32x4 d[NPIECE];
	bool d_hi = false, hi_rows = true;
	// window predictor (as mi_cls_kernel's): bytes 64..WIN-1 of long frames
	// are staged only while the last parsed tile's headers reached past byte
	// 64; the first tile stages them
	bool want_hi = true;
	uint32_t d_win = WIN;
	if (tile < nt)
		d_hi = load_window(rs, d_off, d_len, lane, d, want_hi, d_win);
	for (uint32_t i = threadIdx.x; i < 256u; i += PRS_NW * WAVE)
		s_l4[i] = c_l4tab.v[i];
	if constexpr (CK) {
		const uint32_t *cw = reinterpret_cast<const uint32_t *>(&c_crc32c);
		for (uint32_t i = threadIdx.x; i < CRC_WORDS; i += PRS_NW * WAVE)
			s_crc[i] = cw[i];
	}
	for (uint32_t r = WIN / 4; r < WROWS; ++r)
		W[r * RS + lane] = 0u;   // pad / zero rows: always zero
	__syncthreads();

	uint4 prev_rec = make_uint4(0, 0, 0, 0);
	uint32_t prev_pi = 0;
	bool prev_valid = false;
	for (; tile < nt; tile = nx, nx += stride) {
		const uint32_t pi = tile * WAVE + lane;
		const bool valid = pi < a.n;
		const uint32_t my_off = d_off, my_len = d_len, my_win = d_win;

		wave_lds_sync();   // previous tile's window reads are done
		store_window(W, lane, d, d_hi, hi_rows);
		zero_tail(W, lane, my_len);
		// previous tile's records before this tile's prefetch: the next wait
		// for window data never waits behind a younger store
		if (prev_valid)
			store_rec(a.out + prev_pi, prev_rec);
		prev_valid = false;
		// the next tile's windows, the descriptors of the one after it
		// (mi_cls_kernel's raised wave priority around these loads measured
		// no change here: 23.30 -> 23.26 us on config 3, box noise)
		{
			d_off = n_off;
			d_len = n_len;
			const uint32_t nn = nx + stride, p2 = nn * WAVE + lane;
			n_off = 0;
			n_len = 0;
			if (nx < nt && nn < nt && p2 < a.n) {
				n_off = ld_desc(a.off + p2);
				n_len = ld_desc(a.len + p2);
			}
			if (nx < nt)
				d_hi = load_window(rs, d_off, d_len, lane, d, want_hi, d_win);
		}
		wave_lds_sync();

		Pkt k;
		k.w = W + lane;
		k.g = a.pkts + my_off;
		k.len = my_len;
		k.win = my_win;

		Parsed p;
		if constexpr (START != MI_CLS_PROTO_ETH) {
			p = parse_packet<START>(k, opt);
		} else {
			bool slow, dfr;
			p = parse_fast(k, s_l4, slow, 0u, dfr);
			p.udp_zero = 0;
			if constexpr (CK) {
				// as the pktin-option kernel (mi_cls_kernel, CK): the fast
				// parse stands for the lanes the selection does not change
				slow = slow || p.err != 0u;
				if (opt & OPT_IPV4_CK) {
					const bool v4 = !slow && (p.flags & F_IPV4) != 0u;
					if (__ballot(v4) != 0ull) {
						if (v4) {
							const uint32_t ihl = rb(k, p.l3) & 0xfu;
							uint64_t sum = 0;
							for (uint32_t i = 0; i < ihl; ++i)
								sum += r32(k, p.l3 + 4u * i);
							if (ck_finalize(sum) != 0xffffu)
								slow = true;
							else
								p.flags |= F_L3CK_DONE;
						}
					}
				}
				if (opt & OPT_UDP_CK) {
					const bool u = !slow && (p.flags & F_UDP) != 0u && !(p.flags & F_IPFRAG) &&
						       p.ret == 0;
					if (__ballot(u) != 0ull) {
						if (u && r16(k, p.l4 + 6u) == 0u)
							slow = true;
					}
				}
			}
			if (__ballot(slow) != 0ull) {
				if (slow)
					p = parse_packet(k, opt);
			}
		}
		if constexpr (CK) {
			// _odp_packet_l4_chksum: layer >= L4 only (odp_packet.c:2210)
			if ((opt & OPT_L4_CK) && layer >= MI_CLS_LAYER_L4)
				l4_chksum(k, p, opt, rs, my_off, lane, valid, s_crc);
		}
		{
			const uint32_t l4h = (p.flags & F_TCP) ? 13u : ((p.flags & F_UDP) ? 6u : 0u);
			uint32_t need = p.l3 != 0xFFFFu ? p.l3 + ((p.flags & F_IPV6) ? 40u : 20u) : 0u;
			need = max(need, p.l4 != 0xFFFFu ? p.l4 + l4h : 0u);
			want_hi = __ballot(valid && my_len > 64u && need > 64u) != 0ull;
		}

		// ---- the layer cut (odp_parse.c:372-375, :412) and the return value
		// (odp_packet.c:2207-2216): -1 on any error bit left, or on a
		// truncated L4 header at layer >= L4 (no error bit)
		uint32_t fl = p.flags, er = p.err, l4 = p.l4;
		bool fail;
		if (layer >= MI_CLS_LAYER_L4) {
			fail = p.ret != 0;
		} else {
			fl &= layer == MI_CLS_LAYER_L2 ? PRS_L2_FLAGS : PRS_L3_FLAGS;
			er &= layer == MI_CLS_LAYER_L2 ? PRS_L2_ERR : PRS_L3_ERR;
			l4 = layer == MI_CLS_LAYER_L2 ? 0xFFFFu : l4;
			fail = er != 0u;
		}
		const uint32_t outcome = fail ? MI_CLS_OUT_PARSE_DROP : MI_CLS_OUT_ENQ;
		prev_rec.x = fl;
		prev_rec.y = (er & 0xffu) | (outcome << 8);
		prev_rec.z = 0u;
		prev_rec.w = (p.l3 & 0xffffu) | ((l4 & 0xffffu) << 16);
		prev_pi = pi;
		prev_valid = valid;
	}
	if (prev_valid)
		store_rec(a.out + prev_pi, prev_rec);
}
