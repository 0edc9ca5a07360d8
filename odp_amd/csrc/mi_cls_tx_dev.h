// mi_cls_tx_dev.h -- device side of the pktout checksum insertion
// (mi_cls_chksum_insert, include/mi_cls.h): the IPv4 header checksum, the
// UDP / TCP checksums and the SCTP CRC-32C written into the frames of a batch
// on transmit.
//
// What it replaces (reference, platform/linux-generic/):
//   pktio/loop.c:386-472     check_proto / loopback_fix_checksums (the decision)
//   odp_packet.c:1888-2063   _odp_packet_{ipv4,udp,tcp,sctp}_chksum_insert
// Deviation: the TCP checksum is stored at l4 + 16 (the reference stores it
// at l4 + _ODP_UDP_CSUM_OFFSET = l4 + 6, odp_packet.c:1988).
//
// Shape: as the receive kernels, one wavefront per 64-packet tile, one packet
// per lane, persistent waves over the tiles -- without their parse, window
// staging and rule program: the L3 / L4 offsets come with the packet
// (mi_cls_tx_desc_t; the reference does not re-parse on transmit).  The IPv4
// header sum is per lane (at most 15 dwords); the UDP / TCP range sums and
// the SCTP CRCs are the receive side's wave-cooperative ck_sum_wave /
// sctp_crc_wave (pieces of all 64 frames dealt 64 per round), frames too long
// for the cooperative CRC take its one-lane form (sctp_crc).
#pragma once
#include "mi_cls_dev.h"

#define TX_OPT_IPV4 (1u << 4)   // odp_pktout_config_opt_t.all_bits: <proto>_chksum
#define TX_OPT_UDP (1u << 5)
#define TX_OPT_TCP (1u << 6)
#define TX_OPT_SCTP (1u << 7)
#define TX_L3_SET 1u        // mi_cls_tx_desc_t.flags
#define TX_L3_CK 2u
#define TX_L4_SET 4u
#define TX_L4_CK 8u
#define TX_OFF_INVALID 0xFFFFu

// Frame bytes by batch offset (any alignment, which gfx950 serves); a false
// predicate reads nothing and gives 0.
__device__ __forceinline__ uint32_t tx_ld32(__amdgpu_buffer_rsrc_t rs, uint32_t o, bool ok)
{
	return __builtin_amdgcn_raw_buffer_load_b32(rs, ok ? o : OOB_OFF, 0, 0);
}

__device__ __forceinline__ uint32_t tx_ld16(__amdgpu_buffer_rsrc_t rs, uint32_t o, bool ok)
{
	return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rs, ok ? o : OOB_OFF, 0, 0) & 0xffffu;
}

__device__ __forceinline__ uint32_t tx_ld8(__amdgpu_buffer_rsrc_t rs, uint32_t o, bool ok)
{
	return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, ok ? o : OOB_OFF, 0, 0) & 0xffu;
}

// All sums are of the 16-bit words as the little-endian loads give them
// (as on the receive side): a word's value is stored back low byte first.
// Words are paired from l3 / l4 (l4 - l3 is even: one parity for the IP
// header, the pseudo header and the L4 range), which may be odd frame
// offsets: ck_sum_wave pairs bytes from even frame offsets, so for an odd l4
// it sums [l4 + 1, len), the byte at l4 joins as the high half of the word
// below it, and the folded sum is byte-swapped (RFC 1071 section 2(B): the
// sum of the byte-swapped words is the byte-swapped sum).
__global__ __launch_bounds__(TX_NW * WAVE) void mi_cls_tx_kernel(TxArgs a)
{
	// CRC-32C slicing tables and piece shifts
	__shared__ uint32_t s_crc[CRC_WORDS];

	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint32_t wave = threadIdx.x >> 6;
	{
		const uint32_t *cw = reinterpret_cast<const uint32_t *>(&c_crc32c);
		for (uint32_t i = threadIdx.x; i < CRC_WORDS; i += TX_NW * WAVE)
			s_crc[i] = cw[i];
	}
	__syncthreads();
	const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
		(void *)a.pkts, (short)0, (int)OOB_OFF, 0x00020000);
	const uint32_t nt = (a.n + WAVE - 1) / WAVE;
	const uint32_t opt = a.opt;

	for (uint32_t tile = blockIdx.x * TX_NW + wave; tile < nt; tile += gridDim.x * TX_NW) {
		const uint32_t pi = tile * WAVE + lane;
		const bool valid = pi < a.n;
		uint32_t off = 0, len = 0, l3 = TX_OFF_INVALID, l4 = TX_OFF_INVALID, fl = 0;
		if (valid) {
			off = ld_desc(a.off + pi);
			len = ld_desc(a.len + pi);
			const uint2 d = *reinterpret_cast<const uint2 *>(a.desc + pi);
			l3 = d.x & 0xffffu;
			l4 = d.x >> 16;
			fl = d.y & 0xffu;
		}
		// ---- every per-lane header load of the tile in one batch, none
		// depending on another's data (one memory round trip, not one per
		// step): the L3 header's dwords 0-9 that lie in the frame (the IPv4
		// header without long options / the IPv6 header: version, IHL,
		// fragment word, protocol, addresses), and from l4 the UDP length and
		// checksum words, the TCP checksum word and the first byte of an odd
		// l4 -- each only where the frame holds it, whatever the protocol
		// turns out to be
		const bool l3ok = valid && l3 != TX_OFF_INVALID && l3 < len;
		const uint32_t rem = l3ok ? len - l3 : 0u;
		uint32_t h[10];
#pragma unroll
		for (uint32_t i = 0; i < 10u; ++i)
			h[i] = tx_ld32(rs, off + l3 + 4u * i, rem >= 20u && rem >= 4u * i + 4u);
		const bool l4in = valid && l4 != TX_OFF_INVALID;
		const uint32_t odd = l4 & 1u;
		const uint32_t q1 = tx_ld32(rs, off + l4 + 4u, l4in && l4 + 8u <= len);     // UDP length, checksum
		const uint32_t q2 = tx_ld16(rs, off + l4 + 16u, l4in && l4 + 18u <= len);  // TCP checksum
		const uint32_t hb = tx_ld8(rs, off + l4, l4in && odd != 0u && l4 < len) << 8;

		// ---- the decision (loop.c:389-472)
		const uint32_t ver = (h[0] >> 4) & 15u, ihl = h[0] & 15u;
		const bool v4 = ver == 4u && rem >= 20u, v6 = ver == 6u && rem >= 40u;
		// IPv4: protocol, 255 for a fragment (MF or offset); IPv6: next header
		// (no extension-header walk, as the reference)
		const uint32_t proto = v4 ? ((bsw16(h[1] >> 16) & 0x3fffu) ? 255u : (h[2] >> 8) & 0xffu)
					  : (h[1] >> 16) & 0xffu;
		const bool w_ip = v4 && ((fl & TX_L3_SET) ? (fl & TX_L3_CK) != 0u : (opt & TX_OPT_IPV4) != 0u);
		const uint32_t pk = proto == 17u ? 1u : (proto == 6u ? 2u : (proto == 132u ? 3u : 0u));
		const uint32_t cfg = pk == 1u ? TX_OPT_UDP : (pk == 2u ? TX_OPT_TCP : TX_OPT_SCTP);
		const bool w_l4 = (v4 || v6) && pk != 0u &&
				  ((fl & TX_L4_SET) ? (fl & TX_L4_CK) != 0u : (opt & cfg) != 0u);
		// the contract: l4 valid, l4 - l3 even and at least the fixed IP
		// header, the checksum field inside the frame; else nothing is written
		const uint32_t fo = l4 + (pk == 1u ? 6u : (pk == 2u ? 16u : 8u));   // the field
		const bool l4ok = l4 != TX_OFF_INVALID && l4 >= l3 + (v4 ? 20u : 40u) && ((l4 - l3) & 1u) == 0u &&
				  fo + (pk == 3u ? 4u : 2u) <= len;
		const uint32_t kind = (w_l4 && l4ok) ? pk : 0u;

		// ---- IPv4 header (odp_packet.c:1888-1949), per lane: dwords 0-9
		// are loaded (l3 + 4 IHL <= len: every dword below IHL is in the
		// frame), options past them are rare
		const bool ipdo = w_ip && ihl >= 5u && l3 + 4u * ihl <= len;
		uint32_t ipck = 0;
		{
			uint64_t s = 0;
#pragma unroll
			for (uint32_t i = 0; i < 10u; ++i)   // dword 2: the field taken as zero
				s += i < ihl ? (i == 2u ? (h[i] & 0xffffu) : h[i]) : 0u;
			if (__ballot(ipdo && ihl > 10u) != 0ull) {
#pragma unroll
				for (uint32_t i = 10; i < 15u; ++i)
					s += tx_ld32(rs, off + l3 + 4u * i, ipdo && i < ihl);
			}
			ipck = ~ck_finalize(s) & 0xffffu;
		}

		// ---- UDP / TCP (odp_packet.c:1951-2013)
		const bool sum = kind == 1u || kind == 2u;
		uint32_t l4ck = 0;
		if (__ballot(sum) != 0ull) {
			uint64_t s = 0;
			uint32_t cnt = 0, base = 0, prm = 0;
			if (sum) {
				// the addresses as stored: 8 bytes at l3 + 12 / 32 bytes at l3 + 8
				s = (uint64_t)h[3] + h[4];
				if (!v4)
					s += (uint64_t)h[2] + h[5] + h[6] + h[7] + h[8] + h[9];
				// UDP: the length field as stored; TCP: frame_len - l4, big-endian
				s += kind == 1u ? (q1 & 0xffffu) + (17u << 8) : bsw16(len - l4) + (6u << 8);
				s += 0xffffu - (kind == 1u ? q1 >> 16 : q2);   // the old field out of the range sum
				const uint32_t from = l4 + odd, p0 = from & ~63u;
				cnt = (len - p0 + 63u) >> 6;
				base = off + p0;
				prm = (from - p0) | ((len - p0) << 6);
			}
			const uint32_t r = ck_sum_wave(rs, base, prm, cnt, lane);
			const uint32_t d = ck_finalize((uint64_t)r + hb);
			s += odd ? bsw16(d) : d;
			l4ck = ~ck_finalize(s) & 0xffffu;
			l4ck = (kind == 1u && l4ck == 0u) ? 0xffffu : l4ck;
		}

		// ---- SCTP (odp_packet.c:2049-2063)
		uint32_t crc = 0;
		if (__ballot(kind == 3u) != 0ull) {
			// frames of fewer than CRC_ZN 64-B blocks: the wave cooperates;
			// longer ones: one lane walks its frame
			const bool wv = kind == 3u && len <= 64u * (CRC_ZN - 1u);
			crc = sctp_crc_wave<false>(rs, nullptr, off, wv ? l4 : 0u, wv ? len : 0u, wv ? 1u : 0u,
						   lane, s_crc);
			if (__ballot(kind == 3u && !wv) != 0ull) {
				if (kind == 3u && !wv) {
					const Pkt k = { nullptr, a.pkts + off, len, 0u };
					crc = sctp_crc(k, rs, off, l4, s_crc);
				}
			}
		}

		// ---- the tile's stores, after its last load has returned (lanes
		// read each other's frames in the cooperative sums)
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		uint8_t *p = a.pkts + off;
		if (ipdo) {
			p[l3 + 10u] = (uint8_t)ipck;
			p[l3 + 11u] = (uint8_t)(ipck >> 8);
		}
		if (sum) {
			p[fo] = (uint8_t)l4ck;
			p[fo + 1u] = (uint8_t)(l4ck >> 8);
		}
		if (kind == 3u) {
			p[fo] = (uint8_t)crc;
			p[fo + 1u] = (uint8_t)(crc >> 8);
			p[fo + 2u] = (uint8_t)(crc >> 16);
			p[fo + 3u] = (uint8_t)(crc >> 24);
		}
		if (a.done != nullptr && valid)
			a.done[pi] = (uint8_t)((ipdo ? MI_CLS_TX_IPV4 : 0u) |
					       (kind == 1u ? MI_CLS_TX_UDP : kind == 2u ? MI_CLS_TX_TCP
						: kind == 3u ? MI_CLS_TX_SCTP : 0u));
	}
}
