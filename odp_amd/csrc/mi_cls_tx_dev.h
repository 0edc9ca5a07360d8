// mi_cls_tx_dev.h -- device side of the pktout checksum insertion
// (mi_cls_chksum_insert, include/mi_cls.h): the IPv4 header checksum, the
// UDP / TCP checksums and the SCTP CRC-32C written into the frames of a batch
// on transmit -- and of the pktin flow hash of the loop pktio (mi_cls_tx_hash),
// a step of the same kernel.
//
// What it replaces (reference, platform/linux-generic/):
//   pktio/loop.c:386-472     check_proto / loopback_fix_checksums (the decision)
//   odp_packet.c:1888-2063   _odp_packet_{ipv4,udp,tcp,sctp}_chksum_insert
//   pktio/loop.c:479-530     get_dest_queue (the hash; the modulo is the caller's)
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

#define TX_OPT_IPV4 (1u << 4)   // odp_pktout_config_opt_t.all_bits >> 1: <proto>_chksum
#define TX_OPT_UDP (1u << 5)
#define TX_OPT_TCP (1u << 6)
#define TX_OPT_SCTP (1u << 7)
#define TX_L3_SET 1u        // mi_cls_tx_desc_t.flags
#define TX_L3_CK 2u
#define TX_L4_SET 4u
#define TX_L4_CK 8u
#define TX_OFF_INVALID 0xFFFFu
#define TX_HP_UDP (1u | 8u)     // odp_pktin_hash_proto_t.all_bits: ipv4_udp | ipv6_udp
#define TX_HP_TCP (2u | 16u)    // ipv4_tcp | ipv6_tcp
#define TX_HP_IPV4 4u
#define TX_HP_IPV6 32u

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

// What get_dest_queue (loop.c:479-530) appends for one packet, decided from
// the packet's metadata alone (flags, l3, l4, len; the frame is not parsed):
// the ports dword at l4, then the IPv4 addresses (2 dwords at l3 + 12) or the
// IPv6 addresses (8 dwords at l3 + 8).  A header that does not fit the frame
// appends nothing, and its `else if` is not tried.
struct TxHashSel {
	bool ports, a4, a6;
};

__device__ __forceinline__ TxHashSel tx_hash_sel(uint32_t hp, uint32_t fl, uint32_t len, uint32_t l3, uint32_t l4)
{
	const bool udp = (hp & TX_HP_UDP) != 0u && (fl & MI_CLS_TXF_UDP) != 0u;
	const bool tcp = (hp & TX_HP_TCP) != 0u && (fl & MI_CLS_TXF_TCP) != 0u;
	const bool ip4 = (hp & TX_HP_IPV4) != 0u && (fl & MI_CLS_TXF_IPV4) != 0u;
	const bool ip6 = (hp & TX_HP_IPV6) != 0u && (fl & MI_CLS_TXF_IPV6) != 0u;
	TxHashSel s;
	s.ports = l4 != TX_OFF_INVALID && (udp ? l4 + 8u <= len : (tcp && l4 + 20u <= len));
	s.a4 = l3 != TX_OFF_INVALID && ip4 && l3 + 20u <= len;
	s.a6 = l3 != TX_OFF_INVALID && !ip4 && ip6 && l3 + 40u <= len;
	return s;
}

// odp_hash_crc32c(string, n, 0) of that string (raw reflected CRC-32C, no
// final inversion; the empty string gives 0), per lane, one crc32c_u32 per
// appended dword: `ports` the dword at l4, h[2..9] the L3 header's dwords 2-9.
// The string is a sequence of selects over registers; the IPv6 words are
// skipped when no lane of the wave appends them.
__device__ __forceinline__ uint32_t tx_hash_crc(const uint32_t *tab, TxHashSel s, uint32_t ports,
						 const uint32_t (&h)[10])
{
	uint32_t crc = 0;
	{
		const uint32_t x = crc32c_u32(tab, crc, ports);
		crc = s.ports ? x : crc;
	}
	const bool l3 = s.a4 || s.a6;
#pragma unroll
	for (uint32_t k = 0; k < 2u; ++k) {
		const uint32_t x = crc32c_u32(tab, crc, s.a4 ? h[3u + k] : h[2u + k]);
		crc = l3 ? x : crc;
	}
	if (__ballot(s.a6) != 0ull) {
#pragma unroll
		for (uint32_t k = 2; k < 8u; ++k) {
			const uint32_t x = crc32c_u32(tab, crc, h[2u + k]);
			crc = s.a6 ? x : crc;
		}
	}
	return crc;
}

// HM: what the instantiation does per packet (A: TxArgs, or TxHashArgs for
// the two with the hash)
#define TX_M_CK 0u       // the checksums (mi_cls_chksum_insert)
#define TX_M_CK_HASH 1u  // the checksums and the flow hash, one launch
#define TX_M_HASH 2u     // the flow hash alone: no checksum code, no frame byte written

// All sums are of the 16-bit words as the little-endian loads give them
// (as on the receive side): a word's value is stored back low byte first.
// Words are paired from l3 / l4 (l4 - l3 is even: one parity for the IP
// header, the pseudo header and the L4 range), which may be odd frame
// offsets: ck_sum_wave pairs bytes from even frame offsets, so for an odd l4
// it sums [l4 + 1, len), the byte at l4 joins as the high half of the word
// below it, and the folded sum is byte-swapped (RFC 1071 section 2(B): the
// sum of the byte-swapped words is the byte-swapped sum).
template <uint32_t HM, typename A> __global__ __launch_bounds__(TX_NW * WAVE) void mi_cls_tx_kernel(A a)
{
	// CRC-32C slicing tables and piece shifts (the hash alone: the four
	// slicing tables only)
	constexpr uint32_t NTAB = HM == TX_M_HASH ? 1024u : CRC_WORDS;
	__shared__ uint32_t s_crc[NTAB];

	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint32_t wave = threadIdx.x >> 6;
	{
		const uint32_t *cw = reinterpret_cast<const uint32_t *>(&c_crc32c);
		for (uint32_t i = threadIdx.x; i < NTAB; i += TX_NW * WAVE)
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
		if constexpr (HM == TX_M_HASH) {
			// ---- the hash alone: only the dwords its string can hold
			// (the ports, the IPv4 addresses in L3 dwords 3-4 or the IPv6
			// addresses in 2-9), one batch of loads, one store per lane
			const TxHashSel hs = tx_hash_sel(a.hash_proto, fl, len, l3, l4);
			uint32_t h[10];
			h[0] = h[1] = 0;
#pragma unroll
			for (uint32_t i = 2; i < 10u; ++i)
				h[i] = tx_ld32(rs, off + l3 + 4u * i, hs.a6 || (hs.a4 && (i == 3u || i == 4u)));
			const uint32_t ports = tx_ld32(rs, off + l4, hs.ports);
			const uint32_t fh = tx_hash_crc(s_crc, hs, ports, h);
			if (valid)
				a.hash[pi] = fh;
			if (a.done != nullptr && valid)
				a.done[pi] = 0;
			(void)opt;
		} else {
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
			// the flow hash: its ports dword joins the batch (the addresses
			// are in h[]: a fitting IPv4 / IPv6 header has rem >= 20 / 40)
			TxHashSel hs = {};
			uint32_t ports = 0;
			if constexpr (HM == TX_M_CK_HASH) {
				hs = tx_hash_sel(a.hash_proto, fl, len, l3, l4);
				ports = tx_ld32(rs, off + l4, hs.ports);
			}

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

			// ---- the flow hash, of the frame as this launch leaves it: the
			// reference picks the queue after it fixed the checksums
			// (loop.c:581-582).  Metadata that contradicts the bytes can put a
			// checksum field into the string: the IPv4 header checksum (l3 + 10)
			// is the high half of L3 dword 2, the first IPv6 address word, or
			// any byte of a ports dword at an l4 inside the IP header; it is
			// known here, per lane, and goes into the words.  The L4 field
			// (step below) joins after it is computed.
			uint32_t fh = 0;
			if constexpr (HM == TX_M_CK_HASH) {
				uint32_t hh[10];
#pragma unroll
				for (uint32_t i = 0; i < 10u; ++i)
					hh[i] = h[i];
				hh[2] = ipdo ? (h[2] & 0xffffu) | (ipck << 16) : h[2];
				uint32_t pw = ports;
#pragma unroll
				for (uint32_t b = 0; b < 2u; ++b) {
					const uint32_t at = l3 + 10u + b - l4;   // byte of the ports dword
					const uint32_t m = 0xffu << (8u * (at & 3u));
					pw = ipdo && at < 4u ? (pw & ~m) | ((((ipck >> (8u * b)) & 0xffu) << (8u * (at & 3u)))) : pw;
				}
				fh = tx_hash_crc(s_crc, hs, pw, hh);
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

			// ---- the flow hash where the L4 checksum field lies in its string:
			// only has_ipv6 on an IPv4 frame (the 32 bytes from l3 + 8 reach
			// past the IPv4 header; l4 >= l3 + 20, so the ports dword and the
			// IPv4 addresses never hold the field).  The raw CRC from 0 is
			// linear: the hash of the patched string is the hash above xor the
			// CRC of (old field xor new field) followed by the zeros up to the
			// string's end (at most 14 bytes from the field: fo >= l3 + 26).
			// The old field is read here, before the tile's stores.
			if constexpr (HM == TX_M_CK_HASH) {
				const bool fix = hs.a6 && kind != 0u && fo < l3 + 40u;
				if (__ballot(fix) != 0ull) {
					const uint32_t old = kind == 3u ? tx_ld32(rs, off + fo, fix)
									: tx_ld16(rs, off + fo, fix && kind != 3u);
					const uint32_t d = old ^ (kind == 3u ? crc : l4ck);
					uint32_t x = 0;
#pragma unroll
					for (uint32_t j = 0; j < 14u; ++j) {
						const uint32_t y = crc32c_u8(s_crc, x, j < 4u ? (d >> (8u * j)) & 0xffu : 0u);
						x = fix && fo + j < l3 + 40u ? y : x;
					}
					fh ^= x;
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
			if constexpr (HM == TX_M_CK_HASH) {
				if (valid)
					a.hash[pi] = fh;
			}
		}
	}
}
