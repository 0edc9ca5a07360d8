// mi_cls_lso_dev.h -- device side of the LSO segmentation
// (mi_cls_lso_segment, include/mi_cls.h): every segment of a batch of large
// packets cut, its header edited by the packet's LSO profile, and stored.
//
// What it replaces (reference, platform/linux-generic/odp_packet_io.c):
//   :3154-3251  _odp_lso_create_packets (header copy, payload slices)
//   :2985-3018  lso_update_ipv4 (tot_len, fragment word, header checksum)
//   :3020-3087  lso_update_custom (ADD_SEGMENT_NUM, WRITE_BITS)
// The plan (segment count, payload per segment: :3089-3152) is the host's
// (mi_cls_lso_plan); the kernel takes it from the descriptors.
//
// Shape: one wavefront per entry of the segment table, persistent waves in
// blocks of LSO_NW striding over the table.  A wave's descriptor loads are
// wave-uniform.  The segment's first bytes -- the header, every byte a
// custom field may reach (offset <= 128, size <= 8), and what follows up to
// the next 16-byte boundary of the destination -- are held one dword per
// lane (lane L: segment bytes 4L .. 4L + 3, lanes 0-37); the profile's edits
// are made on those registers (the field bytes gathered with readlane, the
// result put back into the lanes that hold them) before they are stored, so
// every destination byte is written exactly once.  The rest of the payload
// moves in 16-byte pieces: loads at any source alignment (which gfx950
// serves), stores aligned to the destination, a byte tail.  No LDS, no
// scratch; the profile table is read from the kernel arguments.
#pragma once
#include "mi_cls_dev.h"

#define LSO_HEAD_MIN 136u   // MI_CLS_LSO_MAX_PAYLOAD_OFFSET + the widest field
// the head ends below LSO_HEAD_MIN + 16 = 152: lanes 0-37 hold it

// Source bytes by batch offset (any alignment); a false predicate reads
// nothing and gives 0.
__device__ __forceinline__ uint32_t lso_ld32(__amdgpu_buffer_rsrc_t rs, uint32_t o, bool ok)
{
	return __builtin_amdgcn_raw_buffer_load_b32(rs, ok ? o : OOB_OFF, 0, 0);
}

__device__ __forceinline__ uint32_t lso_ld8(__amdgpu_buffer_rsrc_t rs, uint32_t o, bool ok)
{
	return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, ok ? o : OOB_OFF, 0, 0) & 0xffu;
}

__device__ __forceinline__ uint32_t lso_uni(uint32_t v)
{
	return __builtin_amdgcn_readfirstlane(v);
}

// The big-endian value of the header bytes [o, o + size) (o, size
// wave-uniform, size <= 8, o + size <= LSO_HEAD_MIN).
__device__ __forceinline__ uint64_t lso_get(uint32_t hw, uint32_t o, uint32_t size)
{
	uint64_t v = 0;
	for (uint32_t b = 0; b < size; ++b) {
		const uint32_t x = o + b;
		const uint32_t w = __builtin_amdgcn_readlane(hw, __builtin_amdgcn_readfirstlane(x >> 2));
		v = (v << 8) | ((w >> (8u * (x & 3u))) & 0xffu);
	}
	return v;
}

// The header dword of `lane` with the bytes [o, o + size) set to the
// big-endian value v.
__device__ __forceinline__ uint32_t lso_put(uint32_t hw, uint32_t lane, uint32_t o, uint32_t size, uint64_t v)
{
	for (uint32_t b = 0; b < size; ++b) {
		const uint32_t x = o + b, sh = 8u * (x & 3u);
		const uint32_t byte = (uint32_t)(v >> (8u * (size - 1u - b))) & 0xffu;
		hw = lane == (x >> 2) ? (hw & ~(0xffu << sh)) | (byte << sh) : hw;
	}
	return hw;
}

__global__ __launch_bounds__(LSO_NW * WAVE) void mi_cls_lso_kernel(LsoArgs a)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
		(void *)a.src, (short)0, (int)OOB_OFF, 0x00020000);

	for (uint32_t j = blockIdx.x * LSO_NW + wave; j < a.nsegs; j += gridDim.x * LSO_NW) {
		// wave-uniform loads (j is): the values into scalar registers
		const uint2 sg = *reinterpret_cast<const uint2 *>(a.seg + j);
		const uint32_t doff = lso_uni(sg.x), i = lso_uni(sg.y);
		if (i >= a.n)
			continue;
		const uint4 dw = *reinterpret_cast<const uint4 *>(a.desc + i);
		const uint32_t d0 = lso_uni(dw.x), d1 = lso_uni(dw.y), first = lso_uni(dw.z);
		const uint32_t hdr = d0 & 0xffffu, pay = d0 >> 16, l3 = d1 & 0xffffu;
		const uint32_t pi = (d1 >> 16) & 0xffu, nseg = d1 >> 24;
		const uint32_t soff = lso_uni(ld_desc(a.off + i)), slen = lso_uni(ld_desc(a.len + i));
		const uint32_t k = j - first;   // j < first wraps: k >= nseg below
		const bool lead = j == first;   // the wave that reports the packet

		// ---- the descriptor, as mi_cls_lso_plan leaves it; anything else is
		// refused (nothing written but st)
		bool good = nseg >= 2u && nseg <= MI_CLS_LSO_MAX_SEGMENTS && pi < a.nprof &&
			    pi < MI_CLS_LSO_PROFILES && hdr <= MI_CLS_LSO_MAX_PAYLOAD_OFFSET && hdr <= slen &&
			    pay != 0u && k < nseg;
		const uint32_t total = good ? slen - hdr : 0u;
		good = good && (nseg - 1u) * pay < total && total <= nseg * pay;
		const uint32_t proto = good ? a.prof[pi].proto : 0u;
		good = good && (proto == MI_CLS_LSO_PROTO_CUSTOM ||
				(proto == MI_CLS_LSO_PROTO_IPV4 && l3 + 20u <= hdr));
		if (!good) {
			if (lead && lane == 0u)
				a.st[i] = (uint8_t)MI_CLS_LSO_ST_DESC;
			continue;
		}
		const uint32_t last_len = hdr + total - (nseg - 1u) * pay;   // the shortest segment
		const uint32_t shift = k * pay;                              // payload bytes before this one
		const uint32_t seg_len = k == nseg - 1u ? last_len : hdr + pay;
		uint8_t *const D = a.dst + doff;

		// ---- the head: segment bytes [0, hb), hb on a 16-byte boundary of
		// the destination (or the segment's end)
		const uint32_t h0 = LSO_HEAD_MIN + ((0u - ((uint32_t)(uintptr_t)D + LSO_HEAD_MIN)) & 15u);
		const uint32_t hb = seg_len < h0 ? seg_len : h0;
		const uint32_t x0 = 4u * lane;
		// a dword wholly on one side of hdr: one load; else its bytes
		const bool whole = x0 + 4u <= hb && (x0 + 4u <= hdr || x0 >= hdr);
		uint32_t hw = lso_ld32(rs, soff + (x0 < hdr ? x0 : x0 + shift), whole);
#pragma unroll
		for (uint32_t b = 0; b < 4u; ++b) {
			const uint32_t x = x0 + b;
			hw |= lso_ld8(rs, soff + (x < hdr ? x : x + shift), !whole && x < hb) << (8u * b);
		}

		// ---- the profile's edits, on the registers
		uint32_t fail = MI_CLS_LSO_ST_OK;
		if (proto == MI_CLS_LSO_PROTO_IPV4) {
			// lso_update_ipv4 (:2985-3018), _odp_packet_ipv4_chksum_insert
			// (odp_packet.c:1888-1949)
			if ((lso_get(hw, l3, 1u) & 15u) != 5u)
				fail = MI_CLS_LSO_ST_IHL;
			hw = lso_put(hw, lane, l3 + 2u, 2u, (seg_len - l3) & 0xffffu);
			uint32_t frag = ((uint32_t)lso_get(hw, l3 + 6u, 2u) + (shift >> 3)) & 0xffffu;
			frag |= k < nseg - 1u ? 0x2000u : 0u;
			hw = lso_put(hw, lane, l3 + 6u, 2u, frag);
			hw = lso_put(hw, lane, l3 + 10u, 2u, 0u);
			uint32_t s = 0;
			for (uint32_t w = 0; w < 10u; ++w)
				s += (uint32_t)lso_get(hw, l3 + 2u * w, 2u);
			s = (s & 0xffffu) + (s >> 16);
			s = (s & 0xffffu) + (s >> 16);
			hw = lso_put(hw, lane, l3 + 10u, 2u, ~s & 0xffffu);
		} else {
			// lso_update_custom (:3020-3087)
			const uint32_t nf = a.prof[pi].num_custom;
			for (uint32_t f = 0; f < nf && f < MI_CLS_LSO_MAX_CUSTOM; ++f) {
				const mi_cls_lso_field_t fd = a.prof[pi].field[f];
				const uint32_t fo = fd.offset, fs = fd.size;
				// odp_packet_copy_to_mem fails past the segment's end: the
				// shortest segment decides for the whole packet
				if (fo + fs > last_len || fo > MI_CLS_LSO_MAX_PAYLOAD_OFFSET || fs > 8u) {
					fail = MI_CLS_LSO_ST_FIELD;
					break;
				}
				uint64_t v = lso_get(hw, fo, fs);
				if (fd.mod_op == MI_CLS_LSO_ADD_SEGMENT_NUM) {
					v += k;
				} else {
					// first, last, else middle (:3070-3075)
					const uint32_t m = k == 0u ? fd.mask[0] : (k == nseg - 1u ? fd.mask[2] : fd.mask[1]);
					const uint32_t b = k == 0u ? fd.value[0] : (k == nseg - 1u ? fd.value[2] : fd.value[1]);
					v = (v & ~(uint64_t)m) | (b & m);
				}
				hw = lso_put(hw, lane, fo, fs, v);
			}
		}
		if (lead && lane == 0u)
			a.st[i] = (uint8_t)fail;
		if (fail != MI_CLS_LSO_ST_OK)
			continue;   // the same for every segment of the packet: none is written

		// ---- stores: the head by dwords where the destination is 4-byte
		// aligned and the dword lies inside, else by bytes
		if (x0 < hb) {
			uint8_t *p = D + x0;
			if (x0 + 4u <= hb && ((uintptr_t)p & 3u) == 0u) {
				*reinterpret_cast<uint32_t *>(p) = hw;
			} else {
#pragma unroll
				for (uint32_t b = 0; b < 4u; ++b)
					if (x0 + b < hb)
						p[b] = (uint8_t)(hw >> (8u * b));
			}
		}
		// ---- the payload past the head: 16-byte pieces, four loads in
		// flight per lane, then a byte tail
		const uint32_t nfull = (seg_len - hb) >> 4;
		const uint32_t sb = soff + shift;
		for (uint32_t c0 = 0; c0 < nfull; c0 += 4u * WAVE) {
			u32x4 v[4];
#pragma unroll
			for (uint32_t u = 0; u < 4u; ++u) {
				const uint32_t c = c0 + u * WAVE + lane;
				v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, c < nfull ? sb + hb + 16u * c : OOB_OFF,
									     0, 0);
			}
#pragma unroll
			for (uint32_t u = 0; u < 4u; ++u) {
				const uint32_t c = c0 + u * WAVE + lane;
				if (c < nfull)
					*reinterpret_cast<u32x4 *>(D + hb + 16u * c) = v[u];
			}
		}
		const uint32_t t0 = hb + 16u * nfull;
		if (t0 + lane < seg_len)
			D[t0 + lane] = (uint8_t)lso_ld8(rs, sb + t0 + lane, true);
	}
}
