// mi_cls_move_dev.h -- the pool move's kernels (mi_cls_pool_move, mi_cls.h):
// the packet memory of a planned batch.  Every FRESH record's frame is copied
// into the packet the pool plan gave it and the packet's metadata line is
// written; an INPLACE record's line is rewritten where the frame sits.
//
// Two launches on the stream, no block waits for another one:
//
//   move     a wave takes tiles of MI_CLS_MOVE_TILE records, dealt statically
//            (tile w, w + W, ... for wave w of W = grid x MOVE_WAVES).  One
//            record per lane: the fate, the packet's address, the guards, ent
//            and the 64-B line as four 16-B stores.  Then the tile's frames as
//            one run of 16-B pieces: a prefix sum of the lanes' piece counts
//            numbers them, lane j of round B takes pieces B + j, B + 64 + j,
//            ... (MOVE_PIECES of them), finds each piece's owner by a binary
//            search over the lanes' first pieces (as ck_sum_wave) and issues
//            all its loads before the first store.  A 9000-B frame beside 63
//            short ones is spread over the 64 lanes like any other bytes.  The
//            next tile's per-record words are loaded with the first round.
//            The counters: summed per wave, one vector atomic per wave and
//            counter into the context's scratch;
//   finish   one wave: the four counters to out by plain stores.
//
// Source: unaligned 16-B buffer loads through a descriptor of exactly
// pkts_bytes.  A piece whose 16 B would reach past pkts_bytes (only the last
// piece of a frame that ends within 15 B of the buffer's end) is read byte by
// byte up to the buffer's end instead, so no value depends on how the hardware
// clips a load that straddles the end.  Destination: aligned 16-B global
// stores (the line is 64-B aligned, data_from_meta a multiple of 16).
//
// Bounds: every address the kernel forms from caller data is checked before it
// is used: a packet's line and data against [arena_lo, arena_lo + arena_bytes),
// idx against ngot, a frame against pkts_bytes, a table index against the
// table; every per-record load index is clamped below n and every per-record
// store guarded by i < n.  No LDS.
#ifndef MI_CLS_MOVE_DEV_H_
#define MI_CLS_MOVE_DEV_H_

#include "mi_cls_dev.h"

#define MOVE_THREADS (MOVE_WAVES * WAVE)
#define MOVE_PIECES 8u                       // 16-B pieces per lane and round
#ifndef MI_CLS_MOVE_NT
#define MI_CLS_MOVE_NT 1                     // the data stores: 1 nontemporal, 0 plain ("Measured")
#endif
#define MOVE_CTR_MOVED 0u                    // the scratch counters, in mi_cls_move_out_t's order
#define MOVE_CTR_INPLACE 1u
#define MOVE_CTR_BYTES 2u
#define MOVE_CTR_REFUSED 3u
static_assert(MI_CLS_MOVE_TILE == WAVE, "one record per lane");
static_assert(MI_CLS_MOVE_ROUND == MOVE_PIECES * WAVE * 16u, "a round is MOVE_PIECES pieces per lane");
static_assert(sizeof(mi_cls_move_out_t) == 4 * 8, "four counters");
static_assert(sizeof(mi_cls_pkt_meta_t) == 64, "the line is four 16-B stores");
static_assert(sizeof(mi_cls_result_t) == 16, "a record is one 16-B load");

// The per-record words of a tile: loaded one tile ahead.  No branch: the tile
// behind a wave's last one is that one again.
struct MoveRec {
	uint4 r;
	uint64_t pk;
	uint32_t dec, idx, off, len;
};

template <bool PK>
__device__ __forceinline__ MoveRec move_load(const MoveArgs &a, uint64_t tile, uint32_t lane)
{
	MoveRec m;
	const uint64_t i = tile * WAVE + lane;
	const uint32_t ic = (uint32_t)(i < a.n ? i : a.n - 1u);
	m.dec = a.dec[ic];
	m.idx = a.idx[ic];
	m.off = a.off[ic];
	m.len = a.len[ic];
	m.r = reinterpret_cast<const uint4 *>(a.res)[ic];
	m.pk = PK ? a.pk[ic] : 0ull;
	return m;
}

// [p, p + need) lies in the arena and p is a line's address
__device__ __forceinline__ bool move_in_arena(const MoveArgs &a, uint64_t p, uint64_t need)
{
	if (p == 0ull || (p & 63ull) != 0ull || p < a.arena_lo)
		return false;
	const uint64_t at = p - a.arena_lo;
	return at <= a.arena_bytes && need <= a.arena_bytes - at;
}

// The last piece of a frame that ends within 15 B of the buffer's end: the
// bytes up to the end, one by one
__device__ __forceinline__ u32x4 move_tail(__amdgpu_buffer_rsrc_t rs, uint32_t s, uint32_t rem)
{
	u32x4 v = { 0u, 0u, 0u, 0u };
#pragma unroll
	for (uint32_t b = 0; b < 16u; ++b) {
		const uint32_t x = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, b < rem ? s + b : OOB_OFF, 0, 0) & 0xffu;
		v[b >> 2] |= (b < rem ? x : 0u) << (8u * (b & 3u));
	}
	return v;
}

// PK: pk[] is given
template <bool PK>
__global__ __launch_bounds__(MOVE_THREADS) void mi_cls_move_kernel(MoveArgs a)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1u), wave = threadIdx.x / WAVE;
	const uint64_t W = (uint64_t)gridDim.x * MOVE_WAVES;
	const uint64_t tiles = ((uint64_t)a.n + WAVE - 1u) / WAVE;
	const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.pkts, (short)0, (int)a.pkts_bytes,
									    0x00020000);
	const uint32_t ndst = min(a.ndst, (uint32_t)MI_CLS_ENQ_DST_MAX);
	uint32_t moved = 0, inpl = 0, refused = 0;
	unsigned long long bytes = 0;
	uint64_t tile = (uint64_t)blockIdx.x * MOVE_WAVES + wave;
	if (tile >= tiles)
		return;
	MoveRec nx = move_load<PK>(a, tile, lane);
	for (; tile < tiles; tile += W) {
		const MoveRec m = nx;
		const uint64_t i = tile * WAVE + lane;
		const bool in = i < a.n;
		const uint32_t fate = in ? m.dec & 15u : MI_CLS_PF_NONE;
		const bool fresh = fate == MI_CLS_PF_FRESH, keep = fate == MI_CLS_PF_INPLACE;
		const uint32_t len = m.len, pad = (len + 15u) & ~15u;
		const uint4 r = m.r;
		const uint32_t cos = (r.y >> 16) & 0xFFu, queue = r.z & 0xFFFFu;
		// ---- every lane's loads of the first level, no branch among them: the
		// packet (got is readable at index 0 whatever ngot is: the launcher's
		// business) and the table's two words of the CoS
		const bool idx_ok = m.idx < a.ngot;
		const uint64_t taken = a.got[idx_ok ? m.idx : 0u];
		const uint32_t nq = a.tab->cos_nq[cos], q0 = a.tab->cos_q0[cos];
		// ---- the packet and the guards
		uint64_t line = 0ull;
		if (fresh || keep) {
			bool ok = (uint64_t)m.off + len <= a.pkts_bytes;
			if (fresh) {
				line = taken;
				// the second test: the packet its user pointer comes from
				ok = ok && idx_ok && move_in_arena(a, line, (uint64_t)a.data_from_meta + pad) &&
				     (m.pk == 0ull || move_in_arena(a, m.pk, 64u));
			} else {
				line = m.pk;
				ok = ok && PK && move_in_arena(a, line, 64u);
			}
			if (!ok) {
				line = 0ull;
				++refused;
			}
		}
		// ---- the second level: what the line keeps (addresses checked above),
		// the table's entry; then its queue
		u32x4 *l = (u32x4 *)(uintptr_t)line;
		uint32_t doff = a.headroom;
		uint64_t up = 0ull;
		if (line && keep) {
			doff = ((const mi_cls_pkt_meta_t *)l)->data_off;
			up = ((const mi_cls_pkt_meta_t *)l)->user_ptr;
		} else if (line && m.pk) {
			up = ((const mi_cls_pkt_meta_t *)(uintptr_t)m.pk)->user_ptr;
		}
		const uint32_t e = q0 + queue;
		const uint32_t id = a.tab->ent_dst[e < MI_CLS_ENQ_ENT ? e : 0u];
		const bool mapped = ((r.y >> 8) & 0xFFu) == MI_CLS_OUT_ENQ && queue < nq && e < MI_CLS_ENQ_ENT && id < ndst;
		const uint64_t dqv = a.dstq[id < MI_CLS_ENQ_DST_MAX ? id : 0u];   // the scratch holds MI_CLS_ENQ_DST_MAX words
		const uint64_t dq = mapped ? dqv : 0ull;
		if (in)
			a.ent[i] = line;
		// ---- the line
		if (line) {
			if (keep) {
				++inpl;
			} else {
				++moved;
				bytes += len;
			}
			// data_off, len, in_flags | err, cos, cls_mark, l2, l3, l4, rsv |
			// dst_queue, input | user_ptr, rsv
			l[0] = u32x4{ doff, len, r.x, 0u };
			l[1] = u32x4{ (r.y & 0xFFu) | (cos << 8) | (r.z & 0xFFFF0000u), (r.w & 0xFFFFu) << 16, r.w >> 16, 0u };
			l[2] = u32x4{ (uint32_t)dq, (uint32_t)(dq >> 32), (uint32_t)a.input, (uint32_t)(a.input >> 32) };
			l[3] = u32x4{ (uint32_t)up, (uint32_t)(up >> 32), 0u, 0u };
		}
		const uint64_t ahead = tile + W < tiles ? tile + W : tile;
		// ---- the frames, as one run of 16-B pieces over the wave (all lanes)
		const uint32_t cnt = line && fresh ? pad >> 4 : 0u;
		const uint32_t incl = wave_scan_add(cnt, lane);
		const uint32_t first = incl - cnt;   // number of this lane's first piece
		const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
		const uint64_t data = line + a.data_from_meta;
		const uint32_t dlo = (uint32_t)data, dhi = (uint32_t)(data >> 32);
		for (uint32_t B = 0; B < total; B += MOVE_PIECES * WAVE) {
			u32x4 v[MOVE_PIECES];
			uint64_t d[MOVE_PIECES];
			uint32_t s[MOVE_PIECES];
			bool live[MOVE_PIECES], tail[MOVE_PIECES];
			bool any_tail = false;
#pragma unroll
			for (uint32_t h = 0; h < MOVE_PIECES; ++h) {
				const uint32_t g = B + WAVE * h + lane;
				uint32_t lo = 0;
#pragma unroll
				for (uint32_t st = WAVE / 2; st >= 1; st >>= 1) {
					const uint32_t c = lo + st;
					lo = lane_get(first, c) <= g ? c : lo;
				}
				const uint32_t q = 16u * (g - lane_get(first, lo));
				s[h] = lane_get(m.off, lo) + q;
				d[h] = (((uint64_t)lane_get(dhi, lo) << 32) | lane_get(dlo, lo)) + q;
				live[h] = g < total;
				tail[h] = live[h] && (uint64_t)s[h] + 16u > a.pkts_bytes;
				any_tail |= tail[h];
			}
			// the next tile's words travel with the first round's loads
			if (B == 0u)
				nx = move_load<PK>(a, ahead, lane);
#pragma unroll
			for (uint32_t h = 0; h < MOVE_PIECES; ++h)
				v[h] = __builtin_amdgcn_raw_buffer_load_b128(rs, live[h] && !tail[h] ? s[h] : OOB_OFF, 0, 0);
			if (any_tail) {
#pragma unroll
				for (uint32_t h = 0; h < MOVE_PIECES; ++h)
					if (tail[h])
						v[h] = move_tail(rs, s[h], (uint32_t)(a.pkts_bytes - s[h]));
			}
			// every load of the round has landed before its first store, on every
			// lane: stated once here, the compiler need not wait again at the top
			// of the next round, where the stores are still on their way
			__builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), the other counters left alone
#pragma unroll
			for (uint32_t h = 0; h < MOVE_PIECES; ++h)
				if (live[h]) {
#if MI_CLS_MOVE_NT
					__builtin_nontemporal_store(v[h], (u32x4 *)(uintptr_t)d[h]);
#else
					*(u32x4 *)(uintptr_t)d[h] = v[h];
#endif
				}
		}
		if (total == 0u)
			nx = move_load<PK>(a, ahead, lane);
	}
	// ---- the counters: per wave, then one vector atomic each
	uint32_t blo = (uint32_t)bytes, bhi = (uint32_t)(bytes >> 32);
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		moved += (uint32_t)__shfl_xor((int)moved, o);
		inpl += (uint32_t)__shfl_xor((int)inpl, o);
		refused += (uint32_t)__shfl_xor((int)refused, o);
		// a lane's bytes are below 2^32 x 65535; summed in two halves
		const unsigned long long ob = ((unsigned long long)(uint32_t)__shfl_xor((int)bhi, o) << 32) |
					     (uint32_t)__shfl_xor((int)blo, o);
		bytes += ob;
		blo = (uint32_t)bytes;
		bhi = (uint32_t)(bytes >> 32);
	}
	if (lane == 0) {
		if (moved)
			atomicAdd(&a.ctr[MOVE_CTR_MOVED], (unsigned long long)moved);
		if (inpl)
			atomicAdd(&a.ctr[MOVE_CTR_INPLACE], (unsigned long long)inpl);
		if (bytes)
			atomicAdd(&a.ctr[MOVE_CTR_BYTES], bytes);
		if (refused)
			atomicAdd(&a.ctr[MOVE_CTR_REFUSED], (unsigned long long)refused);
	}
}

// One wave: the counters to out (device or host memory), plain stores
__global__ __launch_bounds__(WAVE) void mi_cls_move_finish_kernel(MoveArgs a)
{
	if (threadIdx.x < 4u)
		reinterpret_cast<uint64_t *>(a.out)[threadIdx.x] = a.ctr[threadIdx.x];
}

#endif /* MI_CLS_MOVE_DEV_H_ */
