// mi_cls_pool_dev.h -- the pool plan's kernels (mi_cls_pool_plan, mi_cls.h):
// which records of a classified batch take a packet of their CoS's pool, which
// packet, and which get none (the frame longer than the pool's packets, the
// pool run short) and leave the batch as discards.
//
// A record that is neither NONE, INPLACE nor TOO_LONG is ranked: its rank is
// the number of earlier ranked records of its slot.  Every step is a launch of
// its own on the stream; no block waits for another one:
//
//   count    block b walks its run of tiles: each record's fate before the
//            rank; the ranked records of the run per slot to cnt[slot * grid +
//            b] (slot-major), the INPLACE and TOO_LONG records to the scratch
//            counters (one vector atomic per block and counter);
//   place    block b sums, per slot, the counts of the blocks before it (wave
//            w: slot w's row, 64 consecutive words per load) into its 16 starts
//            in LDS, walks the same run and writes res_out, dec and idx: a
//            record's rank is its slot's start, plus the ranked records of the
//            slot in the run's earlier tiles, plus its rank in the tile -- in
//            its wave by match_lanes (mi_cls_rank_dev.h), and the counts of the
//            tile's waves before it;
//   finish   one block: wave w sums slot w's row to need[w], used[w] = min(need,
//            have); the four counts; all to out by plain stores.
//
// Both walks decide a record's fate with pool_fate() from the same words, so
// the counts and the ranks agree; in place (res_out == res) the place launch
// changes a record's outcome byte only after the count launch has ended, and a
// thread reads its record before it writes it.
//
// LDS: count the table (256 + 64 B), 64 B of counts + 8 B; place the table,
// have and base (2 x 64 B), 2 x 64 B of starts, 2 x 1 KiB of the waves' counts
// and first ranks.
//
// Bounds: nslot is clamped to MI_CLS_POOL_SLOTS; a slot is used as an index
// only when it is below nslot; an own[] value selects nothing unless it equals
// a valid slot + 1; every load index is clamped into the block's run and every
// store guarded by i < n.
#ifndef MI_CLS_POOL_DEV_H_
#define MI_CLS_POOL_DEV_H_

#include "mi_cls_rank_dev.h"

#define POOL_THREADS MI_CLS_POOL_TILE        // one record per thread and tile
#define POOL_WAVES (POOL_THREADS / WAVE)
#define POOL_AHEAD 4u                        // tiles whose loads a block issues together
#define POOL_NONE 0xFFFFFFFFu                // idx of a record that takes no packet
#define POOL_CTR_INPLACE 0u                  // the scratch counters
#define POOL_CTR_TOO_LONG 1u
static_assert(POOL_THREADS == 1024 && POOL_WAVES == MI_CLS_POOL_SLOTS, "wave w sums slot w's row");
static_assert(MI_CLS_POOL_SLOTS == 16, "a slot has four bits (match_lanes, dec)");
static_assert(MI_CLS_POOL_GRID % WAVE == 0, "a row is read in whole waves");
static_assert(sizeof(mi_cls_pool_out_t) == 4 * 8 + 2 * 4 * MI_CLS_POOL_SLOTS, "four counts, need, used");
static_assert(sizeof(mi_cls_result_t) == 16, "a record is one 16-B load and store");

// The run of records of block b: [lo, hi)
__device__ __forceinline__ void pool_span(const PoolArgs &a, uint32_t &lo, uint32_t &hi)
{
	const unsigned long long per = (unsigned long long)a.tpb * POOL_THREADS;
	const unsigned long long l = per * blockIdx.x;
	lo = (uint32_t)(l < a.n ? l : a.n);
	hi = (uint32_t)(l + per < a.n ? l + per : a.n);
}

// A record's fate before the rank: NONE, INPLACE, TOO_LONG, or FRESH for a
// ranked record (FRESH or SHORT once its rank is known).  w1: the record's
// second word (err, outcome, cos, hops); own: 0 when the caller gave none.
// slot: below nslot, 0 for NONE.
__device__ __forceinline__ uint32_t pool_fate(uint32_t w1, uint32_t len, uint32_t own, const uint8_t *s_slot,
					      const uint32_t *s_cap, uint32_t nslot, uint32_t &slot)
{
	slot = 0u;
	if (((w1 >> 8) & 0xFFu) != MI_CLS_OUT_ENQ)
		return MI_CLS_PF_NONE;
	const uint32_t s = s_slot[(w1 >> 16) & 0xFFu];
	if (s >= nslot)
		return MI_CLS_PF_NONE;
	slot = s;
	if (own == s + 1u)
		return MI_CLS_PF_INPLACE;
	return len > s_cap[s] ? MI_CLS_PF_TOO_LONG : MI_CLS_PF_FRESH;
}

// have[] / base[] from the launch arguments to LDS: constant indexes, so the
// arguments stay in scalar registers and no lane-indexed copy of them is made
__device__ __forceinline__ void pool_args_lds(const PoolArgs &a, uint32_t *s_have, uint32_t *s_first)
{
#pragma unroll
	for (uint32_t s = 0; s < MI_CLS_POOL_SLOTS; ++s)
		if (threadIdx.x == s) {
			s_have[s] = a.have[s];
			s_first[s] = a.base[s];
		}
}

// The table's device copy to LDS (the whole block; the caller's barrier follows)
__device__ __forceinline__ void pool_tab_lds(const PoolArgs &a, uint8_t *s_slot, uint32_t *s_cap)
{
	const uint32_t t = threadIdx.x;
	if (t < 256u)
		s_slot[t] = a.tab->cos_slot[t];
	if (t < MI_CLS_POOL_SLOTS)
		s_cap[t] = a.tab->slot_cap[t];
}

__global__ __launch_bounds__(POOL_THREADS) void mi_cls_pool_count_kernel(PoolArgs a)
{
	__shared__ uint8_t s_slot[256];
	__shared__ uint32_t s_cap[MI_CLS_POOL_SLOTS];
	__shared__ uint32_t s_cnt[MI_CLS_POOL_SLOTS];
	__shared__ uint32_t s_ctr[2];
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1);
	const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
	const uint32_t nslot = min(a.nslot, (uint32_t)MI_CLS_POOL_SLOTS);
	pool_tab_lds(a, s_slot, s_cap);
	if (t < MI_CLS_POOL_SLOTS)
		s_cnt[t] = 0u;
	if (t < 2u)
		s_ctr[t] = 0u;
	__syncthreads();
	uint32_t lo, hi;
	pool_span(a, lo, hi);
	uint32_t inpl = 0, toolong = 0;
	// POOL_AHEAD tiles at a time, their records loaded (indexes clamped into the
	// run) before the first is used, as in the enqueue plan's key kernel
	for (unsigned long long base = lo; base < hi; base += POOL_AHEAD * POOL_THREADS) {
		uint32_t wa[POOL_AHEAD], la[POOL_AHEAD], oa[POOL_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < POOL_AHEAD; ++u) {
			const unsigned long long i = base + u * POOL_THREADS + t;
			const uint32_t ic = (uint32_t)(i < hi ? i : hi - 1u);
			wa[u] = reinterpret_cast<const uint32_t *>(a.res)[4u * (size_t)ic + 1u];
			la[u] = a.len[ic];
			oa[u] = a.own ? (uint32_t)a.own[ic] : 0u;
		}
#pragma unroll
		for (uint32_t u = 0; u < POOL_AHEAD; ++u) {
			const unsigned long long i = base + u * POOL_THREADS + t;
			uint32_t slot = 0u, fate = MI_CLS_PF_NONE;
			if (i < hi)
				fate = pool_fate(wa[u], la[u], oa[u], s_slot, s_cap, nslot, slot);
			inpl += fate == MI_CLS_PF_INPLACE ? 1u : 0u;
			toolong += fate == MI_CLS_PF_TOO_LONG ? 1u : 0u;
			// per wave the first lane of each slot adds its lanes
			const bool ranked = fate == MI_CLS_PF_FRESH;
			const unsigned long long m = match_lanes(slot, 4) & __ballot(ranked);
			if (ranked && (m & below) == 0ull)
				atomicAdd(&s_cnt[slot], (uint32_t)__popcll(m));
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		inpl += (uint32_t)__shfl_xor((int)inpl, o);
		toolong += (uint32_t)__shfl_xor((int)toolong, o);
	}
	if (lane == 0) {
		if (inpl)
			atomicAdd(&s_ctr[POOL_CTR_INPLACE], inpl);
		if (toolong)
			atomicAdd(&s_ctr[POOL_CTR_TOO_LONG], toolong);
	}
	__syncthreads();
	if (t < MI_CLS_POOL_SLOTS)
		a.cnt[t * a.grid + blockIdx.x] = s_cnt[t];
	if (t < 2u && s_ctr[t])
		atomicAdd(&a.ctr[t], (unsigned long long)s_ctr[t]);
}

// Slot `wave`'s row of the count matrix summed over the blocks [0, nb): every
// lane of the wave gets the sum.  Loads of 64 consecutive words.
__device__ __forceinline__ uint32_t pool_row_sum(const PoolArgs &a, uint32_t wave, uint32_t lane, uint32_t nb)
{
	uint32_t s = 0;
	for (uint32_t b = lane; b < nb; b += WAVE)
		s += a.cnt[wave * a.grid + b];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		s += (uint32_t)__shfl_xor((int)s, o);
	return s;
}

__global__ __launch_bounds__(POOL_THREADS) void mi_cls_pool_place_kernel(PoolArgs a)
{
	__shared__ uint8_t s_slot[256];
	__shared__ uint32_t s_cap[MI_CLS_POOL_SLOTS];
	__shared__ uint32_t s_have[MI_CLS_POOL_SLOTS], s_first[MI_CLS_POOL_SLOTS];
	__shared__ uint32_t s_base[2][MI_CLS_POOL_SLOTS];            // each slot's next rank in this run
	__shared__ uint32_t s_wc[POOL_WAVES * MI_CLS_POOL_SLOTS];    // per wave and slot: the tile's count
	__shared__ uint32_t s_ws[POOL_WAVES * MI_CLS_POOL_SLOTS];    // per wave and slot: its first rank
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
	const uint32_t nslot = min(a.nslot, (uint32_t)MI_CLS_POOL_SLOTS);
	pool_tab_lds(a, s_slot, s_cap);
	pool_args_lds(a, s_have, s_first);
	{
		// the ranked records of slot `wave` in the blocks before this one
		const uint32_t s = pool_row_sum(a, wave, lane, min(blockIdx.x, a.grid));
		if (lane == 0)
			s_base[0][wave] = s;
	}
	__syncthreads();
	uint32_t lo, hi, par = 0;
	pool_span(a, lo, hi);
	uint32_t *wc = s_wc + wave * MI_CLS_POOL_SLOTS;
	for (unsigned long long base = lo; base < hi; base += POOL_AHEAD * POOL_THREADS) {
		uint4 ra[POOL_AHEAD];
		uint32_t la[POOL_AHEAD], oa[POOL_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < POOL_AHEAD; ++u) {
			const unsigned long long i = base + u * POOL_THREADS + t;
			const uint32_t ic = (uint32_t)(i < hi ? i : hi - 1u);
			ra[u] = reinterpret_cast<const uint4 *>(a.res)[ic];
			la[u] = a.len[ic];
			oa[u] = a.own ? (uint32_t)a.own[ic] : 0u;
		}
#pragma unroll
		for (uint32_t u = 0; u < POOL_AHEAD; ++u) {
			const unsigned long long i = base + u * POOL_THREADS + t;
			if (base + u * POOL_THREADS >= hi)   // the whole block: no tile left
				break;
			const bool in = i < hi;
			uint32_t slot = 0u, fate = MI_CLS_PF_NONE;
			if (in)
				fate = pool_fate(ra[u].y, la[u], oa[u], s_slot, s_cap, nslot, slot);
			const bool ranked = fate == MI_CLS_PF_FRESH;
			// the wave's own LDS accesses are in order: no barrier between the
			// zeroing and the counts
			if (lane < MI_CLS_POOL_SLOTS)
				wc[lane] = 0u;
			const unsigned long long m = match_lanes(slot, 4) & __ballot(ranked);
			if (ranked && (m & below) == 0ull)
				wc[slot] = (uint32_t)__popcll(m);
			__syncthreads();
			// thread (w, s): slot s's first rank for wave w of the tile; wave 15's
			// also the run's next rank of s after the tile (the other row of
			// s_base: this one is still being read)
			if (t < POOL_WAVES * MI_CLS_POOL_SLOTS) {
				const uint32_t w = t / MI_CLS_POOL_SLOTS, s = t % MI_CLS_POOL_SLOTS;
				uint32_t acc = s_base[par][s];
				for (uint32_t x = 0; x < w; ++x)
					acc += s_wc[x * MI_CLS_POOL_SLOTS + s];
				s_ws[t] = acc;
				if (w == POOL_WAVES - 1u)
					s_base[par ^ 1u][s] = acc + s_wc[t];
			}
			__syncthreads();
			par ^= 1u;
			if (in) {
				uint32_t idx = POOL_NONE;
				if (ranked) {
					const uint32_t rank = s_ws[wave * MI_CLS_POOL_SLOTS + slot] + (uint32_t)__popcll(m & below);
					if (rank < s_have[slot])
						idx = s_first[slot] + rank;
					else
						fate = MI_CLS_PF_SHORT;
				}
				uint4 r = ra[u];
				if (fate == MI_CLS_PF_TOO_LONG || fate == MI_CLS_PF_SHORT)
					r.y = (r.y & ~0xFF00u) | ((uint32_t)MI_CLS_OUT_DISCARD << 8);
				reinterpret_cast<uint4 *>(a.res_out)[i] = r;
				a.dec[i] = fate | slot << 4;
				a.idx[i] = idx;
			}
		}
	}
}

// One block.  grid == 0 (n == 0): every sum is 0.
__global__ __launch_bounds__(POOL_THREADS) void mi_cls_pool_finish_kernel(PoolArgs a)
{
	__shared__ uint32_t s_need[MI_CLS_POOL_SLOTS], s_used[MI_CLS_POOL_SLOTS];
	__shared__ uint32_t s_have[MI_CLS_POOL_SLOTS], s_first[MI_CLS_POOL_SLOTS];
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	pool_args_lds(a, s_have, s_first);
	__syncthreads();
	const uint32_t need = pool_row_sum(a, wave, lane, min(a.grid, (uint32_t)MI_CLS_POOL_GRID));
	if (lane == 0) {
		s_need[wave] = need;
		s_used[wave] = min(need, s_have[wave]);
	}
	__syncthreads();
	uint32_t *o32 = reinterpret_cast<uint32_t *>(a.out) + 8u;   // need[], used[] follow the four counts
	if (t < MI_CLS_POOL_SLOTS) {
		o32[t] = s_need[t];
		o32[MI_CLS_POOL_SLOTS + t] = s_used[t];
	}
	if (t < 4u) {
		unsigned long long fresh = 0, shorted = 0;
		for (uint32_t s = 0; s < MI_CLS_POOL_SLOTS; ++s) {
			fresh += s_used[s];
			shorted += s_need[s] - s_used[s];
		}
		const unsigned long long v = t == 0u ? a.ctr[POOL_CTR_INPLACE] : t == 1u ? fresh :
					     t == 2u ? a.ctr[POOL_CTR_TOO_LONG] : shorted;
		reinterpret_cast<uint64_t *>(a.out)[t] = v;
	}
}

#endif /* MI_CLS_POOL_DEV_H_ */
