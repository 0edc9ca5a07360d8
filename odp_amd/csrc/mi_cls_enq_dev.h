// mi_cls_enq_dev.h -- the enqueue plan's kernels (mi_cls_enq_plan, mi_cls.h):
// the stable grouping of a classified batch by destination queue, the list of
// the records that are not delivered, and the pktio counters.
//
// A record's key is its destination id, or ndst when it is not delivered: the
// plan is the stable sort of the record indexes by key, and gbeg the keys'
// starts.  Keys have up to 14 bits (ndst <= 8192), sorted in one or two
// stable passes of ENQ_BINS = 256 bins (least significant digit first).  Every
// step is a launch of its own on the stream; no block waits for another one:
//
//   key      block b walks its run of tiles: each record's key (the table in
//            LDS) to key16[], the counters, and the low digit's counts of the
//            run to mat[digit * grid + b];
//   scan     one block: mat becomes its exclusive prefix sums, which, the
//            matrix being digit-major, are each (digit, block)'s first place;
//   scatter  block b walks the same run: a record's place is its (digit,
//            block) start, plus the records of that digit in the run's earlier
//            tiles, plus its rank in the tile -- in its wave by match_lanes
//            (mi_cls_rank_dev.h), and the counts of the tile's waves before it;
//   count    (two passes) the high digit's counts over the first pass' order;
//   gbeg     one pass: the scanned matrix holds each key's start (its first
//            block's entry); two: thread j looks at the keys at places j - 1
//            and j of the final order and writes the starts of the groups
//            that begin there; the counters go from the scratch to the
//            caller's block.
//
// Bounds: a key is at most ndst (ENQ_DST_MAX + 1 values), every table index is
// checked before use (a record the table does not map is `stale`), and a
// place is below n because the counts and the ranks come from the same
// key16[] / hi8[] bytes, which only these kernels write.
#ifndef MI_CLS_ENQ_DEV_H_
#define MI_CLS_ENQ_DEV_H_

#include "mi_cls_rank_dev.h"

#define ENQ_THREADS MI_CLS_ENQ_TILE          // one record per thread and tile
#define ENQ_WAVES (ENQ_THREADS / WAVE)
#define ENQ_BINS (1u << MI_CLS_ENQ_DIGIT)
#define ENQ_NCTR 6u                          // the words of mi_cls_enq_out_t
#define ENQ_AHEAD 4u                         // tiles whose loads a block issues together
#define ENQ_SCAN_PER 64u                     // matrix entries per thread of the scan, at most
static_assert(ENQ_BINS * MI_CLS_ENQ_GRID <= ENQ_SCAN_PER * MI_CLS_ENQ_TILE, "the scan holds the matrix in registers");
static_assert(sizeof(mi_cls_enq_out_t) == ENQ_NCTR * sizeof(uint64_t), "six 64-bit counters");
static_assert(MI_CLS_ENQ_DST_MAX < (1u << (2 * MI_CLS_ENQ_DIGIT)), "a key (<= ndst) has two digits");
static_assert(MI_CLS_ENQ_DST_MAX <= 0xFFFEu, "a key fits 16 bits");
static_assert(ENQ_THREADS == 1024 && ENQ_BINS <= ENQ_THREADS, "one thread per bin");
static_assert(MI_CLS_ENQ_ENT == 8 * ENQ_THREADS, "the table's entries load as one 16-B piece per thread");
// LDS per block: key kernel 16 KiB of entries + 2 KiB; scatter 17 KiB: four
// blocks fit a CU's 160 KiB, and the 1024-thread block is what bounds it

// The run of records of block b: [lo, hi)
__device__ __forceinline__ void enq_run(const EnqArgs &a, uint32_t &lo, uint32_t &hi)
{
	const unsigned long long per = (unsigned long long)a.tpb * ENQ_THREADS;
	const unsigned long long l = per * blockIdx.x;
	lo = (uint32_t)(l < a.n ? l : a.n);
	hi = (uint32_t)(l + per < a.n ? l + per : a.n);
}

// One tile's digits counted into s_cnt (zeroed by the caller): per wave the
// first lane of each digit adds its lanes (one LDS atomic per distinct digit
// and wave, whatever the skew).  v: the digit, ENQ_BINS for a lane without a
// record.
__device__ __forceinline__ void enq_count_tile(uint32_t v, uint32_t *s_cnt, unsigned long long below)
{
	const unsigned long long m = match_lanes(v, MI_CLS_ENQ_DIGIT + 1);
	if (v < ENQ_BINS && (m & below) == 0ull)
		atomicAdd(&s_cnt[v], (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(ENQ_THREADS) void mi_cls_enq_key_kernel(EnqArgs a)
{
	__shared__ uint16_t s_dst[MI_CLS_ENQ_ENT];
	__shared__ uint16_t s_q0[256];
	__shared__ uint8_t s_nq[256];
	__shared__ uint32_t s_cnt[ENQ_BINS];
	__shared__ unsigned long long s_ctr[ENQ_NCTR];
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1);
	const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
	{
		// ent_dst sits at byte 776 of the table: 8-byte aligned
		const uint2 *src = reinterpret_cast<const uint2 *>(a.tab->ent_dst);
		uint2 *dst = reinterpret_cast<uint2 *>(s_dst);
		dst[2u * t] = src[2u * t];
		dst[2u * t + 1u] = src[2u * t + 1u];
		if (t < 256u) {
			s_q0[t] = a.tab->cos_q0[t];
			s_nq[t] = a.tab->cos_nq[t];
			s_cnt[t] = 0u;
		}
		if (t < ENQ_NCTR)
			s_ctr[t] = 0ull;
	}
	__syncthreads();
	uint32_t lo, hi;
	enq_run(a, lo, hi);
	// per thread: records, so 32 bits; octets 64 (a run can hold 2^24 tiles)
	uint32_t errs = 0, disc = 0, pkts = 0, dlv = 0, stale = 0;
	unsigned long long octs = 0;
	// ENQ_AHEAD tiles at a time: their records are loaded (indexes clamped
	// into the run, no branch) before the first is used, so a block with one
	// wave per SIMD waits for memory once per ENQ_AHEAD tiles
	for (unsigned long long base = lo; base < hi; base += ENQ_AHEAD * ENQ_THREADS) {
		mi_cls_result_t ra[ENQ_AHEAD];
		uint32_t la[ENQ_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < ENQ_AHEAD; ++u) {
			const unsigned long long i = base + u * ENQ_THREADS + t;
			const uint32_t ic = (uint32_t)(i < hi ? i : hi - 1u);
			ra[u] = a.res[ic];
			la[u] = a.len[ic];
		}
#pragma unroll
		for (uint32_t u = 0; u < ENQ_AHEAD; ++u) {
			const unsigned long long i = base + u * ENQ_THREADS + t;
			uint32_t v = ENQ_BINS;
			if (i < hi) {
				const mi_cls_result_t r = ra[u];
				const uint32_t len = la[u];
				uint32_t key = a.ndst;
				errs += (r.err != 0u || r.outcome == MI_CLS_OUT_PARSE_DROP) ? 1u : 0u;
				disc += (r.outcome == MI_CLS_OUT_DISCARD || r.outcome == MI_CLS_OUT_LOOP) ? 1u : 0u;
				if (r.outcome == MI_CLS_OUT_ENQ) {
					const uint32_t e = (uint32_t)s_q0[r.cos] + r.queue;
					const uint32_t id = r.queue < s_nq[r.cos] && e < MI_CLS_ENQ_ENT ? s_dst[e] : 0xFFFFu;
					if (id < a.ndst) {
						key = id;
						++dlv;
						if (r.err == 0u) {
							++pkts;
							octs += len;
						}
					} else {
						++stale;
					}
				}
				a.key16[i] = (uint16_t)key;
				v = key & (ENQ_BINS - 1u);
			}
			enq_count_tile(v, s_cnt, below);
		}
	}
	// counters: summed per wave, one LDS add per wave, then one vector atomic
	// of the block to device memory
	{
		unsigned long long c[ENQ_NCTR] = { errs, disc, pkts, octs, dlv, stale };
#pragma unroll
		for (uint32_t j = 0; j < ENQ_NCTR; ++j) {
#pragma unroll
			for (int o = 32; o > 0; o >>= 1)
				c[j] += __shfl_xor(c[j], o);
			if (lane == 0 && c[j])
				atomicAdd(&s_ctr[j], c[j]);
		}
	}
	__syncthreads();
	if (t < ENQ_BINS)
		a.mat[t * a.grid + blockIdx.x] = s_cnt[t];
	if (t < ENQ_NCTR && s_ctr[t])
		atomicAdd(&a.ctr[t], s_ctr[t]);
}

// The high digit's counts of block b's run of the first pass' order
__global__ __launch_bounds__(ENQ_THREADS) void mi_cls_enq_count_kernel(EnqArgs a)
{
	__shared__ uint32_t s_cnt[ENQ_BINS];
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1);
	const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
	if (t < ENQ_BINS)
		s_cnt[t] = 0u;
	__syncthreads();
	uint32_t lo, hi;
	enq_run(a, lo, hi);
	for (unsigned long long base = lo; base < hi; base += ENQ_AHEAD * ENQ_THREADS) {
		uint32_t v[ENQ_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < ENQ_AHEAD; ++u) {
			const unsigned long long i = base + u * ENQ_THREADS + t;
			v[u] = a.hi8[i < hi ? i : hi - 1u];
			v[u] = i < hi ? v[u] : ENQ_BINS;
		}
#pragma unroll
		for (uint32_t u = 0; u < ENQ_AHEAD; ++u)
			enq_count_tile(v[u], s_cnt, below);
	}
	__syncthreads();
	if (t < ENQ_BINS)
		a.mat[t * a.grid + blockIdx.x] = s_cnt[t];
}

// mat[0 .. ENQ_BINS * grid) becomes its exclusive prefix sums.  One block:
// thread t sums its run of entries, the block scans the 1024 sums (in a wave
// by shuffles, the waves' totals by the first wave), thread t writes its run.
__global__ __launch_bounds__(ENQ_THREADS) void mi_cls_enq_scan_kernel(EnqArgs a)
{
	__shared__ uint32_t s_w[ENQ_WAVES];
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	const uint32_t total = ENQ_BINS * a.grid;
	const uint32_t per = (total + ENQ_THREADS - 1u) / ENQ_THREADS;
	const uint32_t lo = min(t * per, total), hi = min(lo + per, total);
	// the thread's run in registers (per <= ENQ_SCAN_PER; unrolled, constant
	// indexes): its loads go out together, and so do its stores below
	uint32_t v[ENQ_SCAN_PER];
	uint32_t sum = 0;
#pragma unroll
	for (uint32_t j = 0; j < ENQ_SCAN_PER; ++j) {
		v[j] = lo + j < hi ? a.mat[lo + j] : 0u;
		sum += v[j];
	}
	uint32_t x = sum;
	for (uint32_t o = 1; o < WAVE; o <<= 1) {
		const uint32_t y = (uint32_t)__shfl_up((int)x, o);
		x += lane >= o ? y : 0u;
	}
	if (lane == WAVE - 1u)
		s_w[wave] = x;
	__syncthreads();
	if (wave == 0) {
		const uint32_t v = lane < ENQ_WAVES ? s_w[lane] : 0u;
		uint32_t y = v;
		for (uint32_t o = 1; o < ENQ_WAVES; o <<= 1) {
			const uint32_t z = (uint32_t)__shfl_up((int)y, o);
			y += lane >= o ? z : 0u;
		}
		if (lane < ENQ_WAVES)
			s_w[lane] = y - v;
	}
	__syncthreads();
	uint32_t acc = s_w[wave] + x - sum;
#pragma unroll
	for (uint32_t j = 0; j < ENQ_SCAN_PER; ++j) {
		if (lo + j < hi)
			a.mat[lo + j] = acc;
		acc += v[j];
	}
}

// One stable pass.  PASS 0: records in arrival order by the low digit of
// key16; the places go to perm (LAST) or, with each record's high digit, to
// tperm / hi8.  PASS 1: the first pass' order by hi8, to perm.
template <int PASS, bool LAST>
__global__ __launch_bounds__(ENQ_THREADS) void mi_cls_enq_scatter_kernel(EnqArgs a)
{
	__shared__ uint32_t s_base[ENQ_BINS];              // each digit's next place in this run
	__shared__ uint32_t s_wc[ENQ_WAVES * ENQ_BINS];    // per wave and digit: count, then start
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
	if (t < ENQ_BINS)
		s_base[t] = a.mat[t * a.grid + blockIdx.x];
	uint32_t lo, hi;
	enq_run(a, lo, hi);
	uint32_t *wc = s_wc + wave * ENQ_BINS;
	for (unsigned long long base = lo; base < hi; base += ENQ_AHEAD * ENQ_THREADS) {
		// the keys (and first-pass places) of ENQ_AHEAD tiles loaded together,
		// as in the key kernel; then tile by tile, every tile of the group run by
		// the whole block (a tile past the run has no record: v = ENQ_BINS)
		uint32_t ka[ENQ_AHEAD], sa[ENQ_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < ENQ_AHEAD; ++u) {
			const unsigned long long i = base + u * ENQ_THREADS + t;
			const uint32_t ic = (uint32_t)(i < hi ? i : hi - 1u);
			ka[u] = PASS == 0 ? (uint32_t)a.key16[ic] : (uint32_t)a.hi8[ic];
			sa[u] = PASS == 1 ? a.tperm[ic] : ic;
		}
#pragma unroll
		for (uint32_t u = 0; u < ENQ_AHEAD; ++u) {
			const bool in = base + u * ENQ_THREADS + t < hi;
			const uint32_t key = ka[u], src = sa[u];
			const uint32_t v = in ? key & (ENQ_BINS - 1u) : ENQ_BINS;
			for (uint32_t j = lane; j < ENQ_BINS; j += WAVE)
				wc[j] = 0u;
			// the wave's own LDS accesses are in order: no barrier between the
			// zeroing and the counts
			const unsigned long long m = match_lanes(v, MI_CLS_ENQ_DIGIT + 1);
			if (v < ENQ_BINS && (m & below) == 0ull)
				wc[v] = (uint32_t)__popcll(m);
			__syncthreads();
			// thread d: digit d's start for each wave of the tile, and the run's
			// next place of d after the tile
			if (t < ENQ_BINS) {
				uint32_t acc = s_base[t];
				for (uint32_t w = 0; w < ENQ_WAVES; ++w) {
					const uint32_t c = s_wc[w * ENQ_BINS + t];
					s_wc[w * ENQ_BINS + t] = acc;
					acc += c;
				}
				s_base[t] = acc;
			}
			__syncthreads();
			if (v < ENQ_BINS) {
				const uint32_t at = wc[v] + (uint32_t)__popcll(m & below);
				if (at < a.n) {   // always (see the head of this file)
					if (LAST) {
						a.perm[at] = src;
					} else {
						a.tperm[at] = src;
						a.hi8[at] = (uint8_t)(key >> MI_CLS_ENQ_DIGIT);
					}
				}
			}
			__syncthreads();   // s_wc is zeroed again
		}
	}
}

// gbeg[g] = the number of records whose key is below g, g in 0 .. ndst + 1:
// thread j (0 .. n) writes the groups that begin at place j, those above the
// key at place j - 1 up to the key at place j (up to ndst + 1 at place n).  A
// long span (empty groups) is written by the whole wave.  Grid-stride in whole
// waves; the counters leave the scratch by plain stores.  After a single pass
// the scanned matrix already holds the starts: thread g copies gbeg[g].
#define ENQ_GB_THREADS 256
__global__ __launch_bounds__(ENQ_GB_THREADS) void mi_cls_enq_gbeg_kernel(EnqArgs a)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const unsigned long long stride = (unsigned long long)gridDim.x * ENQ_GB_THREADS;
	if (blockIdx.x == 0 && threadIdx.x < ENQ_NCTR)
		reinterpret_cast<uint64_t *>(a.out)[threadIdx.x] = a.ctr[threadIdx.x];
	if (a.passes == 1u) {
		// one pass: a key is its digit, and the scanned matrix has each digit's
		// start in its first block's entry (g <= ndst < ENQ_BINS)
		for (unsigned long long g = (unsigned long long)blockIdx.x * ENQ_GB_THREADS + threadIdx.x;
		     g <= a.ndst + 1u; g += stride)
			a.gbeg[g] = g <= a.ndst ? a.mat[(uint32_t)g * a.grid] : a.n;
		return;
	}
	for (unsigned long long b =(unsigned long long)blockIdx.x * ENQ_GB_THREADS + (threadIdx.x - lane); b <= a.n;
	     b += stride) {
		const unsigned long long j = b + lane;
		uint32_t g0 = 1u, g1 = 0u;   // empty
		if (j <= a.n) {
			// (indexes and keys clamped: no read or store outside the arrays
			// whatever perm holds)
			g0 = j ? min((uint32_t)a.key16[min(a.perm[j - 1u], a.n - 1u)], a.ndst) + 1u : 0u;
			g1 = j < a.n ? min((uint32_t)a.key16[min(a.perm[j], a.n - 1u)], a.ndst) : a.ndst + 1u;
		}
		const bool some = g0 <= g1, big = some && g1 - g0 >= 4u;
		if (some && !big)
			for (uint32_t g = g0; g <= g1; ++g)
				a.gbeg[g] = (uint32_t)j;
		unsigned long long todo = __ballot(big);
		while (todo) {
			const int s = __ffsll((long long)todo) - 1;
			todo &= todo - 1ull;
			const uint32_t l = (uint32_t)__shfl((int)g0, s), h = (uint32_t)__shfl((int)g1, s);
			const uint32_t jj = (uint32_t)(b + (uint32_t)s);
			for (uint32_t g = l + lane; g <= h; g += WAVE)
				a.gbeg[g] = jj;
		}
	}
}

#endif /* MI_CLS_ENQ_DEV_H_ */
