// mi_cls_run_dev.h -- the run plan's kernels (mi_cls_enq_runs, mi_cls.h): a
// classified batch's delivered records in arrival order, cut into the
// reference's runs (equal destination id and CoS, ended by a burst's end), each
// run's packet-vector count, the records that are not delivered, and the pktio
// counters.
//
// A record's key is (destination id << 8 | cos), RUN_NONE when it is not
// delivered.  A delivered record is a run head when the delivered record before
// it -- however many undelivered ones lie between -- has another key or lies
// in another burst, or when there is none.  Every step is a launch of its own
// on the stream; no block waits for another one:
//
//   key      block b walks its run of tiles: each record's key to key[], the
//            counters, and the block's summary: its delivered records, the
//            heads among them that the block decides alone (all but its first
//            delivered record), its first and its last delivered (index, key);
//   scan     one block over the <= MI_CLS_RUN_GRID summaries: the last
//            delivered (index, key) before each block (the rightmost valid one:
//            it passes through blocks that delivered nothing), with it whether
//            the block's first delivered record is a head, and the prefix sums
//            of the delivered records and of the heads;
//   scatter  block b walks the same run: a delivered record's place in seq is
//            its rank among the delivered ones, another's the delivered total
//            plus its rank among the others; a head writes its place and key to
//            head[its rank among the heads];
//   finish   thread r: run r's count from the next head's place, its flags and
//            vectors; the vector sums by atomics on the scratch counters;
//   out      the counters leave the scratch by plain stores.
//
// The delivered record before a lane: in its wave, the highest delivered lane
// below it (a ballot and one shuffle); else the last one of the tile's earlier
// waves, else of the earlier tiles (run_tile: one LDS row per wave and one
// barrier per tile).
//
// Bounds: every table index is checked before use as in the enqueue plan; a
// place is below n and a head's rank below the delivered count because the
// scan's sums and the scatter's ranks come from the same key[] words, which
// only the key kernel writes; both are checked before the store all the same.
#ifndef MI_CLS_RUN_DEV_H_
#define MI_CLS_RUN_DEV_H_

#include "mi_cls_rank_dev.h"

#define RUN_THREADS MI_CLS_RUN_TILE          // one record per thread and tile
#define RUN_WAVES (RUN_THREADS / WAVE)
#define RUN_NONE 0xFFFFFFFFu                 // no key (not delivered), no index (no such record)
#define RUN_NCTR 6u                          // the counters shared with mi_cls_enq_out_t
#define RUN_NOUT 24u                         // the words of mi_cls_run_out_t
#define RUN_CTR_NRUNS 6u
#define RUN_CTR_VECTORS 7u
#define RUN_CTR_NEED 8u
#define RUN_AHEAD 4u                         // tiles whose loads a block issues together
#define RUN_SUM 8u                           // words of a block's summary (six used)
#define RUN_ROW 6u                           // words a wave publishes per tile
static_assert(sizeof(mi_cls_run_out_t) == RUN_NOUT * sizeof(uint64_t), "24 64-bit words");
static_assert(RUN_CTR_NEED + MI_CLS_RUN_VSLOTS == RUN_NOUT, "vec_need ends the block");
static_assert(sizeof(mi_cls_run_t) == 16, "a run is one 16-B store");
static_assert(RUN_THREADS == 1024 && RUN_WAVES <= WAVE, "one lane per wave of the tile");
static_assert(MI_CLS_RUN_GRID == 256, "the scan is one block of a thread per summary");
static_assert(MI_CLS_ENQ_ENT == 8 * RUN_THREADS, "the table's entries load as one 16-B piece per thread");
static_assert(MI_CLS_ENQ_DST_MAX <= (1u << 16), "id << 8 | cos is no RUN_NONE");

// The run of records of block b: [lo, hi)
__device__ __forceinline__ void run_span(const RunArgs &a, uint32_t &lo, uint32_t &hi)
{
	const unsigned long long per = (unsigned long long)a.tpb * RUN_THREADS;
	const unsigned long long l = per * blockIdx.x;
	lo = (uint32_t)(l < a.n ? l : a.n);
	hi = (uint32_t)(l + per < a.n ? l + per : a.n);
}

__device__ __forceinline__ uint32_t run_top(unsigned long long m)   // m != 0: its highest bit
{
	return 63u - (uint32_t)__clzll((long long)m);
}

// The last delivered record so far (idx RUN_NONE: none)
struct RunCarry {
	uint32_t idx, key;
};

struct RunTile {
	bool head;              // this lane's record begins a run
	uint32_t drank, hrank;  // delivered records, heads of the tile before this lane
	uint32_t dtot, htot;    // the tile's delivered records and heads
	bool open;              // (FIRST_IS_HEAD false) the tile holds the first delivered
	uint32_t oidx, okey;    // record since the carry was none: that record
};

// One tile, run by the whole block: lane's record i has `key`.  carry: the last
// delivered record before the tile, replaced by the one after it.  A delivered
// record with none before it is a head (FIRST_IS_HEAD: the scatter, whose carry
// comes from the scan) or is left out of the heads and reported (the key
// kernel: the block cannot tell).  s: RUN_ROW x RUN_WAVES words of LDS; two
// rows alternate between calls, so one barrier per tile is enough: a row is
// written again only after the barrier of the tile in between.
template <bool FIRST_IS_HEAD>
__device__ __forceinline__ RunTile run_tile(uint32_t key, uint32_t i, uint32_t burst, RunCarry &carry, uint32_t *s)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
	const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
	const bool dlv = key != RUN_NONE;
	// in the wave: the delivered lane before this one, by a ballot and a shuffle
	const unsigned long long d = __ballot(dlv);
	const unsigned long long db = d & below;
	const uint32_t src = db ? run_top(db) : lane;
	const uint32_t q = i / burst;
	const uint32_t pk = (uint32_t)__shfl((int)key, (int)src), pq = (uint32_t)__shfl((int)q, (int)src);
	const bool hin = dlv && db != 0ull && (pk != key || pq != q);
	const unsigned long long hw = __ballot(hin);
	{
		// the wave's row: delivered, heads decided in the wave, its first and
		// its last delivered (index, key); lane k writes word k
		const int f = d ? __ffsll((long long)d) - 1 : 0, l = d ? (int)run_top(d) : 0;
		const uint32_t fi = (uint32_t)__shfl((int)i, f), fk = (uint32_t)__shfl((int)key, f);
		const uint32_t li = (uint32_t)__shfl((int)i, l), lk = (uint32_t)__shfl((int)key, l);
		const uint32_t v = lane == 0 ? (uint32_t)__popcll(d) : lane == 1 ? (uint32_t)__popcll(hw) :
				   lane == 2 ? fi : lane == 3 ? fk : lane == 4 ? li : lk;
		if (lane < RUN_ROW)
			s[lane * RUN_WAVES + wave] = v;
	}
	__syncthreads();
	// lane j < RUN_WAVES looks at wave j of the tile (every wave does the same)
	const bool wl = lane < RUN_WAVES;
	const uint32_t j = wl ? lane : 0u;
	const uint32_t dc = wl ? s[j] : 0u, hn = wl ? s[RUN_WAVES + j] : 0u;
	const uint32_t fi = s[2u * RUN_WAVES + j], fk = s[3u * RUN_WAVES + j];
	const uint32_t li = s[4u * RUN_WAVES + j], lk = s[5u * RUN_WAVES + j];
	const unsigned long long m = __ballot(dc != 0u);   // the waves that delivered
	const unsigned long long mb = m & below;
	const uint32_t ws = mb ? run_top(mb) : lane;
	uint32_t ci = (uint32_t)__shfl((int)li, (int)ws), ck = (uint32_t)__shfl((int)lk, (int)ws);
	if (!mb) {
		ci = carry.idx;
		ck = carry.key;
	}
	// wave j's first delivered record against the one before it
	const bool none = ci == RUN_NONE;
	const bool bh = dc != 0u && (none ? FIRST_IS_HEAD : (ck != fk || ci / burst != fi / burst));
	uint32_t dx = dc, hx = hn + (bh ? 1u : 0u);   // inclusive sums over the waves
#pragma unroll
	for (uint32_t o = 1; o < RUN_WAVES; o <<= 1) {
		const uint32_t y = (uint32_t)__shfl_up((int)dx, o), z = (uint32_t)__shfl_up((int)hx, o);
		dx += lane >= o ? y : 0u;
		hx += lane >= o ? z : 0u;
	}
	RunTile r;
	r.dtot = (uint32_t)__shfl((int)dx, RUN_WAVES - 1);
	r.htot = (uint32_t)__shfl((int)hx, RUN_WAVES - 1);
	r.open = false;
	r.oidx = r.okey = RUN_NONE;
	if (!FIRST_IS_HEAD) {
		const unsigned long long op = __ballot(dc != 0u && none);
		if (op) {
			const int o = __ffsll((long long)op) - 1;
			r.open = true;
			r.oidx = (uint32_t)__shfl((int)fi, o);
			r.okey = (uint32_t)__shfl((int)fk, o);
		}
	}
	const uint32_t dbase = (uint32_t)__shfl((int)(dx - dc), (int)wave);
	const uint32_t hbase = (uint32_t)__shfl((int)(hx - hn - (bh ? 1u : 0u)), (int)wave);
	const bool myb = __shfl((int)bh, (int)wave) != 0;
	if (m) {
		const int top = (int)run_top(m);
		carry.idx = (uint32_t)__shfl((int)li, top);
		carry.key = (uint32_t)__shfl((int)lk, top);
	}
	// this wave's lanes: the first delivered one takes the wave's answer
	const bool firsth = dlv && db == 0ull && myb;
	const unsigned long long hall = hw | __ballot(firsth);
	r.head = hin || firsth;
	r.drank = dbase + (uint32_t)__popcll(db);
	r.hrank = hbase + (uint32_t)__popcll(hall & below);
	return r;
}

__global__ __launch_bounds__(RUN_THREADS) void mi_cls_run_key_kernel(RunArgs a)
{
	__shared__ uint16_t s_dst[MI_CLS_ENQ_ENT];
	__shared__ uint16_t s_q0[256];
	__shared__ uint8_t s_nq[256];
	__shared__ uint32_t s_t[2][RUN_ROW * RUN_WAVES];
	__shared__ unsigned long long s_ctr[RUN_NCTR];
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1);
	{
		// ent_dst sits at byte 776 of the table: 8-byte aligned
		const uint2 *src = reinterpret_cast<const uint2 *>(a.tab->ent_dst);
		uint2 *dst = reinterpret_cast<uint2 *>(s_dst);
		dst[2u * t] = src[2u * t];
		dst[2u * t + 1u] = src[2u * t + 1u];
		if (t < 256u) {
			s_q0[t] = a.tab->cos_q0[t];
			s_nq[t] = a.tab->cos_nq[t];
		}
		if (t < RUN_NCTR)
			s_ctr[t] = 0ull;
	}
	__syncthreads();
	uint32_t lo, hi;
	run_span(a, lo, hi);
	uint32_t errs = 0, disc = 0, pkts = 0, dlv = 0, stale = 0;
	unsigned long long octs = 0;
	// the block's summary, the same in every thread
	RunCarry carry = { RUN_NONE, RUN_NONE };
	uint32_t bdlv = 0, bheads = 0, bfi = RUN_NONE, bfk = RUN_NONE, par = 0;
	// RUN_AHEAD tiles at a time, their records loaded (indexes clamped into the
	// run) before the first is used, as in the enqueue plan's key kernel
	for (unsigned long long base = lo; base < hi; base += RUN_AHEAD * RUN_THREADS) {
		mi_cls_result_t ra[RUN_AHEAD];
		uint32_t la[RUN_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < RUN_AHEAD; ++u) {
			const unsigned long long i = base + u * RUN_THREADS + t;
			const uint32_t ic = (uint32_t)(i < hi ? i : hi - 1u);
			ra[u] = a.res[ic];
			la[u] = a.len[ic];
		}
#pragma unroll
		for (uint32_t u = 0; u < RUN_AHEAD; ++u) {
			const unsigned long long i = base + u * RUN_THREADS + t;
			if (base + u * RUN_THREADS >= hi)   // the whole block: no tile left
				break;
			uint32_t key = RUN_NONE;
			if (i < hi) {
				const mi_cls_result_t r = ra[u];
				const uint32_t len = la[u];
				errs += (r.err != 0u || r.outcome == MI_CLS_OUT_PARSE_DROP) ? 1u : 0u;
				disc += (r.outcome == MI_CLS_OUT_DISCARD || r.outcome == MI_CLS_OUT_LOOP) ? 1u : 0u;
				if (r.outcome == MI_CLS_OUT_ENQ) {
					const uint32_t e = (uint32_t)s_q0[r.cos] + r.queue;
					const uint32_t id = r.queue < s_nq[r.cos] && e < MI_CLS_ENQ_ENT ? s_dst[e] : 0xFFFFu;
					if (id < a.ndst) {
						key = id << 8 | r.cos;
						++dlv;
						if (r.err == 0u) {
							++pkts;
							octs += len;
						}
					} else {
						++stale;
					}
				}
				a.key[i] = key;
			}
			const RunTile r = run_tile<false>(key, (uint32_t)i, a.burst, carry, s_t[par]);
			par ^= 1u;
			bdlv += r.dtot;
			bheads += r.htot;
			if (r.open) {
				bfi = r.oidx;
				bfk = r.okey;
			}
		}
	}
	{
		unsigned long long c[RUN_NCTR] = { errs, disc, pkts, octs, dlv, stale };
#pragma unroll
		for (uint32_t j = 0; j < RUN_NCTR; ++j) {
#pragma unroll
			for (int o = 32; o > 0; o >>= 1)
				c[j] += __shfl_xor(c[j], o);
			if (lane == 0 && c[j])
				atomicAdd(&s_ctr[j], c[j]);
		}
	}
	__syncthreads();
	if (t < RUN_NCTR && s_ctr[t])
		atomicAdd(&a.ctr[t], s_ctr[t]);
	if (t == 0) {
		uint32_t *sum = a.sum + blockIdx.x * RUN_SUM;
		sum[0] = bdlv;
		sum[1] = bheads;
		sum[2] = bfi;
		sum[3] = bfk;
		sum[4] = carry.idx;
		sum[5] = carry.key;
	}
}

// One block, thread b for block b's summary: what precedes each block.  The
// last delivered record is carried by a rightmost-valid scan (in the wave the
// ballot and shuffle of run_tile, the earlier waves' through LDS); the sums by
// shuffles, the waves' totals through LDS.
#define RUN_SCAN_WAVES (MI_CLS_RUN_GRID / WAVE)
__global__ __launch_bounds__(MI_CLS_RUN_GRID) void mi_cls_run_scan_kernel(RunArgs a)
{
	__shared__ uint32_t s_li[RUN_SCAN_WAVES], s_lk[RUN_SCAN_WAVES];
	__shared__ uint32_t s_d[RUN_SCAN_WAVES], s_h[RUN_SCAN_WAVES];
	const uint32_t b = threadIdx.x, lane = b & (WAVE - 1), wave = b / WAVE;
	const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
	const bool in = b < a.grid;
	const uint32_t *sum = a.sum + (in ? b : 0u) * RUN_SUM;
	const uint32_t dc = in ? sum[0] : 0u, hn = in ? sum[1] : 0u;
	const uint32_t fi = sum[2], fk = sum[3], li = sum[4], lk = sum[5];
	const unsigned long long m = __ballot(dc != 0u);
	const unsigned long long mb = m & below;
	const uint32_t ws = mb ? run_top(mb) : lane;
	uint32_t ci = (uint32_t)__shfl((int)li, (int)ws), ck = (uint32_t)__shfl((int)lk, (int)ws);
	{
		const int top = m ? (int)run_top(m) : 0;
		const uint32_t wi = (uint32_t)__shfl((int)li, top), wk = (uint32_t)__shfl((int)lk, top);
		if (lane == 0) {
			s_li[wave] = m ? wi : RUN_NONE;
			s_lk[wave] = m ? wk : RUN_NONE;
		}
	}
	__syncthreads();
	if (!mb) {
		ci = ck = RUN_NONE;
		for (uint32_t w = 0; w < wave; ++w)
			if (s_li[w] != RUN_NONE) {
				ci = s_li[w];
				ck = s_lk[w];
			}
	}
	const bool bh = dc != 0u && (ci == RUN_NONE || ck != fk || ci / a.burst != fi / a.burst);
	uint32_t dx = dc, hx = hn + (bh ? 1u : 0u);
	for (uint32_t o = 1; o < WAVE; o <<= 1) {
		const uint32_t y = (uint32_t)__shfl_up((int)dx, o), z = (uint32_t)__shfl_up((int)hx, o);
		dx += lane >= o ? y : 0u;
		hx += lane >= o ? z : 0u;
	}
	if (lane == WAVE - 1u) {
		s_d[wave] = dx;
		s_h[wave] = hx;
	}
	__syncthreads();
	for (uint32_t w = 0; w < wave; ++w) {
		dx += s_d[w];
		hx += s_h[w];
	}
	if (in)
		a.pre[b] = make_uint4(dx - dc, hx - hn - (bh ? 1u : 0u), ci, ck);
	if (b == MI_CLS_RUN_GRID - 1u) {   // blocks past the grid add nothing: the totals
		a.tot[0] = dx;
		a.tot[1] = hx;
		a.ctr[RUN_CTR_NRUNS] = hx;
	}
}

__global__ __launch_bounds__(RUN_THREADS) void mi_cls_run_scatter_kernel(RunArgs a)
{
	__shared__ uint32_t s_t[2][RUN_ROW * RUN_WAVES];
	const uint32_t t = threadIdx.x;
	const uint4 p = a.pre[blockIdx.x];
	const uint32_t total = a.tot[0];
	RunCarry carry = { p.z, p.w };
	uint32_t dbase = p.x, hbase = p.y, par = 0;
	uint32_t lo, hi;
	run_span(a, lo, hi);
	for (unsigned long long base = lo; base < hi; base += RUN_AHEAD * RUN_THREADS) {
		uint32_t ka[RUN_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < RUN_AHEAD; ++u) {
			const unsigned long long i = base + u * RUN_THREADS + t;
			ka[u] = a.key[i < hi ? i : hi - 1u];
		}
#pragma unroll
		for (uint32_t u = 0; u < RUN_AHEAD; ++u) {
			const unsigned long long i = base + u * RUN_THREADS + t;
			if (base + u * RUN_THREADS >= hi)
				break;
			const bool in = i < hi;
			const uint32_t key = in ? ka[u] : RUN_NONE;
			const RunTile r = run_tile<true>(key, (uint32_t)i, a.burst, carry, s_t[par]);
			par ^= 1u;
			if (in) {
				const uint32_t dr = dbase + r.drank;   // delivered records before this one
				const uint32_t at = key != RUN_NONE ? dr : total + ((uint32_t)i - dr);
				if (at < a.n)   // always (see the head of this file)
					a.seq[at] = (uint32_t)i;
				const uint32_t hr = hbase + r.hrank;
				if (r.head && hr < a.n)
					a.head[hr] = make_uint2(at, key);
			}
			dbase += r.dtot;
			hbase += r.htot;
		}
	}
}

// Run r, by thread r (grid-stride): its count from the next head's place (the
// delivered total after the last run), flags and vectors; the entry is one
// 16-B store, left out past run_cap.  The vectors are summed over all runs: per
// block in LDS, then one vector atomic per slot and block on the scratch (the
// blocks' atomics on one word follow one another, so the grid is a few large
// blocks: the launcher gives it at most MI_CLS_RUN_GRID of them).
#define RUN_FIN_THREADS 1024
__global__ __launch_bounds__(RUN_FIN_THREADS) void mi_cls_run_finish_kernel(RunArgs a)
{
	__shared__ unsigned long long s_need[MI_CLS_RUN_VSLOTS + 1];   // the last: all slots
	const uint32_t t = threadIdx.x;
	const uint32_t nruns = min(a.tot[1], a.n), total = a.tot[0];
	if (t <= MI_CLS_RUN_VSLOTS)
		s_need[t] = 0ull;
	__syncthreads();
	const unsigned long long stride = (unsigned long long)gridDim.x * RUN_FIN_THREADS;
	for (unsigned long long r = (unsigned long long)blockIdx.x * RUN_FIN_THREADS + t; r < nruns; r += stride) {
		const uint2 h = a.head[r];
		const uint32_t next = r + 1u < nruns ? a.head[r + 1u].x : total;
		const uint32_t count = next - h.x;
		const uint32_t cos = h.y & 0xFFu, dst = h.y >> 8;
		const uint32_t mode = a.rtab->mode[cos], vmax = a.rtab->vmax[cos];
		const bool vec = count >= 2u && (mode & MI_CLS_RUN_VEC) != 0u && vmax != 0u;
		const uint32_t nvec = vec ? (count - 1u) / vmax + 1u : 0u;
		const uint32_t flags = vec ? MI_CLS_RUN_VEC : (mode & MI_CLS_RUN_AGGR);
		if (r < a.run_cap)
			reinterpret_cast<uint4 *>(a.runs)[r] = make_uint4(h.x, count, dst | cos << 16 | flags << 24, nvec);
		if (nvec) {
			atomicAdd(&s_need[a.rtab->vslot[cos] & (MI_CLS_RUN_VSLOTS - 1u)], (unsigned long long)nvec);
			atomicAdd(&s_need[MI_CLS_RUN_VSLOTS], (unsigned long long)nvec);
		}
	}
	__syncthreads();
	if (t <= MI_CLS_RUN_VSLOTS && s_need[t])
		atomicAdd(&a.ctr[t < MI_CLS_RUN_VSLOTS ? RUN_CTR_NEED + t : RUN_CTR_VECTORS], s_need[t]);
}

__global__ __launch_bounds__(WAVE) void mi_cls_run_out_kernel(RunArgs a)
{
	if (threadIdx.x < RUN_NOUT)
		reinterpret_cast<uint64_t *>(a.out)[threadIdx.x] = a.ctr[threadIdx.x];
}

#endif /* MI_CLS_RUN_DEV_H_ */
