// mi_cls_vec_dev.h -- the vector fill's kernels (mi_cls_vec_fill, mi_cls.h):
// a planned batch's event arrays and packet vectors.  The run count and the
// delivered count are read from the run plan's out by every launch, so the
// host needs neither.  Every step is a launch of its own on the stream; no
// block waits for another one:
//
//   count   block b walks its run of tiles of runs: per vector slot the sum of
//           nvec over its vector runs, and the sum of its event places (count
//           of a plain run, nvec of a vector run), to column b of a matrix of
//           MI_CLS_RUN_VSLOTS + 1 rows -- at most 17 x MI_CLS_VEC_GRID words,
//           so the next launch sums its own prefix and there is no scan launch;
//   place   block b: wave w sums row w over the earlier blocks (coalesced
//           loads, a shuffle reduction; wave 0 the event row too), then the
//           block walks the same runs: a run's rank in its slot and its first
//           event place are weighted prefix sums -- in the wave one
//           wave_scan_add per distinct slot present (the lanes of the other
//           slots add 0) and one for the event places, across the waves and
//           tiles through LDS.  It writes evr[r] as one 16-byte store and
//           keeps ev_first, g, vfirst and the clamped count in the scratch;
//   fill    parallel over the delivered places, not the runs, so that one run
//           of the whole batch and a batch of runs of one packet both spread
//           over the grid.  A block finds the run that owns its first place by
//           one binary search over runs[].first; per tile the run heads inside
//           it mark their place in LDS and a running maximum gives every place
//           its run.  Each thread then does the double gather ent[seq[p]] and
//           one 8-byte store, to ev or to a vector's table; the thread of a
//           vector's first packet also writes its size and its ev entry.  Lost
//           packets are appended with one atomic per wave;
//   finish  one block, wave w summing row w whole: the counters, the event
//           span and vec_used to out by plain stores.
//
// Bounds: runs[] and evr[] are indexed below min(nruns, run_cap, n); seq and
// ev below n; a seq value is checked against n before it indexes ent; a vgot
// index against nvgot; a vector's address against the arena with its table's
// end (vec_ok); a lost place against n.  A plan that is not the run plan's
// (overlapping runs, counts that do not add up) gives unspecified values
// inside those bounds.
#ifndef MI_CLS_VEC_DEV_H_
#define MI_CLS_VEC_DEV_H_

#include "mi_cls_dev.h"

#define VEC_THREADS MI_CLS_VEC_TILE          // one run or one place per thread and tile
#define VEC_WAVES (VEC_THREADS / WAVE)
#define VEC_ROWS (MI_CLS_RUN_VSLOTS + 1u)    // the slots and the event places
#define VEC_EV MI_CLS_RUN_VSLOTS             // the event places' row
#define VEC_NONE 0xFFFFFFFFu
#define VEC_AHEAD 4u                         // tiles whose loads a block issues together
#define VEC_NOUT 24u                         // the words of mi_cls_vec_out_t
#define VEC_CTR_EVENTS 0u                    // the scratch counters
#define VEC_CTR_VECTORS 1u
#define VEC_CTR_IN_VECTORS 2u
#define VEC_CTR_LOST 3u
#define VEC_CTR_HOLES 4u
#define VEC_CTR_REFUSED 5u
#define VEC_NCTR 8u
static_assert(sizeof(mi_cls_vec_out_t) == VEC_NOUT * sizeof(uint64_t), "24 64-bit words");
static_assert(sizeof(mi_cls_evrun_t) == 16 && sizeof(mi_cls_run_t) == 16, "one 16-B load and store each");
static_assert(VEC_THREADS == 1024 && VEC_WAVES == MI_CLS_RUN_VSLOTS, "wave w sums slot w's row");
static_assert(VEC_WAVES * VEC_ROWS <= VEC_THREADS, "a thread per (wave, row)");

// What every launch reads from the run plan's out
struct VecPlan {
	uint32_t nr;     // runs to work on: min(nruns, run_cap, n)
	uint32_t dlv;    // delivered places: min(delivered, n)
	bool trunc;      // nruns > run_cap: nothing is written but out
};

__device__ __forceinline__ VecPlan vec_plan(const VecArgs &a)
{
	const unsigned long long nruns = a.rout->nruns, d = a.rout->delivered;
	const uint32_t cap = min(a.run_cap, a.n);
	VecPlan p;
	p.trunc = nruns > a.run_cap;
	p.nr = nruns < cap ? (uint32_t)nruns : cap;
	p.dlv = d < a.n ? (uint32_t)d : a.n;
	return p;
}

// A run as the kernels use it
struct VecRun {
	uint32_t cnt;    // count, clamped to the delivered places from first on
	uint32_t slot, vm;
	uint32_t nvec;   // 0 for a plain run
	uint32_t we;     // its event places
	bool vec;
};

__device__ __forceinline__ VecRun vec_run(uint4 r, uint32_t dlv, const uint16_t *s_vmax, const uint8_t *s_vslot)
{
	VecRun v;
	const uint32_t cos = (r.z >> 16) & 0xFFu;
	v.cnt = r.x < dlv ? min(r.y, dlv - r.x) : 0u;
	v.vec = ((r.z >> 24) & MI_CLS_RUN_VEC) != 0u;
	v.slot = s_vslot[cos] & (MI_CLS_RUN_VSLOTS - 1u);
	v.vm = max((uint32_t)s_vmax[cos], 1u);
	v.nvec = v.vec ? r.w : 0u;
	v.we = v.vec ? r.w : v.cnt;
	return v;
}

// The run of tiles of block b under `tpb` tiles per block: [lo, hi) of `total`
__device__ __forceinline__ void vec_span(uint32_t tpb, uint32_t total, uint32_t &lo, uint32_t &hi)
{
	const unsigned long long per = (unsigned long long)tpb * VEC_THREADS;
	const unsigned long long l = per * blockIdx.x;
	lo = (uint32_t)(l < total ? l : total);
	hi = (uint32_t)(l + per < total ? l + per : total);
}

// The run table's device copy to LDS (the whole block; the caller's barrier follows)
__device__ __forceinline__ void vec_tab_lds(const VecArgs &a, uint16_t *s_vmax, uint8_t *s_vslot)
{
	const uint32_t t = threadIdx.x;
	if (t < 256u) {
		s_vmax[t] = a.rtab->vmax[t];
		s_vslot[t] = a.rtab->vslot[t];
	}
}

// vhave[] / vbase[] from the launch arguments to LDS by constant indexes, as
// pool_args_lds does
__device__ __forceinline__ void vec_args_lds(const VecArgs &a, uint32_t *s_have, uint32_t *s_first)
{
#pragma unroll
	for (uint32_t s = 0; s < MI_CLS_RUN_VSLOTS; ++s)
		if (threadIdx.x == s) {
			s_have[s] = a.vhave[s];
			s_first[s] = a.vbase[s];
		}
}

__global__ __launch_bounds__(VEC_THREADS) void mi_cls_vec_count_kernel(VecArgs a)
{
	__shared__ uint16_t s_vmax[256];
	__shared__ uint8_t s_vslot[256];
	__shared__ uint32_t s_sum[VEC_ROWS];
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1);
	const VecPlan p = vec_plan(a);
	if (p.trunc)
		return;
	vec_tab_lds(a, s_vmax, s_vslot);
	if (t < VEC_ROWS)
		s_sum[t] = 0u;
	__syncthreads();
	uint32_t lo, hi;
	vec_span(a.tpb, p.nr, lo, hi);
	uint32_t evs = 0;
	for (unsigned long long base = lo; base < hi; base += VEC_AHEAD * VEC_THREADS) {
		uint4 ra[VEC_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < VEC_AHEAD; ++u) {
			const unsigned long long r = base + u * VEC_THREADS + t;
			ra[u] = reinterpret_cast<const uint4 *>(a.runs)[r < hi ? r : hi - 1u];
		}
#pragma unroll
		for (uint32_t u = 0; u < VEC_AHEAD; ++u) {
			const unsigned long long r = base + u * VEC_THREADS + t;
			if (r < hi) {
				const VecRun v = vec_run(ra[u], p.dlv, s_vmax, s_vslot);
				evs += v.we;
				if (v.nvec)
					atomicAdd(&s_sum[v.slot], v.nvec);
			}
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		evs += (uint32_t)__shfl_xor((int)evs, o);
	if (lane == 0 && evs)
		atomicAdd(&s_sum[VEC_EV], evs);
	__syncthreads();
	if (t < VEC_ROWS)
		a.mat[t * a.grid + blockIdx.x] = s_sum[t];
}

// Row `row` of the matrix summed over the blocks [0, nb): every lane of the
// wave gets the sum.  Loads of 64 consecutive words.
__device__ __forceinline__ uint32_t vec_row_sum(const VecArgs &a, uint32_t row, uint32_t lane, uint32_t nb)
{
	uint32_t s = 0;
	for (uint32_t b = lane; b < nb; b += WAVE)
		s += a.mat[row * a.grid + b];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		s += (uint32_t)__shfl_xor((int)s, o);
	return s;
}

__global__ __launch_bounds__(VEC_THREADS) void mi_cls_vec_place_kernel(VecArgs a)
{
	__shared__ uint16_t s_vmax[256];
	__shared__ uint8_t s_vslot[256];
	__shared__ uint32_t s_have[MI_CLS_RUN_VSLOTS], s_first[MI_CLS_RUN_VSLOTS];
	__shared__ uint32_t s_base[2][VEC_ROWS];             // each row's sum before the tile
	__shared__ uint32_t s_wc[VEC_WAVES * VEC_ROWS];      // per wave and row: the tile's sum
	__shared__ uint32_t s_ws[VEC_WAVES * VEC_ROWS];      // per wave and row: the sum before the wave
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	const VecPlan p = vec_plan(a);
	if (p.trunc)
		return;
	vec_tab_lds(a, s_vmax, s_vslot);
	vec_args_lds(a, s_have, s_first);
	{
		const uint32_t nb = min(blockIdx.x, a.grid);
		const uint32_t s = vec_row_sum(a, wave, lane, nb);
		if (lane == 0)
			s_base[0][wave] = s;
		if (wave == 0) {
			const uint32_t e = vec_row_sum(a, VEC_EV, lane, nb);
			if (lane == 0)
				s_base[0][VEC_EV] = e;
		}
	}
	__syncthreads();
	uint32_t lo, hi, par = 0;
	vec_span(a.tpb, p.nr, lo, hi);
	uint32_t *wc = s_wc + wave * VEC_ROWS;
	unsigned long long events = 0;
	for (unsigned long long base = lo; base < hi; base += VEC_AHEAD * VEC_THREADS) {
		uint4 ra[VEC_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < VEC_AHEAD; ++u) {
			const unsigned long long r = base + u * VEC_THREADS + t;
			ra[u] = reinterpret_cast<const uint4 *>(a.runs)[r < hi ? r : hi - 1u];
		}
#pragma unroll
		for (uint32_t u = 0; u < VEC_AHEAD; ++u) {
			const unsigned long long r = base + u * VEC_THREADS + t;
			if (base + u * VEC_THREADS >= hi)   // the whole block: no tile left
				break;
			const bool in = r < hi;
			VecRun v = vec_run(ra[u], p.dlv, s_vmax, s_vslot);
			if (!in) {
				v.vec = false;
				v.nvec = v.we = v.cnt = 0u;
			}
			// the wave's own LDS accesses are in order: no barrier between the
			// zeroing and the sums
			if (lane < VEC_ROWS)
				wc[lane] = 0u;
			// the vectors of the wave's earlier runs of this lane's slot: one
			// scan per distinct slot among the wave's vector runs
			uint32_t inrank = 0u;
			unsigned long long todo = __ballot(v.nvec != 0u);
			while (todo) {
				const uint32_t s = (uint32_t)__shfl((int)v.slot, __ffsll((long long)todo) - 1);
				const bool mine = v.nvec != 0u && v.slot == s;
				const uint32_t incl = wave_scan_add(mine ? v.nvec : 0u, lane);
				if (mine)
					inrank = incl - v.nvec;
				if (lane == WAVE - 1u)
					wc[s] = incl;
				todo &= ~__ballot(mine);
			}
			const uint32_t eincl = wave_scan_add(v.we, lane);
			if (lane == WAVE - 1u)
				wc[VEC_EV] = eincl;
			__syncthreads();
			// thread (w, s): row s's sum before wave w of the tile; wave 15's also
			// the sum after the tile (the other row of s_base: this one is still
			// being read)
			if (t < VEC_WAVES * VEC_ROWS) {
				const uint32_t w = t / VEC_ROWS, s = t % VEC_ROWS;
				uint32_t acc = s_base[par][s];
				for (uint32_t x = 0; x < w; ++x)
					acc += s_wc[x * VEC_ROWS + s];
				s_ws[t] = acc;
				if (w == VEC_WAVES - 1u)
					s_base[par ^ 1u][s] = acc + s_wc[t];
			}
			__syncthreads();
			par ^= 1u;
			if (in) {
				const uint32_t ev_first = s_ws[wave * VEC_ROWS + VEC_EV] + eincl - v.we;
				uint32_t g = 0u, vfirst = VEC_NONE, ev_count = v.cnt, pk = v.cnt;
				if (v.vec) {
					const uint32_t rank = s_ws[wave * VEC_ROWS + v.slot] + inrank;
					const uint32_t have = s_have[v.slot];
					g = rank < have ? min(v.nvec, have - rank) : 0u;
					if (g)
						vfirst = s_first[v.slot] + rank;
					ev_count = g;
					const unsigned long long room = (unsigned long long)g * v.vm;
					pk = room < v.cnt ? (uint32_t)room : v.cnt;
				}
				reinterpret_cast<uint4 *>(a.evr)[r] = make_uint4(ev_first, ev_count, pk, vfirst);
				a.pl[r] = make_uint4(ev_first, g, vfirst, v.cnt);
				events += ev_count;
			}
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		events += __shfl_xor(events, o);
	if (lane == 0 && events)
		atomicAdd(&a.ctr[VEC_CTR_EVENTS], events);
}

// Vector v with a table of `size` entries lies in the arena, whole
__device__ __forceinline__ bool vec_ok(const VecArgs &a, uint64_t v, uint32_t size)
{
	const uint64_t need = (uint64_t)a.tbl_off + 8ull * size;
	return v != 0ull && (v & 7ull) == 0ull && v >= a.varena_lo && need <= a.varena_bytes &&
	       v - a.varena_lo <= a.varena_bytes - need;
}

__global__ __launch_bounds__(VEC_THREADS) void mi_cls_vec_fill_kernel(VecArgs a)
{
	__shared__ uint16_t s_vmax[256];
	__shared__ uint32_t s_head[VEC_THREADS];   // the run whose head is at this place of the tile, 0: none
	__shared__ uint32_t s_wm[VEC_WAVES];       // per wave: the last run that begins in it
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
	const VecPlan p = vec_plan(a);
	if (p.trunc || p.nr == 0u)
		return;
	if (t < 256u)
		s_vmax[t] = a.rtab->vmax[t];
	uint32_t lo, hi;
	vec_span(a.ftpb, p.dlv, lo, hi);
	if (lo >= hi)   // the whole block
		return;
	// the last run that begins at or before the block's first place (run 0 when
	// none does: its places then fail the test against the run below)
	uint32_t cur;
	{
		uint32_t l = 0u, h = p.nr;
		while (l < h) {
			const uint32_t m = l + (h - l) / 2u;
			if (a.runs[m].first <= lo)
				l = m + 1u;
			else
				h = m;
		}
		cur = l ? l - 1u : 0u;
	}
	uint32_t vectors = 0, in_vectors = 0, holes = 0, refused = 0;
	for (unsigned long long base = lo; base < hi; base += VEC_AHEAD * VEC_THREADS) {
		uint32_t sa[VEC_AHEAD];
#pragma unroll
		for (uint32_t u = 0; u < VEC_AHEAD; ++u) {
			const unsigned long long q = base + u * VEC_THREADS + t;
			sa[u] = a.seq[q < hi ? q : hi - 1u];
		}
#pragma unroll
		for (uint32_t u = 0; u < VEC_AHEAD; ++u) {
			const unsigned long long tb = base + u * VEC_THREADS;
			if (tb >= hi)   // the whole block: no tile left
				break;
			const unsigned long long q = tb + t;
			const bool in = q < hi;
			// the runs after `cur` whose heads lie in this tile mark them: at most
			// one per place, so they are among the next VEC_THREADS runs
			s_head[t] = 0u;
			__syncthreads();
			{
				const unsigned long long rr = (unsigned long long)cur + 1u + t;
				if (rr < p.nr) {
					const uint32_t f = a.runs[rr].first;
					if (f >= tb && f - tb < VEC_THREADS)
						atomicMax(&s_head[(uint32_t)(f - tb)], (uint32_t)rr);
				}
			}
			__syncthreads();
			// every place's run: the running maximum of the marks (run indexes
			// grow with the place), from `cur` on
			uint32_t r = s_head[t];
#pragma unroll
			for (uint32_t o = 1; o < WAVE; o <<= 1) {
				const uint32_t y = (uint32_t)__shfl_up((int)r, o);
				r = lane >= o ? max(r, y) : r;
			}
			if (lane == WAVE - 1u)
				s_wm[wave] = r;
			__syncthreads();
			r = max(r, cur);
			for (uint32_t w = 0; w < VEC_WAVES; ++w) {
				const uint32_t m = s_wm[w];
				if (w < wave)
					r = max(r, m);
				cur = max(cur, m);
			}
			uint64_t h = 0ull;
			bool wrote = false, lostp = false;
			if (in) {
				const uint4 R = reinterpret_cast<const uint4 *>(a.runs)[r];
				const uint4 P = a.pl[r];   // ev_first, g, vfirst, the clamped count
				const uint32_t o = (uint32_t)q - R.x;
				if ((uint32_t)q >= R.x && o < P.w) {
					const uint32_t i = sa[u];
					const uint64_t e = i < a.n ? a.ent[i] : 0ull;
					h = e ? e - a.ent_to_handle : 0ull;
					if (((R.z >> 24) & MI_CLS_RUN_VEC) == 0u) {
						const uint32_t at = P.x + o;
						if (at >= P.x && at < a.n) {
							a.ev[at] = h;
							wrote = true;
						}
					} else {
						const uint32_t vm = max((uint32_t)s_vmax[(R.z >> 16) & 0xFFu], 1u);
						const uint32_t k = o / vm, j = o - k * vm;
						const uint32_t at = P.x + k;
						const bool evw = j == 0u && k < R.w && at >= P.x && at < a.n;
						if (k < P.y) {
							const uint32_t vi = P.z + k;
							const uint32_t size = min(vm, P.w - k * vm);
							const uint64_t v = vi >= P.z && vi < a.nvgot ? a.vgot[vi] : 0ull;
							const bool ok = vec_ok(a, v, size);
							if (ok) {
								*reinterpret_cast<uint64_t *>(v + a.tbl_off + 8ull * j) = h;
								wrote = true;
								++in_vectors;
								if (j == 0u) {
									*reinterpret_cast<uint32_t *>(v + a.size_off) = size;
									++vectors;
								}
							}
							if (j == 0u && !ok)
								++refused;
							if (evw)
								a.ev[at] = ok ? v : 0ull;
						} else {
							lostp = true;
							if (evw)
								a.ev[at] = 0ull;
						}
					}
				}
			}
			// the wave's lost packets: one atomic, places by ballot ranks
			const unsigned long long lm = __ballot(lostp);
			if (lm) {
				unsigned long long lb = 0ull;
				if (lane == 0u)
					lb = atomicAdd(&a.ctr[VEC_CTR_LOST], (unsigned long long)__popcll(lm));
				lb = __shfl(lb, 0);
				const unsigned long long at = lb + (uint32_t)__popcll(lm & below);
				if (lostp && at < a.n) {
					a.lost[at] = h;
					wrote = true;
				}
			}
			holes += wrote && h == 0ull ? 1u : 0u;
		}
	}
	uint32_t c[4] = { vectors, in_vectors, holes, refused };
	const uint32_t where[4] = { VEC_CTR_VECTORS, VEC_CTR_IN_VECTORS, VEC_CTR_HOLES, VEC_CTR_REFUSED };
#pragma unroll
	for (uint32_t j = 0; j < 4u; ++j) {
#pragma unroll
		for (int o = 32; o > 0; o >>= 1)
			c[j] += (uint32_t)__shfl_xor((int)c[j], o);
		if (lane == 0 && c[j])
			atomicAdd(&a.ctr[where[j]], (unsigned long long)c[j]);
	}
}

// One block; wave w sums row w of the matrix whole (wave 0 the event row too),
// as the pool plan's finish does.  n == 0: out is zeroed and nothing is read.
__global__ __launch_bounds__(VEC_THREADS) void mi_cls_vec_finish_kernel(VecArgs a)
{
	__shared__ uint32_t s_row[VEC_ROWS];
	__shared__ uint32_t s_have[MI_CLS_RUN_VSLOTS], s_first[MI_CLS_RUN_VSLOTS];
	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	uint64_t *out = reinterpret_cast<uint64_t *>(a.out);
	if (a.n == 0u) {
		if (t < VEC_NOUT)
			out[t] = 0ull;
		return;
	}
	const VecPlan p = vec_plan(a);
	if (p.trunc) {
		if (t < VEC_NOUT)
			out[t] = t == 7u ? 1ull : 0ull;
		return;
	}
	vec_args_lds(a, s_have, s_first);
	{
		const uint32_t nb = min(a.grid, (uint32_t)MI_CLS_VEC_GRID);
		const uint32_t s = vec_row_sum(a, wave, lane, nb);
		if (lane == 0)
			s_row[wave] = s;
		if (wave == 0) {
			const uint32_t e = vec_row_sum(a, VEC_EV, lane, nb);
			if (lane == 0)
				s_row[VEC_EV] = e;
		}
	}
	__syncthreads();
	if (t < VEC_NOUT) {
		const unsigned long long v =
			t == 0u ? a.ctr[VEC_CTR_EVENTS] : t == 1u ? s_row[VEC_EV] : t == 2u ? a.ctr[VEC_CTR_VECTORS] :
			t == 3u ? a.ctr[VEC_CTR_IN_VECTORS] : t == 4u ? a.ctr[VEC_CTR_LOST] :
			t == 5u ? a.ctr[VEC_CTR_HOLES] : t == 6u ? a.ctr[VEC_CTR_REFUSED] : t == 7u ? 0ull :
			min(s_row[t - 8u], s_have[t - 8u]);
		out[t] = v;
	}
}

#endif /* MI_CLS_VEC_DEV_H_ */
