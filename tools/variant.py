#!/usr/bin/env python3
"""Measurement variants of the classification kernel (test tooling, never a
shipped build).

A variant is a named list of text patches applied to a copy of
odp_amd/csrc/mi_cls_dev.h (and optional -D defines); the patched copy is
built into variants/<name>/ with odp_amd._build, so the product header keeps
no experiment switches and hipRTC compiles only product code.  Time a
variant against the shipped library with tools/ab.py --libs odp_amd,variants/<name>.

  python tools/variant.py NAME [NAME...]      build (MI_CLS_ONLY limits the
                                              kernel translation units)
  python tools/variant.py --list

Variants:
  stageonly   windows staged and a record written per packet, no parse or
              classification (the staging floor; records are wrong)
  parseonly   stage + parse, no classification (records are wrong)
  ts          the full kernel plus per-wave s_memrealtime stamps (kernel
              entry, setup done, first and last tile window landed, end),
              written over the records of each wave's first tile
              (tools/ts_probe.py decodes them; records are wrong there)
  stagenostore  stageonly without the record stores (records are not written)
  tsp         ts plus the last tile's parse-done and descent-done stamps
  tsd         the receive decide kernel prints its phase times per burst
"""
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_AFTER_SYNC = """		if constexpr (!PLH)
			prefetch();
		wave_lds_sync();
"""

PATCHES = {
    "stageonly": [(_AFTER_SYNC, _AFTER_SYNC + """		if constexpr (PLH)
			prefetch();
		if (valid) {
			uint4 rec;
			rec.x = W[3 * RS + lane] ^ W[8 * RS + lane];
			rec.y = my_len;
			rec.z = 0;
			rec.w = 0;
			*(uint4 *)(a.out + pi) = rec;
		}
		continue;
""")],
    "parseonly": [("""		// ---- select the starting CoS (cls_select_cos, odp_classification.c:1694-1726)
""", """		if (valid) {
			uint4 rec;
			rec.x = p.flags;
			rec.y = p.err;
			rec.z = x.f ^ x.l4;
			rec.w = (p.l3 & 0xffffu) | ((p.l4 & 0xffffu) << 16);
			*(uint4 *)(a.out + pi) = rec;
		}
		continue;
		// ---- select the starting CoS (cls_select_cos, odp_classification.c:1694-1726)
""")],
    "ts": [
        ("""	const uint32_t wave = threadIdx.x >> 6;
	uint32_t *W = s_win + wave * RS * WROWS;
""", """	const uint32_t wave = threadIdx.x >> 6;
	uint32_t *W = s_win + wave * RS * WROWS;
	const uint64_t ts0 = __builtin_amdgcn_s_memrealtime();
"""),
        ("""	uint4 prev_rec = make_uint4(0, 0, 0, 0);
	uint32_t prev_pi = 0;
""", """	const uint64_t ts1 = __builtin_amdgcn_s_memrealtime();
	uint64_t ts2 = 0, ts3 = 0;
	uint32_t ntl = 0;
	uint4 prev_rec = make_uint4(0, 0, 0, 0);
	uint32_t prev_pi = 0;
"""),
        ("""		zero_tail(W, lane, my_len);   // same wave: LDS stores stay in order
""", """		zero_tail(W, lane, my_len);   // same wave: LDS stores stay in order
		{
			const uint64_t t = __builtin_amdgcn_s_memrealtime();
			ts2 = ntl == 0u ? t : ts2;
			ts3 = t;
			++ntl;
		}
"""),
        ("""	if (prev_valid)
		store_rec(out_rs, prev_pi, prev_rec);
	// the waves of block 0""", """	if (prev_valid)
		store_rec(out_rs, prev_pi, prev_rec);
	{
		const uint64_t ts4 = __builtin_amdgcn_s_memrealtime();
		const uint32_t t0 = blockIdx.x * NW + wave;
		const uint64_t v = lane == 0 ? ts0 : lane == 1 ? ts1 : lane == 2 ? ts2 : lane == 3 ? ts3 : ts4;
		if (lane < 5u && t0 * WAVE + lane < a.n) {
			uint4 r;
			r.x = (uint32_t)v;
			r.y = (uint32_t)(v >> 32);
			// HW_ID (wave / SIMD / CU / SH / SE) and XCC_ID: s_getreg ids 4, 20
			const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
			const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
			r.z = ntl | ((hw >> 8) & 0xFFFFu) << 8 | (xcc & 0xFu) << 24 | ((hw >> 4) & 3u) << 28;
			r.w = blockIdx.x | (wave << 24);
			*(uint4 *)(a.out + t0 * WAVE + lane) = r;
		}
	}
	// the waves of block 0"""),
    ],
}
# stagenostore: stageonly without the per-packet record stores (a store
# that never happens keeps the loads live): what the stores cost the stream
PATCHES["stagenostore"] = [(PATCHES["stageonly"][0][0], PATCHES["stageonly"][0][1].replace(
    "		if (valid) {", "		if (valid && (W[3 * RS + lane] ^ W[8 * RS + lane]) == 0x9e3779b9u + my_len) {"))]
# prio: the next tile's loads issued at raised wave priority (s_setprio 2
# around prefetch), so a wave about to issue loads is served before the
# others' compute
PATCHES["prio"] = [("""		if constexpr (!PLH)
			prefetch();
		wave_lds_sync();
""", """		if constexpr (!PLH) {
			__builtin_amdgcn_s_setprio(2);
			prefetch();
			__builtin_amdgcn_s_setprio(0);
		}
		wave_lds_sync();
""")]
PATCHES["prio1"] = [(PATCHES["prio"][0][0], PATCHES["prio"][0][1].replace("s_setprio(2)", "s_setprio(1)"))]
# priority only around the window loads of the next tile
PATCHES["priowin"] = [("""			if (nx < nt)
				d_hi = load_window(rs, d_off, d_len, lane, d, want_hi, d_win);
		};""", """			if (nx < nt) {
				__builtin_amdgcn_s_setprio(2);
				d_hi = load_window(rs, d_off, d_len, lane, d, want_hi, d_win);
				__builtin_amdgcn_s_setprio(0);
			}
		};""")]
# priority raised for the whole tile's compute once its windows are in LDS
# (older tiles first), dropped before the next tile's loads
PATCHES["priocomp"] = [("""		wave_lds_sync();   // previous tile's window reads are done
		store_window(W, lane, d, d_hi, hi_rows);""", """		__builtin_amdgcn_s_setprio(0);
		wave_lds_sync();   // previous tile's window reads are done
		store_window(W, lane, d, d_hi, hi_rows);"""),
    ("""		if constexpr (!PLH)
			prefetch();
		wave_lds_sync();
""", """		if constexpr (!PLH)
			prefetch();
		__builtin_amdgcn_s_setprio(2);
		wave_lds_sync();
""")]
# priority for the next tile's loads only when its frames are longer than
# the window (scattered windows; a tile of back-to-back short frames reads
# contiguous bytes and keeps default priority)
PATCHES["priolong"] = [("""		if constexpr (!PLH)
			prefetch();
		wave_lds_sync();
""", """		if constexpr (!PLH) {
			const bool pri = __ballot(n_len > 64u) != 0ull;
			if (pri)
				__builtin_amdgcn_s_setprio(2);
			prefetch();
			if (pri)
				__builtin_amdgcn_s_setprio(0);
		}
		wave_lds_sync();
""")]
# round-6 follow-ups of the shipped load priority (mi_cls_kernel prefetch_pri)
PATCHES["prio3"] = [("""				if (pri)
					__builtin_amdgcn_s_setprio(2);""", """				if (pri)
					__builtin_amdgcn_s_setprio(3);""")]
# raised from the top of the iteration (window store, record store) through
# the prefetch
PATCHES["priotop"] = [("""		wave_lds_sync();   // previous tile's window reads are done
		store_window(W, lane, d, d_hi, hi_rows);""", """		if constexpr (!CK && !PLH) {
			if (__ballot(n_len > 64u) != 0ull)
				__builtin_amdgcn_s_setprio(2);
		}
		wave_lds_sync();   // previous tile's window reads are done
		store_window(W, lane, d, d_hi, hi_rows);""")]
# tree kernels: the far pieces' loads (bytes 64..95) at raised priority too
PATCHES["priofar"] = [("""			any_h = __ballot(hneed) != 0ull;
			if (any_h) {""", """			any_h = __ballot(hneed) != 0ull;
			if (any_h)
				__builtin_amdgcn_s_setprio(3);
			if (any_h) {""")]
# option kernels: each checksum round's piece loads at raised priority
PATCHES["priock"] = [
    ("""			u32x4 v[CK_HALVES][4];
			uint32_t xh[CK_HALVES], xt[CK_HALVES];
#pragma unroll
			for (uint32_t h = 0; h < CK_HALVES; ++h) {""", """			u32x4 v[CK_HALVES][4];
			uint32_t xh[CK_HALVES], xt[CK_HALVES];
			__builtin_amdgcn_s_setprio(3);
#pragma unroll
			for (uint32_t h = 0; h < CK_HALVES; ++h) {"""),
    ("""					rs, pt ? ob[h] + (uint32_t)(hb[h] & ~3) : OOB_OFF, 0, 0);
			}""", """					rs, pt ? ob[h] + (uint32_t)(hb[h] & ~3) : OOB_OFF, 0, 0);
			}
			__builtin_amdgcn_s_setprio(0);"""),
    ("""		u32x4 v[4];
#pragma unroll
		for (uint32_t i = 0; i < 4; ++i) {
			const uint32_t o = o0 + 16u * i;""", """		u32x4 v[4];
		__builtin_amdgcn_s_setprio(3);
#pragma unroll
		for (uint32_t i = 0; i < 4; ++i) {
			const uint32_t o = o0 + 16u * i;"""),
    ("""				rs, (live && b != 0u && o < flen && o + 16u > fl4) ? ob0 + o : OOB_OFF, 0, 0);
		}""", """				rs, (live && b != 0u && o < flen && o + 16u > fl4) ? ob0 + o : OOB_OFF, 0, 0);
		}
		__builtin_amdgcn_s_setprio(0);"""),
]
# tsp: ts plus the last tile's compute phases (parse done, descent done)
# in lanes 5 and 6 of the stamp block
PATCHES["tsp"] = PATCHES["ts"][:3] + [
    ("""		// ---- select the starting CoS (cls_select_cos, odp_classification.c:1694-1726)
""", """		ts5 = __builtin_amdgcn_s_memrealtime();
		// ---- select the starting CoS (cls_select_cos, odp_classification.c:1694-1726)
"""),
    ("""		// ---- final CoS -> outcome / queue (_odp_cls_classify_packet, :1742-1771)
""", """		ts6 = __builtin_amdgcn_s_memrealtime();
		// ---- final CoS -> outcome / queue (_odp_cls_classify_packet, :1742-1771)
"""),
    ("""	uint64_t ts2 = 0, ts3 = 0;
""", """	uint64_t ts2 = 0, ts3 = 0, ts5 = 0, ts6 = 0;
"""),
    (PATCHES["ts"][3][0], PATCHES["ts"][3][1]
     .replace("lane == 3 ? ts3 : ts4", "lane == 3 ? ts3 : lane == 4 ? ts4 : lane == 5 ? ts5 : ts6")
     .replace("lane < 5u && t0 * WAVE + lane < a.n", "lane < 7u && t0 * WAVE + lane < a.n")),
]
# tsd: the receive decide kernel prints its phase times (s_memrealtime,
# 10 ns ticks from entry: loads + table in LDS, slot ranks, counters, queue
# groups, end) from thread 0 of every burst of 4096 frames
_KD = "mi_cls_kd.hip"
PATCHES["tsd"] = [
    (_KD, """	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	const mi_cls_rxtab_t &tab = *d.tab;""", """	const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
	const uint64_t q0 = __builtin_amdgcn_s_memrealtime();
	uint64_t q1 = 0, q2 = 0, q3 = 0, q4 = 0;
	const mi_cls_rxtab_t &tab = *d.tab;"""),
    (_KD, """	__syncthreads();
	// (1) each frame's fate and slot""", """	__syncthreads();
	q1 = __builtin_amdgcn_s_memrealtime();
	// (1) each frame's fate and slot"""),
    (_KD, """	__syncthreads();
	// (3) delivered or not, the counters, the queue group""", """	__syncthreads();
	q2 = __builtin_amdgcn_s_memrealtime();
	// (3) delivered or not, the counters, the queue group"""),
    (_KD, """	// (4) the stable permutation of the delivered frames by queue group, as""", """	q3 = __builtin_amdgcn_s_memrealtime();
	// (4) the stable permutation of the delivered frames by queue group, as"""),
    (_KD, """	// every output, after the last barrier""", """	q4 = __builtin_amdgcn_s_memrealtime();
	// every output, after the last barrier"""),
    (_KD, """		a.out->short_pool = sh;
	}""", """		a.out->short_pool = sh;
		if (n == 4096u)
			printf("TSD %u %u %u %u %u\\n", (uint32_t)(q1 - q0), (uint32_t)(q2 - q0), (uint32_t)(q3 - q0),
			       (uint32_t)(q4 - q0), (uint32_t)(__builtin_amdgcn_s_memrealtime() - q0));
	}"""),
]
# The record store's cache policy (store_rec; profiles/r08_edges_ab.txt).
# rec17: sc0 sc1 (auxiliary 17) instead of sc1.
_WT = "	__builtin_amdgcn_raw_buffer_store_b128(v, out_rs, pi * 16u, 0, 16);\n"
PATCHES["rec17"] = [(_WT, _WT.replace("0, 16)", "0, 17)"))]
# rectail: written through only once the wave's tile queue is exhausted (the
# records of its last two tiles: the ones still dirty in L2 when the launch
# ends); the tiles before them stay nontemporal
PATCHES["rectail"] = [
    ("""		if (prev_valid)
			store_rec(out_rs, prev_pi, prev_rec);
		prev_valid = false;
""", """		if (prev_valid) {
			if (nx < nt)
				store_rec(a.out + prev_pi, prev_rec);
			else
				store_rec(out_rs, prev_pi, prev_rec);
		}
		prev_valid = false;
""")]
DEFINES = {}


def build(name):
    if name not in PATCHES:
        raise SystemExit(f"unknown variant {name}: {', '.join(PATCHES)}")
    from odp_amd import _build
    src = tempfile.mkdtemp(prefix=f"variant_{name}_")
    try:
        for f in os.listdir(_build.SRC):
            shutil.copy(os.path.join(_build.SRC, f), src)
        for patch in PATCHES[name]:
            # (old, new) patches mi_cls_dev.h; (file, old, new) another source
            fn, old, new = patch if len(patch) == 3 else ("mi_cls_dev.h",) + tuple(patch)
            p = os.path.join(src, fn)
            with open(p) as f:
                text = f.read()
            if text.count(old) != 1:
                raise SystemExit(f"variant {name}: anchor not unique/absent in {fn}:\n{old}")
            with open(p, "w") as f:
                f.write(text.replace(old, new))
        out = os.path.join(ROOT, "variants", name)
        print(_build.build(force=True, out_dir=out, defines=DEFINES.get(name, ()), src_dir=src))
    finally:
        shutil.rmtree(src, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] == "--list":
        print("\n".join(PATCHES))
    else:
        for n in sys.argv[1:]:
            build(n)
