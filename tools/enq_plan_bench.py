#!/usr/bin/env python3
"""The enqueue plan (mi_cls_enq_plan) beside the classification it follows and
the host loop it replaces, on config 3's and config 5's records.

Per config, in one process: each step launches the classification and then the
plan of its records on the same stream, with a HIP event before, between and
after; the two spans are reported as median and min over the steps (after
warm-up steps), so both see the same clocks and the same cache state the
receive path would give them.  The plan's launches are timed together: its
steps are stream-ordered launches with no host work in between.

The host loop is a plain C per-record grouping of the same records (switch on
the outcome, the counters, the table lookup, one list per destination: a count
pass and a placing pass), compiled -O2, single thread, median of --host-runs
runs; its output is compared with the GPU's.

  python tools/enq_plan_bench.py [--n 1000000] [--steps 60] [--warmup 10] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_LOOP = r"""
#include <stdint.h>
#include <string.h>
#include "mi_cls.h"

static inline uint32_t key_of(const mi_cls_result_t *r, const mi_cls_enq_tab_t *t, mi_cls_enq_out_t *o,
			      uint16_t len)
{
	uint32_t key = t->ndst;

	if (r->err || r->outcome == MI_CLS_OUT_PARSE_DROP)
		o->in_errors++;
	switch (r->outcome) {
	case MI_CLS_OUT_DISCARD:
	case MI_CLS_OUT_LOOP:
		o->in_discards++;
		break;
	case MI_CLS_OUT_ENQ: {
		const uint32_t e = (uint32_t)t->cos_q0[r->cos] + r->queue;

		if (r->queue < t->cos_nq[r->cos] && e < MI_CLS_ENQ_ENT && t->ent_dst[e] < t->ndst) {
			key = t->ent_dst[e];
			o->delivered++;
			if (!r->err) {
				o->packets++;
				o->octets += len;
			}
		} else {
			o->stale++;
		}
		break;
	}
	default:
		break;
	}
	return key;
}

void host_plan(const mi_cls_result_t *res, const uint16_t *len, uint32_t n, const mi_cls_enq_tab_t *t,
	       uint32_t *perm, uint32_t *gbeg, mi_cls_enq_out_t *o, uint16_t *key, uint32_t *next)
{
	memset(o, 0, sizeof(*o));
	memset(gbeg, 0, (t->ndst + 2) * sizeof(*gbeg));
	for (uint32_t i = 0; i < n; i++) {
		key[i] = (uint16_t)key_of(&res[i], t, o, len[i]);
		gbeg[key[i] + 1]++;
	}
	for (uint32_t g = 0; g <= t->ndst; g++) {
		next[g] = gbeg[g];
		gbeg[g + 1] += gbeg[g];
	}
	for (uint32_t i = 0; i < n; i++)
		perm[next[key[i]]++] = i;
}
"""


def build_host_loop(tmp):
    src, so = os.path.join(tmp, "host_plan.c"), os.path.join(tmp, "host_plan.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP)
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           "-o", so, src])
    lib = C.CDLL(so)
    lib.host_plan.restype = None
    lib.host_plan.argtypes = [C.c_void_p] * 2 + [C.c_uint32] + [C.c_void_p] * 6
    return lib


def stats_us(ms):
    return {"us_median": round(1e3 * statistics.median(ms), 2), "us_min": round(1e3 * min(ms), 2),
            "us_max": round(1e3 * max(ms), 2)}


def run_config(torch, cfg, a, host):
    from odp_amd import rules as R
    from odp_amd.cls import ENQ_OUT_FIELDS, Classifier
    dev = torch.device("cuda:0")
    b, prog = R.CONFIGS[cfg](a.n)
    c = Classifier(gpu=0)
    try:
        c.apply(prog)
        c.spec_wait()
        tab, queues, _ = c.enq_table()
        n, ng = b.n, tab.ndst + 2
        t_buf = torch.from_numpy(np.ascontiguousarray(b.buf)).to(dev)
        t_off = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        t_res = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_perm = torch.empty(n, dtype=torch.int32, device=dev)
        t_gbeg = torch.empty(ng, dtype=torch.int32, device=dev)
        t_out = torch.empty(len(ENQ_OUT_FIELDS), dtype=torch.int64, device=dev)
        cur = torch.cuda.current_stream(dev)
        stream = cur.cuda_stream
        cls_ms, plan_ms = [], []
        evs = []
        for _ in range(a.warmup + a.steps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record(cur)
            rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_res.data_ptr(),
                                   stream)
            e[1].record(cur)
            k = c.last_launch()
            rc = rc or c.L.odp_amd_cls_enq_plan(c.pktio, t_res.data_ptr(), t_len.data_ptr(), n, C.byref(tab),
                                                t_perm.data_ptr(), t_gbeg.data_ptr(), t_out.data_ptr(), stream)
            e[2].record(cur)
            if rc:
                raise RuntimeError(f"launch failed: {rc}")
            evs.append(e)
        torch.cuda.synchronize(dev)
        for e in evs[a.warmup:]:
            cls_ms.append(e[0].elapsed_time(e[1]))
            plan_ms.append(e[1].elapsed_time(e[2]))
        info = (C.c_uint32 * 7)()
        c.L.odp_amd_cls_last_launch(c.pktio, info, 7)
        rec = t_res.cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE)
        perm = t_perm.cpu().numpy().view(np.uint32)
        gbeg = t_gbeg.cpu().numpy().view(np.uint32)
        out = t_out.cpu().numpy().view(np.uint64)
        # the host loop over the same records
        lens = np.ascontiguousarray(b.len, dtype=np.uint16)
        h_perm, h_gbeg = np.zeros(n, np.uint32), np.zeros(ng, np.uint32)
        h_out, h_key, h_next = np.zeros(6, np.uint64), np.zeros(n, np.uint16), np.zeros(ng, np.uint32)
        ts = []
        for _ in range(a.host_runs):
            t0 = time.perf_counter()
            host.host_plan(rec.ctypes.data, lens.ctypes.data, n, C.addressof(tab), h_perm.ctypes.data,
                           h_gbeg.ctypes.data, h_out.ctypes.data, h_key.ctypes.data, h_next.ctypes.data)
            ts.append(1e3 * (time.perf_counter() - t0))
        same = bool(np.array_equal(perm, h_perm) and np.array_equal(gbeg, h_gbeg) and np.array_equal(out, h_out))
        plan, cl, hl = stats_us(plan_ms), stats_us(cls_ms), stats_us(ts)
        return {"packets": n, "destinations": int(tab.ndst), "queues_used": int(np.count_nonzero(np.diff(gbeg[:-1]))),
                "counters": {k: int(v) for k, v in zip(ENQ_OUT_FIELDS, out)},
                "classify": dict(cl, kernel=k["name"], grid=k["grid"]),
                "plan": dict(plan, digit_passes=int(info[1]), grid=int(info[6]),
                             ns_per_packet_median=round(1e3 * plan["us_median"] / n, 3)),
                "host_loop": dict(hl, ns_per_packet_median=round(1e3 * hl["us_median"] / n, 3), runs=a.host_runs),
                "plan_over_classify_median": round(plan["us_median"] / cl["us_median"], 3),
                "host_loop_over_plan_median": round(hl["us_median"] / plan["us_median"], 1),
                "gpu_equals_host_loop": same}
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=9)
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch

    from odp_amd import _build
    _build.build()
    if not torch.cuda.is_available():
        raise SystemExit("enq_plan_bench: no GPU")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(prefix="enq_plan_bench_") as tmp:
        host = build_host_loop(tmp)
        for cfg in a.configs:
            res[f"config{cfg}"] = run_config(torch, cfg, a, host)
    s = json.dumps(res)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
