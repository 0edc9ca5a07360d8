#!/usr/bin/env python3
"""The run plan (mi_cls_enq_runs) beside the classification it follows and the
host loop it replaces, on config 3's and config 5's records.

Per config and burst size, in one process: each step launches the
classification and then the run plan of its records on the same stream, with a
HIP event before, between and after; the two spans are reported as median, min
and max over the steps (after warm-up steps).  The run plan's launches are
timed together: they are stream-ordered launches with no host work in between.
Every CoS delivers packet vectors of up to --vmax packets from one of four
vector pools (slot = CoS index & 3), so the finish step's vector sums run.

The host loop is a plain C per-record walk of the same records (the counters,
the table lookup, the delivered list, a run closed when the key changes or a
burst begins, the list of the rest appended), compiled -O2, single thread,
median of --host-runs runs; its seq, runs and out are compared with the GPU's.

  python tools/enq_runs_bench.py [--n 1000000] [--steps 60] [--warmup 10] [--out FILE]
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

static inline void close_run(mi_cls_run_t *r, uint32_t end, const mi_cls_run_tab_t *rt, mi_cls_run_out_t *o)
{
	const uint32_t mode = rt->mode[r->cos];

	r->count = end - r->first;
	if (r->count >= 2 && (mode & MI_CLS_RUN_VEC)) {
		r->flags = MI_CLS_RUN_VEC;
		r->nvec = (r->count - 1) / rt->vmax[r->cos] + 1;
		o->vectors += r->nvec;
		o->vec_need[rt->vslot[r->cos]] += r->nvec;
	} else {
		r->flags = (uint8_t)(mode & MI_CLS_RUN_AGGR);
		r->nvec = 0;
	}
}

void host_runs(const mi_cls_result_t *res, const uint16_t *len, uint32_t n, const mi_cls_enq_tab_t *t,
	       const mi_cls_run_tab_t *rt, uint32_t burst, uint32_t *seq, mi_cls_run_t *runs,
	       mi_cls_run_out_t *o, uint32_t *rest)
{
	uint32_t nd = 0, nr = 0, nrest = 0, prev = 0xFFFFFFFFu, left = burst;

	memset(o, 0, sizeof(*o));
	for (uint32_t i = 0; i < n; i++) {
		const mi_cls_result_t *r = &res[i];
		uint32_t id = t->ndst;

		if (burst && left-- == 0) {   /* a burst begins: the run before it is enqueued */
			left = burst - 1;
			prev = 0xFFFFFFFFu;
		}
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
				id = t->ent_dst[e];
				o->delivered++;
				if (!r->err) {
					o->packets++;
					o->octets += len[i];
				}
			} else {
				o->stale++;
			}
			break;
		}
		default:
			break;
		}
		if (id == t->ndst) {
			rest[nrest++] = i;
			continue;
		}
		const uint32_t key = id << 8 | r->cos;

		if (key != prev) {
			if (nr)
				close_run(&runs[nr - 1], nd, rt, o);
			runs[nr].first = nd;
			runs[nr].dst = (uint16_t)id;
			runs[nr].cos = r->cos;
			nr++;
			prev = key;
		}
		seq[nd++] = i;
	}
	if (nr)
		close_run(&runs[nr - 1], nd, rt, o);
	memcpy(seq + nd, rest, (size_t)nrest * sizeof(*rest));
	o->nruns = nr;
}
"""


def build_host_loop(tmp):
    src, so = os.path.join(tmp, "host_runs.c"), os.path.join(tmp, "host_runs.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP)
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           "-o", so, src])
    lib = C.CDLL(so)
    lib.host_runs.restype = None
    lib.host_runs.argtypes = [C.c_void_p] * 2 + [C.c_uint32] + [C.c_void_p] * 2 + [C.c_uint32] + [C.c_void_p] * 4
    return lib


def stats_us(ms):
    return {"us_median": round(1e3 * statistics.median(ms), 2), "us_min": round(1e3 * min(ms), 2),
            "us_max": round(1e3 * max(ms), 2)}


def run_config(torch, cfg, a, host):
    from odp_amd import cls
    from odp_amd import rules as R
    dev = torch.device("cuda:0")
    b, prog = R.CONFIGS[cfg](a.n)
    c = cls.Classifier(gpu=0)
    try:
        c.apply(prog)
        c.spec_wait()
        tab, queues, _ = c.enq_table()
        rtab = cls.run_tab(np.full(256, cls.RUN_VEC, np.uint8), np.full(256, a.vmax, np.uint16),
                           (np.arange(256) & 3).astype(np.uint8))
        n = b.n
        t_buf = torch.from_numpy(np.ascontiguousarray(b.buf)).to(dev)
        t_off = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        t_res = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_seq = torch.empty(n, dtype=torch.int32, device=dev)
        t_runs = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_out = torch.empty(cls.RUN_OUT_WORDS, dtype=torch.int64, device=dev)
        cur = torch.cuda.current_stream(dev)
        stream = cur.cuda_stream
        lens = np.ascontiguousarray(b.len, dtype=np.uint16)
        res = {"packets": n, "destinations": int(tab.ndst), "vmax": a.vmax}
        for burst in a.bursts:
            evs = []
            for _ in range(a.warmup + a.steps):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record(cur)
                rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_res.data_ptr(),
                                       stream)
                e[1].record(cur)
                k = c.last_launch()
                rc = rc or c.L.odp_amd_cls_enq_runs(c.pktio, t_res.data_ptr(), t_len.data_ptr(), n, C.byref(tab),
                                                    C.byref(rtab), burst, t_seq.data_ptr(), t_runs.data_ptr(), n,
                                                    t_out.data_ptr(), stream)
                e[2].record(cur)
                if rc:
                    raise RuntimeError(f"launch failed: {rc}")
                evs.append(e)
            torch.cuda.synchronize(dev)
            cls_ms = [e[0].elapsed_time(e[1]) for e in evs[a.warmup:]]
            run_ms = [e[1].elapsed_time(e[2]) for e in evs[a.warmup:]]
            info = (C.c_uint32 * 7)()
            c.L.odp_amd_cls_last_launch(c.pktio, info, 7)
            rec = t_res.cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE)
            seq = t_seq.cpu().numpy().view(np.uint32)
            out = t_out.cpu().numpy().view(np.uint64)
            nruns = int(out[6])
            runs = t_runs.cpu().numpy().view(np.uint32)[:nruns]
            # the host loop over the same records
            h_seq, h_rest = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            h_runs, h_out = np.zeros((n, 4), np.uint32), np.zeros(cls.RUN_OUT_WORDS, np.uint64)
            ts = []
            for _ in range(a.host_runs):
                t0 = time.perf_counter()
                host.host_runs(rec.ctypes.data, lens.ctypes.data, n, C.addressof(tab), C.addressof(rtab), burst,
                               h_seq.ctypes.data, h_runs.ctypes.data, h_out.ctypes.data, h_rest.ctypes.data)
                ts.append(1e3 * (time.perf_counter() - t0))
            same = bool(np.array_equal(seq, h_seq) and np.array_equal(out, h_out) and
                        np.array_equal(runs, h_runs[:nruns]))
            rp, cl, hl = stats_us(run_ms), stats_us(cls_ms), stats_us(ts)
            res[f"burst{burst}"] = {
                "out": cls.run_out_dict(out),
                "classify": dict(cl, kernel=k["name"], grid=k["grid"]),
                "run_plan": dict(rp, launches=int(info[1]), grid=int(info[6]),
                                 ns_per_packet_median=round(1e3 * rp["us_median"] / n, 3)),
                "host_loop": dict(hl, ns_per_packet_median=round(1e3 * hl["us_median"] / n, 3), runs=a.host_runs),
                "run_plan_over_classify_median": round(rp["us_median"] / cl["us_median"], 3),
                "host_loop_over_run_plan_median": round(hl["us_median"] / rp["us_median"], 1),
                "run_plan_below_host_loop": bool(rp["us_median"] < hl["us_median"]),
                "gpu_equals_host_loop": same}
        return res
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=9)
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--bursts", type=int, nargs="+", default=[0, 4096])
    ap.add_argument("--vmax", type=int, default=32)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch

    from odp_amd import _build
    _build.build()
    if not torch.cuda.is_available():
        raise SystemExit("enq_runs_bench: no GPU")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(prefix="enq_runs_bench_") as tmp:
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
