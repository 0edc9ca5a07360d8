#!/usr/bin/env python3
"""The pool plan (mi_cls_pool_plan) beside the classification it follows, the
enqueue plan on the same records and the host loop it replaces, on config 3's
and config 5's records with 1, 4 and 16 pool slots spread over the CoS.

Per config and slot count, in one process: each step launches the
classification, then the pool plan of its records (res_out disjoint, so every
step and the enqueue plan see the same records), then the enqueue plan, on one
stream with a HIP event before, between and after; the spans are reported as
median, min and max over the steps after the warm-up steps.  Each plan's
launches are timed together: they are stream-ordered launches with no host work
in between.

A slot holds 1536-byte packets, the last of several 128-byte ones (so some
frames are too long); every slot has three quarters of its need at hand (so
some frames find their pool short).

The host loop is a plain C per-record ranking of the same records, compiled
-O2, single thread, median of --host-runs runs; its output is compared with the
GPU's, word for word.

  python tools/pool_plan_bench.py [--n 1000000] [--steps 60] [--warmup 10] [--out FILE]
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

void host_pools(const mi_cls_result_t *res, const uint16_t *len, const uint8_t *own, uint32_t n,
		const mi_cls_pool_tab_t *t, const uint32_t *have, const uint32_t *base, mi_cls_result_t *res_out,
		uint32_t *dec, uint32_t *idx, mi_cls_pool_out_t *o)
{
	memset(o, 0, sizeof(*o));
	for (uint32_t i = 0; i < n; i++) {
		const mi_cls_result_t r = res[i];
		const uint32_t slot = t->cos_slot[r.cos];
		uint32_t fate = MI_CLS_PF_NONE, at = 0xFFFFFFFFu;

		res_out[i] = r;
		if (r.outcome == MI_CLS_OUT_ENQ && slot < t->nslot) {
			if (own && own[i] == slot + 1u) {
				fate = MI_CLS_PF_INPLACE;
				o->inplace++;
			} else if (len[i] > t->slot_cap[slot]) {
				fate = MI_CLS_PF_TOO_LONG;
				o->too_long++;
			} else {
				const uint32_t rank = o->need[slot]++;

				if (rank < have[slot]) {
					fate = MI_CLS_PF_FRESH;
					at = base[slot] + rank;
					o->fresh++;
				} else {
					fate = MI_CLS_PF_SHORT;
					o->shorted++;
				}
			}
			if (fate == MI_CLS_PF_TOO_LONG || fate == MI_CLS_PF_SHORT)
				res_out[i].outcome = MI_CLS_OUT_DISCARD;
			fate |= slot << 4;
		}
		dec[i] = fate;
		idx[i] = at;
	}
	for (uint32_t k = 0; k < MI_CLS_POOL_SLOTS; k++)
		o->used[k] = o->need[k] < have[k] ? o->need[k] : have[k];
}
"""


def build_host_loop(tmp):
    src, so = os.path.join(tmp, "host_pools.c"), os.path.join(tmp, "host_pools.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP)
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           "-o", so, src])
    lib = C.CDLL(so)
    lib.host_pools.restype = None
    lib.host_pools.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 7
    return lib


def stats_us(ms):
    return {"us_median": round(1e3 * statistics.median(ms), 2), "us_min": round(1e3 * min(ms), 2),
            "us_max": round(1e3 * max(ms), 2)}


def run_config(torch, cfg, nslot, a, host):
    from odp_amd import cls
    from odp_amd import rules as R
    dev = torch.device("cuda:0")
    b, prog = R.CONFIGS[cfg](a.n)
    c = cls.Classifier(gpu=0)
    try:
        c.apply(prog)
        c.spec_wait()
        tab, _, _ = c.enq_table()
        # the CoS with queues, spread over the slots in turn
        with_q = np.nonzero(np.ctypeslib.as_array(tab.cos_nq))[0]
        cos_slot = np.full(256, 0xFF, np.uint8)
        cos_slot[with_q] = np.arange(with_q.shape[0]) % nslot
        caps = [1536] * nslot
        if nslot > 1:
            caps[-1] = 128
        ptab = cls.pool_tab(cos_slot, caps)
        n, ng = b.n, tab.ndst + 2
        u = C.c_uint32 * cls.POOL_SLOTS
        t_buf = torch.from_numpy(np.ascontiguousarray(b.buf)).to(dev)
        t_off = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        t_res = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_ro = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_dec = torch.empty(n, dtype=torch.int32, device=dev)
        t_idx = torch.empty(n, dtype=torch.int32, device=dev)
        t_pout = torch.empty(cls.POOL_OUT_WORDS, dtype=torch.int32, device=dev)
        t_perm = torch.empty(n, dtype=torch.int32, device=dev)
        t_gbeg = torch.empty(ng, dtype=torch.int32, device=dev)
        t_eout = torch.empty(len(cls.ENQ_OUT_FIELDS), dtype=torch.int64, device=dev)
        cur = torch.cuda.current_stream(dev)
        stream = cur.cuda_stream

        def pools(have, base):
            return c.L.odp_amd_cls_pool_plan(c.pktio, t_res.data_ptr(), t_len.data_ptr(), None, n, C.byref(ptab),
                                             u(*have), u(*base), t_ro.data_ptr(), t_dec.data_ptr(),
                                             t_idx.data_ptr(), t_pout.data_ptr(), stream)

        # the need first, then three quarters of it at hand
        rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_res.data_ptr(), stream)
        rc = rc or pools([cls.POOL_UNLIMITED] * cls.POOL_SLOTS, [0] * cls.POOL_SLOTS)
        if rc:
            raise RuntimeError(f"launch failed: {rc}")
        torch.cuda.synchronize(dev)
        need = np.array(cls.pool_out_dict(t_pout.cpu().numpy().view(np.uint32))["need"])
        have = (need * 3 // 4).tolist()
        base = (np.cumsum(have) - have).tolist()
        evs = []
        for _ in range(a.warmup + a.steps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(cur)
            rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_res.data_ptr(),
                                   stream)
            e[1].record(cur)
            k = c.last_launch()
            rc = rc or pools(have, base)
            e[2].record(cur)
            rc = rc or c.L.odp_amd_cls_enq_plan(c.pktio, t_res.data_ptr(), t_len.data_ptr(), n, C.byref(tab),
                                                t_perm.data_ptr(), t_gbeg.data_ptr(), t_eout.data_ptr(), stream)
            e[3].record(cur)
            if rc:
                raise RuntimeError(f"launch failed: {rc}")
            evs.append(e)
        torch.cuda.synchronize(dev)
        spans = [[e[j].elapsed_time(e[j + 1]) for e in evs[a.warmup:]] for j in range(3)]
        rec = t_res.cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE)
        g = [t.cpu().numpy().view(np.uint32).reshape(-1) for t in (t_ro, t_dec, t_idx, t_pout)]
        # the host loop over the same records
        lens = np.ascontiguousarray(b.len, dtype=np.uint16)
        h_ro, h_dec, h_idx = np.zeros(n, R.RESULT_DTYPE), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        h_out = np.zeros(cls.POOL_OUT_WORDS, np.uint32)
        ts = []
        for _ in range(a.host_runs):
            t0 = time.perf_counter()
            host.host_pools(rec.ctypes.data, lens.ctypes.data, None, n, C.addressof(ptab), u(*have), u(*base),
                            h_ro.ctypes.data, h_dec.ctypes.data, h_idx.ctypes.data, h_out.ctypes.data)
            ts.append(1e3 * (time.perf_counter() - t0))
        same = bool(np.array_equal(g[0], h_ro.view(np.uint32).reshape(-1)) and np.array_equal(g[1], h_dec) and
                    np.array_equal(g[2], h_idx) and np.array_equal(g[3], h_out))
        cl, pl, en, hl = stats_us(spans[0]), stats_us(spans[1]), stats_us(spans[2]), stats_us(ts)
        out = cls.pool_out_dict(g[3])
        return {"packets": n, "slots": nslot, "out": {f: out[f] for f in cls.POOL_OUT_FIELDS},
                "need": out["need"][:nslot], "used": out["used"][:nslot],
                "classify": dict(cl, kernel=k["name"], grid=k["grid"]),
                "pool_plan": dict(pl, ns_per_packet_median=round(1e3 * pl["us_median"] / n, 3)),
                "enq_plan": en,
                "host_loop": dict(hl, ns_per_packet_median=round(1e3 * hl["us_median"] / n, 3), runs=a.host_runs),
                "pool_plan_over_enq_plan_median": round(pl["us_median"] / en["us_median"], 3),
                "pool_plan_over_classify_median": round(pl["us_median"] / cl["us_median"], 3),
                "host_loop_over_pool_plan_median": round(hl["us_median"] / pl["us_median"], 1),
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
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch

    from odp_amd import _build
    _build.build()
    if not torch.cuda.is_available():
        raise SystemExit("pool_plan_bench: no GPU")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(prefix="pool_plan_bench_") as tmp:
        host = build_host_loop(tmp)
        for cfg in a.configs:
            for ns in a.slots:
                res[f"config{cfg}_slots{ns}"] = run_config(torch, cfg, ns, a, host)
    s = json.dumps(res)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
