#!/usr/bin/env python3
"""The vector fill (mi_cls_vec_fill) at the end of its chain, beside the host
loop it replaces, on config 3's and config 5's records.

Per config and burst size, in one process: each step launches the
classification, the pool plan, the pool move, the run plan and the vector fill
on the same stream, with a HIP event before, between and after; the spans are
reported as median, min and max over the steps (after warm-up steps).  The fill
reads the plan's run count on the device and the move's ent[]: nothing is read
back between the stages.  Every CoS with queues takes packets of one pool of
1536-byte packets, of which the whole need is at hand, and delivers packet
vectors of up to --vmax packets from one of four vector pools (slot = CoS index
& 3); packets and vectors lie in device memory and each vector pool supplies
exactly what the plan needs.

The host loop is a plain C walk of the same plan (per run: its packets gathered
through seq and ent, vectors taken one by one, tables and sizes written, the
event array and the per-run entry), compiled -O2, single thread, median of
--host-runs runs; its ev, evr, lost, out and vectors are compared with the GPU's.

  python tools/vec_fill_bench.py [--n 1000000] [--steps 60] [--warmup 10] [--out FILE]
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

SIZE_OFF, TBL_OFF, E2H = 16, 24, 64
HEADROOM, DFM, CAP = 128, 192, 1536
INPUT = 0x0DD0_0000_0000_0042

HOST_LOOP = r"""
#include <stdint.h>
#include <string.h>
#include "mi_cls.h"

/* vec: the vectors' memory as the host sees it; vgot holds device addresses,
 * dev0 is the device address of vec[0] */
void host_fill(const uint32_t *seq, const mi_cls_run_t *runs, uint32_t nruns, const uint64_t *ent,
	       const uint64_t *vgot, const mi_cls_run_tab_t *rt, const uint32_t *vbase, const uint32_t *vhave,
	       uint64_t e2h, uint32_t size_off, uint32_t tbl_off, uint8_t *vec, uint64_t dev0, uint64_t *ev,
	       mi_cls_evrun_t *evr, uint64_t *lost, mi_cls_vec_out_t *o)
{
	uint32_t evn = 0, next[MI_CLS_RUN_VSLOTS] = { 0 };
	uint64_t need[MI_CLS_RUN_VSLOTS] = { 0 };

	memset(o, 0, sizeof(*o));
	for (uint32_t r = 0; r < nruns; r++) {
		const mi_cls_run_t *u = &runs[r];
		const uint32_t *s = seq + u->first;

		evr[r].ev_first = evn;
		evr[r].vfirst = 0xFFFFFFFFu;
		if (!(u->flags & MI_CLS_RUN_VEC)) {
			for (uint32_t i = 0; i < u->count; i++) {
				const uint64_t e = ent[s[i]];

				o->holes += e == 0;
				ev[evn++] = e ? e - e2h : 0;
			}
			evr[r].ev_count = evr[r].pk_enq = u->count;
			o->events += u->count;
			continue;
		}
		const uint32_t slot = rt->vslot[u->cos], vm = rt->vmax[u->cos];
		uint32_t done = 0, g = 0;

		need[slot] += u->nvec;
		for (uint32_t k = 0; k < u->nvec; k++) {
			if (next[slot] >= vhave[slot]) {
				ev[evn++] = 0;
				continue;
			}
			const uint32_t vi = vbase[slot] + next[slot]++;
			const uint32_t sz = u->count - done < vm ? u->count - done : vm;
			uint8_t *v = vec + (vgot[vi] - dev0);
			uint64_t *tbl = (uint64_t *)(v + tbl_off);

			if (g++ == 0)
				evr[r].vfirst = vi;
			for (uint32_t j = 0; j < sz; j++) {
				const uint64_t e = ent[s[done + j]];

				o->holes += e == 0;
				tbl[j] = e ? e - e2h : 0;
			}
			*(uint32_t *)(v + size_off) = sz;
			ev[evn++] = vgot[vi];
			done += sz;
			o->vectors++;
			o->in_vectors += sz;
		}
		for (uint32_t i = done; i < u->count; i++) {
			const uint64_t e = ent[s[i]];

			o->holes += e == 0;
			lost[o->lost++] = e ? e - e2h : 0;
		}
		evr[r].ev_count = g;
		evr[r].pk_enq = done;
		o->events += g;
	}
	o->ev_span = evn;
	for (uint32_t k = 0; k < MI_CLS_RUN_VSLOTS; k++)
		o->vec_used[k] = need[k] < vhave[k] ? need[k] : vhave[k];
}
"""


def build_host_loop(tmp):
    src, so = os.path.join(tmp, "host_fill.c"), os.path.join(tmp, "host_fill.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP)
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           "-o", so, src])
    lib = C.CDLL(so)
    lib.host_fill.restype = None
    lib.host_fill.argtypes = ([C.c_void_p] * 2 + [C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint64] + [C.c_uint32] * 2 +
                              [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4)
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
        vslot = (np.arange(256) & 3).astype(np.uint8)
        rtab = cls.run_tab(np.full(256, cls.RUN_VEC, np.uint8), np.full(256, a.vmax, np.uint16), vslot)
        n = b.n
        t_buf = torch.from_numpy(np.ascontiguousarray(b.buf)).to(dev)
        t_off = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        t_res = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_seq = torch.empty(n, dtype=torch.int32, device=dev)
        t_runs = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_rout = torch.empty(cls.RUN_OUT_WORDS, dtype=torch.int64, device=dev)
        # one packet pool for every CoS with queues
        with_q = np.nonzero(np.ctypeslib.as_array(tab.cos_nq))[0]
        cos_slot = np.full(256, 0xFF, np.uint8)
        cos_slot[with_q] = 0
        ptab = cls.pool_tab(cos_slot, [CAP])
        dstq = np.array(queues, np.uint64)
        u = C.c_uint32 * cls.POOL_SLOTS
        t_ro = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_dec = torch.empty(n, dtype=torch.int32, device=dev)
        t_idx = torch.empty(n, dtype=torch.int32, device=dev)
        t_pout = torch.empty(cls.POOL_OUT_WORDS, dtype=torch.int32, device=dev)
        t_ent = torch.empty(n, dtype=torch.int64, device=dev)
        t_mout = torch.empty(4, dtype=torch.int64, device=dev)
        t_ev = torch.empty(n, dtype=torch.int64, device=dev)
        t_evr = torch.empty((n, 4), dtype=torch.int32, device=dev)
        t_lost = torch.empty(n, dtype=torch.int64, device=dev)
        t_out = torch.empty(cls.VEC_OUT_WORDS, dtype=torch.int64, device=dev)
        cur = torch.cuda.current_stream(dev)
        stream = cur.cuda_stream
        res = {"packets": n, "destinations": int(tab.ndst), "vmax": a.vmax}
        stride = TBL_OFF + 8 * a.vmax

        def pools(have):
            return c.L.odp_amd_cls_pool_plan(c.pktio, t_res.data_ptr(), t_len.data_ptr(), None, n, C.byref(ptab),
                                             u(have), u(0), t_ro.data_ptr(), t_dec.data_ptr(), t_idx.data_ptr(),
                                             t_pout.data_ptr(), stream)

        def plan_runs(burst):
            return c.L.odp_amd_cls_enq_runs(c.pktio, t_ro.data_ptr(), t_len.data_ptr(), n, C.byref(tab),
                                            C.byref(rtab), burst, t_seq.data_ptr(), t_runs.data_ptr(), n,
                                            t_rout.data_ptr(), stream)

        # the packets: the need first, then all of it at hand, in one device tensor
        rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_res.data_ptr(), stream)
        rc = rc or pools(cls.POOL_UNLIMITED)
        if rc:
            raise RuntimeError(f"launch failed: {rc}")
        torch.cuda.synchronize(dev)
        have = int(cls.pool_out_dict(t_pout.cpu().numpy().view(np.uint32))["need"][0])
        t_pkt = torch.zeros(have * (DFM + CAP) + 64, dtype=torch.uint8, device=dev)
        lo = (t_pkt.data_ptr() + 63) & ~63
        got = (lo + (DFM + CAP) * np.arange(max(have, 1), dtype=np.uint64)).astype(np.uint64)
        t_got = torch.from_numpy(got.view(np.int64)).to(dev)
        ma = cls.move_args(tab, dstq, pkts=t_buf.data_ptr(), pkts_bytes=t_buf.numel(), off=t_off.data_ptr(),
                           len=t_len.data_ptr(), res=t_ro.data_ptr(), dec=t_dec.data_ptr(), idx=t_idx.data_ptr(),
                           got=t_got.data_ptr(), ngot=have, n=n, input=INPUT, headroom=HEADROOM,
                           data_from_meta=DFM, arena_lo=lo, arena_bytes=have * (DFM + CAP), ent=t_ent.data_ptr(),
                           out=t_mout.data_ptr())
        for burst in a.bursts:
            # the chain once, for the vectors each pool must supply
            rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_res.data_ptr(), stream)
            rc = rc or pools(have) or c.pool_move(ma, stream) or plan_runs(burst)
            if rc:
                raise RuntimeError(f"launch failed: {rc}")
            torch.cuda.synchronize(dev)
            rout = cls.run_out_dict(t_rout.cpu().numpy().view(np.uint64))
            vhave = np.array(rout["vec_need"], np.int64)
            vbase = np.cumsum(vhave) - vhave
            nv = int(vhave.sum())
            t_vec = torch.zeros(max(nv, 1) * stride, dtype=torch.uint8, device=dev)
            vgot = (t_vec.data_ptr() + stride * np.arange(nv)).astype(np.uint64)
            t_vgot = torch.from_numpy(vgot.view(np.int64) if nv else np.zeros(1, np.int64)).to(dev)
            va = cls.vec_args(rtab, vbase=vbase, vhave=vhave, vcap=[a.vmax] * 4, seq=t_seq.data_ptr(),
                              runs=t_runs.data_ptr(), run_out=t_rout.data_ptr(), ent=t_ent.data_ptr(),
                              vgot=t_vgot.data_ptr(), n=n, run_cap=n, nvgot=nv, size_off=SIZE_OFF, tbl_off=TBL_OFF,
                              ent_to_handle=E2H, varena_lo=t_vec.data_ptr(), varena_bytes=t_vec.numel(),
                              ev=t_ev.data_ptr(), evr=t_evr.data_ptr(), lost=t_lost.data_ptr(), out=t_out.data_ptr())
            evs = []
            for _ in range(a.warmup + a.steps):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                e[0].record(cur)
                rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_res.data_ptr(),
                                       stream)
                e[1].record(cur)
                rc = rc or pools(have)
                e[2].record(cur)
                rc = rc or c.pool_move(ma, stream)
                e[3].record(cur)
                rc = rc or plan_runs(burst)
                e[4].record(cur)
                rc = rc or c.vec_fill(va, stream)
                e[5].record(cur)
                if rc:
                    raise RuntimeError(f"launch failed: {rc}")
                evs.append(e)
            torch.cuda.synchronize(dev)
            span = [[e[k].elapsed_time(e[k + 1]) for e in evs[a.warmup:]] for k in range(5)]
            info = (C.c_uint32 * 7)()
            c.L.odp_amd_cls_last_launch(c.pktio, info, 7)
            out = t_out.cpu().numpy().view(np.uint64)
            od = cls.vec_out_dict(out)
            nruns = rout["nruns"]
            seq = t_seq.cpu().numpy().view(np.uint32)
            runs = np.ascontiguousarray(t_runs.cpu().numpy().view(np.uint32)[:nruns])
            ev = t_ev.cpu().numpy().view(np.uint64)[: od["ev_span"]]
            evr = t_evr.cpu().numpy().view(np.uint32)[:nruns]
            lost = np.sort(t_lost.cpu().numpy().view(np.uint64)[: od["lost"]])
            vec = t_vec.cpu().numpy()
            ent = t_ent.cpu().numpy().view(np.uint64)
            # the host loop over the same plan
            h_ev, h_lost = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            h_evr, h_out = np.zeros((n, 4), np.uint32), np.zeros(cls.VEC_OUT_WORDS, np.uint64)
            h_vec = np.zeros_like(vec)
            u32 = C.c_uint32 * 16
            hb, hh = u32(*[int(x) for x in vbase]), u32(*[int(x) for x in vhave])
            ts = []
            for _ in range(a.host_runs):
                t0 = time.perf_counter()
                host.host_fill(seq.ctypes.data, runs.ctypes.data, nruns, ent.ctypes.data, vgot.ctypes.data,
                               C.addressof(rtab), hb, hh, E2H, SIZE_OFF, TBL_OFF, h_vec.ctypes.data,
                               t_vec.data_ptr(), h_ev.ctypes.data, h_evr.ctypes.data, h_lost.ctypes.data,
                               h_out.ctypes.data)
                ts.append(1e3 * (time.perf_counter() - t0))
            same = bool(np.array_equal(out, h_out) and np.array_equal(ev, h_ev[: od["ev_span"]]) and
                        np.array_equal(evr, h_evr[:nruns]) and np.array_equal(vec, h_vec) and
                        np.array_equal(lost, np.sort(h_lost[: od["lost"]])))
            cl, pl, mv, rp, vf, hl = (stats_us(x) for x in (*span, ts))
            # what the fill moves: seq, ent and the handle stores per delivered packet, runs in (twice:
            # count and place, once more gathered by the fill), evr and the per-run scratch out and in
            moved = rout["delivered"] * (4 + 8 + 8) + nruns * (16 * 3 + 16 + 16 + 16) + od["vectors"] * 12
            res[f"burst{burst}"] = {
                "run_out": rout, "out": od,
                "move_out": cls.move_out_dict(t_mout.cpu().numpy().view(np.uint64)),
                "classify": cl, "pool_plan": pl, "pool_move": mv, "run_plan": rp,
                "vec_fill": dict(vf, launches=int(info[1]), grid=int(info[6]),
                                 ns_per_packet_median=round(1e3 * vf["us_median"] / n, 3),
                                 bytes_moved=int(moved), us_at_8TBps=round(moved / 8e6, 2)),
                "host_loop": dict(hl, ns_per_packet_median=round(1e3 * hl["us_median"] / n, 3), runs=a.host_runs),
                "host_loop_over_vec_fill_median": round(hl["us_median"] / vf["us_median"], 1),
                "vec_fill_below_host_loop": bool(vf["us_median"] < hl["us_median"]),
                "gpu_equals_host_loop": same}
            del t_vec
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
        raise SystemExit("vec_fill_bench: no GPU")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(prefix="vec_fill_bench_") as tmp:
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
