#!/usr/bin/env python3
"""The pool move (mi_cls_pool_move) in the chain it completes -- classify, pool
plan, pool move, enqueue plan on one stream -- and beside the host loop it
replaces, on config 3's and config 5's records (IMIX frames) with 1, 4 and 16
pool slots spread over the CoS, frames and packets in device memory.

Per config and slot count, in one process: each step launches the four stages
on one stream with a HIP event before, between and after; the spans are
reported as median, min and max over the steps after the warm-up steps.  The
slots are the pool-plan bench's: 1536-byte packets, the last of several slots
128-byte ones (so some frames are too long); every slot has three quarters of
its need at hand (so some frames find their pool short).

The move's rate is its frame bytes read plus written over its span, beside the
6.29 TB/s a plain device copy reaches on this GPU; all_bytes adds the lines and
the per-record words it reads and writes.

The host loop is plain C, one thread, -O2: per FRESH record a memcpy of the
frame in its 16-byte pieces and the metadata line, into a host copy of the
packets; median of --host-runs runs.  Its packets are compared with the GPU's
byte for byte.

  python tools/pool_move_bench.py [--n 1000000] [--steps 60] [--warmup 10] [--out FILE]
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

COPY_TBS = 6.29                  # a device copy on this GPU, read + written
HEADROOM, DFM, INPUT = 128, 192, 0x0DD00042

HOST_LOOP = r"""
#include <stdint.h>
#include <string.h>
#include "mi_cls.h"

/* mem: the host copy of the packets, whose byte 0 has the device address lo */
void host_move(const uint8_t *pkts, uint64_t bytes, const uint32_t *off, const uint16_t *len,
	       const mi_cls_result_t *res, const uint32_t *dec, const uint32_t *idx, uint32_t n, const uint64_t *got,
	       const mi_cls_enq_tab_t *t, const uint64_t *dstq, uint64_t input, uint32_t headroom, uint32_t dfm,
	       uint8_t *mem, uint64_t lo, uint64_t *ent, mi_cls_move_out_t *o)
{
	memset(o, 0, sizeof(*o));
	for (uint32_t i = 0; i < n; i++) {
		ent[i] = 0;
		if ((dec[i] & 15u) != MI_CLS_PF_FRESH)
			continue;
		const mi_cls_result_t r = res[i];
		const uint64_t line = got[idx[i]];
		mi_cls_pkt_meta_t m;
		const uint32_t pad = ((uint32_t)len[i] + 15u) & ~15u;
		const uint64_t room = bytes - off[i];
		const uint32_t e = (uint32_t)t->cos_q0[r.cos] + r.queue;

		memset(&m, 0, sizeof(m));
		m.data_off = headroom;
		m.len = len[i];
		m.in_flags = r.in_flags;
		m.err = r.err;
		m.cos = r.cos;
		m.cls_mark = r.mark;
		m.l3 = r.l3_offset;
		m.l4 = r.l4_offset;
		if (r.outcome == MI_CLS_OUT_ENQ && r.queue < t->cos_nq[r.cos] && e < MI_CLS_ENQ_ENT &&
		    t->ent_dst[e] < t->ndst)
			m.dst_queue = dstq[t->ent_dst[e]];
		m.input = input;
		memcpy(mem + (line - lo), &m, sizeof(m));
		/* the frame in its 16-byte pieces; behind the buffer's end, zeros */
		if (room >= pad) {
			memcpy(mem + (line - lo) + dfm, pkts + off[i], pad);
		} else {
			memcpy(mem + (line - lo) + dfm, pkts + off[i], room);
			memset(mem + (line - lo) + dfm + room, 0, pad - room);
		}
		ent[i] = line;
		o->moved++;
		o->bytes += len[i];
	}
}
"""


def build_host_loop(tmp):
    src, so = os.path.join(tmp, "host_move.c"), os.path.join(tmp, "host_move.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP)
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           "-o", so, src])
    lib = C.CDLL(so)
    lib.host_move.restype = None
    vp = C.c_void_p
    lib.host_move.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, C.c_uint32,
                              C.c_uint32, vp, C.c_uint64, vp, vp]
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
        tab, queues, _ = c.enq_table()
        dstq = np.array(queues, np.uint64)
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
        t_ent = torch.empty(n, dtype=torch.int64, device=dev)
        t_mout = torch.empty(4, dtype=torch.int64, device=dev)
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
        # the packets taken: slot k's at base[k], a line, the headroom, the slot's capacity
        stride = [DFM + caps[k] for k in range(nslot)]
        starts = np.cumsum([0] + [have[k] * stride[k] for k in range(nslot)])
        nbytes = int(starts[-1])
        t_pkt = torch.zeros(nbytes + 64, dtype=torch.uint8, device=dev)
        lo = (t_pkt.data_ptr() + 63) & ~63
        got = np.zeros(max(1, sum(have[:nslot])), np.uint64)
        for k in range(nslot):
            got[base[k]: base[k] + have[k]] = lo + int(starts[k]) + stride[k] * np.arange(have[k], dtype=np.uint64)
        t_got = torch.from_numpy(got.view(np.int64)).to(dev)
        ma = cls.move_args(tab, dstq, pkts=t_buf.data_ptr(), pkts_bytes=t_buf.numel(), off=t_off.data_ptr(),
                           len=t_len.data_ptr(), res=t_ro.data_ptr(), dec=t_dec.data_ptr(), idx=t_idx.data_ptr(),
                           got=t_got.data_ptr(), ngot=len(got), n=n, input=INPUT, headroom=HEADROOM,
                           data_from_meta=DFM, arena_lo=lo, arena_bytes=nbytes, ent=t_ent.data_ptr(),
                           out=t_mout.data_ptr())
        evs = []
        for _ in range(a.warmup + a.steps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            e[0].record(cur)
            rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_res.data_ptr(),
                                   stream)
            e[1].record(cur)
            k = c.last_launch()
            rc = rc or pools(have, base)
            e[2].record(cur)
            rc = rc or c.pool_move(ma, stream)
            e[3].record(cur)
            rc = rc or c.L.odp_amd_cls_enq_plan(c.pktio, t_ro.data_ptr(), t_len.data_ptr(), n, C.byref(tab),
                                                t_perm.data_ptr(), t_gbeg.data_ptr(), t_eout.data_ptr(), stream)
            e[4].record(cur)
            if rc:
                raise RuntimeError(f"launch failed: {rc}")
            evs.append(e)
        torch.cuda.synchronize(dev)
        spans = [[e[j].elapsed_time(e[j + 1]) for e in evs[a.warmup:]] for j in range(4)]
        mout = cls.move_out_dict(t_mout.cpu().numpy().view(np.uint64))
        # the host loop over the same plan, into a host copy of the packets
        ro = t_ro.cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE)
        dec, idx = t_dec.cpu().numpy().view(np.uint32), t_idx.cpu().numpy().view(np.uint32)
        buf = np.ascontiguousarray(b.buf)
        off = np.ascontiguousarray(b.off, dtype=np.uint32)
        lens = np.ascontiguousarray(b.len, dtype=np.uint16)
        h_ent, h_out = np.zeros(n, np.uint64), np.zeros(4, np.uint64)
        ts = []
        for _ in range(a.host_runs):
            mem = np.zeros(nbytes, np.uint8)
            t0 = time.perf_counter()
            host.host_move(buf.ctypes.data, buf.nbytes, off.ctypes.data, lens.ctypes.data, ro.ctypes.data,
                           dec.ctypes.data, idx.ctypes.data, n, got.ctypes.data, C.addressof(tab), dstq.ctypes.data,
                           INPUT, HEADROOM, DFM, mem.ctypes.data, lo, h_ent.ctypes.data, h_out.ctypes.data)
            ts.append(1e3 * (time.perf_counter() - t0))
        at = lo - t_pkt.data_ptr()
        same = bool(np.array_equal(t_pkt[at: at + nbytes].cpu().numpy(), mem) and
                    np.array_equal(t_ent.cpu().numpy().view(np.uint64), h_ent) and
                    cls.move_out_dict(h_out) == mout)
        cl, pl, mv, en, hl = (stats_us(s) for s in (*spans, ts))
        frame_bytes = 2 * mout["bytes"]
        all_bytes = frame_bytes + 64 * (mout["moved"] + mout["inplace"]) + n * (4 + 2 + 16 + 4 + 4 + 8) + \
            8 * mout["moved"]
        tbs = frame_bytes / (mv["us_median"] * 1e-6) / 1e12
        return {"packets": n, "slots": nslot, "out": mout, "mean_frame": round(float(np.mean(b.len)), 1),
                "classify": dict(cl, kernel=k["name"], grid=k["grid"]), "pool_plan": pl,
                "pool_move": dict(mv, ns_per_packet_median=round(1e3 * mv["us_median"] / n, 3),
                                  frame_bytes=frame_bytes, all_bytes=all_bytes, frame_tb_per_s=round(tbs, 3),
                                  all_tb_per_s=round(all_bytes / (mv["us_median"] * 1e-6) / 1e12, 3),
                                  share_of_copy_rate=round(tbs / COPY_TBS, 3)),
                "enq_plan": en,
                "host_loop": dict(hl, ns_per_packet_median=round(1e3 * hl["us_median"] / n, 3), runs=a.host_runs),
                "host_loop_over_pool_move_median": round(hl["us_median"] / mv["us_median"], 1),
                "gpu_equals_host_loop": same}
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch

    from odp_amd import cls
    if "ODP_AMD_LIB_DIR" not in os.environ:      # a variant build's libraries are measured as they are
        from odp_amd import _build
        _build.build()
    if not torch.cuda.is_available():
        raise SystemExit("pool_move_bench: no GPU")
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "libraries": os.path.relpath(os.path.dirname(cls.LIB_MI), ROOT), "copy_rate_tb_per_s": COPY_TBS}
    with tempfile.TemporaryDirectory(prefix="pool_move_bench_") as tmp:
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
