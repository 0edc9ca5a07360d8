#!/usr/bin/env python3
"""The parse-only kernel vs the classification kernel under a default-CoS-only
program, timed interleaved in one process on config 3's batch, rotating over
4 device copies, on the same bytes:

  plain      mi_cls_parse (ETH, ALL, no checksums)
             vs mi_cls_classify without pktin options
  checksums  mi_cls_parse (ETH, ALL, checksums 0xF)
             vs the pktin-option (CK) classification kernel, options 0x3C,
             on the batch with valid checksums written in
             (pktgen.set_checksums: every UDP / TCP sum runs over its frame)

The classification runs the generic kernels (MI_CLS_JIT=0: no
program-specialised kernel).  Per launch: time (median and min over the
rounds), algorithmic bytes (min(len, 128) window + 6 B descriptor + 16 B record
per packet; the checksum lines read whole frames) and their fraction of 8 TB/s.
Last, the wall time of one host call (mi_cls_parse_host, page-locked, 1 / 64 /
4096 packets): what an odp_packet_parse call costs.

  python tools/parse_bench.py [--n 1000000] [--rounds 7] [--steps 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["MI_CLS_JIT"] = "0"
HBM_PEAK = 8.0e12


def span_ms(torch, stream, steps, fn, args):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    for i in range(steps):
        rc = fn(*args[i % len(args)])
        if rc:
            raise RuntimeError(f"launch failed: {rc}")
    ev1.record(stream)
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps


def one_packet_call(p, b):
    """Wall time of mi_cls_parse_host for one packet in page-locked memory
    (launch + wait: what one odp_packet_parse call costs on the GPU side),
    and for 64 and 4096 packets in one call."""
    import time

    from odp_amd import rules as R
    from odp_amd.cls import PinnedArray
    out = {}
    for n in (1, 64, 4096):
        s = b.slice(0, n)
        keep = [PinnedArray(s.buf.nbytes), PinnedArray(4 * n), PinnedArray(2 * n), PinnedArray(16 * n)]
        buf, off, ln = keep[0].view(np.uint8), keep[1].view(np.uint32, n), keep[2].view(np.uint16, n)
        rec = keep[3].view(R.RESULT_DTYPE, n)
        buf[:], off[:], ln[:] = s.buf, s.off, s.len
        ts = []
        for i in range(220):
            t0 = time.perf_counter()
            p.parse_host(buf, off, ln, rec)
            ts.append(time.perf_counter() - t0)
        out[f"n{n}_us_median"] = round(1e6 * statistics.median(ts[20:]), 1)
        for k in keep:
            k.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch

    from odp_amd import _build
    from odp_amd import rules as R
    from odp_amd.cls import LAYER_ALL, PROTO_ETH, Classifier, ParseContext
    _build.build()
    if not torch.cuda.is_available():
        raise SystemExit("parse_bench: no GPU")
    from odp_amd import pktgen as pg
    b, _ = R.config3(a.n)
    bck = pg.set_checksums(pg.Batch(b.buf.copy(), b.off, b.len))
    dev = torch.device("cuda:0")
    c = Classifier(gpu=0)
    c.apply([R.cos("default", queue=1), ("default", 0)])
    p = ParseContext(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    keep, bufs = [], []
    for src in [b] * a.rotate + [bck] * a.rotate:
        tb = torch.from_numpy(src.buf).to(dev)
        to = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        tl = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        o_p = torch.empty((b.n, 4), dtype=torch.int32, device=dev)
        o_c = torch.empty((b.n, 4), dtype=torch.int32, device=dev)
        keep += [tb, to, tl, o_p, o_c]
        bufs.append((tb.data_ptr(), to.data_ptr(), tl.data_ptr(), o_p.data_ptr(), o_c.data_ptr()))
    cur = torch.cuda.current_stream(dev)
    frame = int(b.len.astype(np.int64).sum())
    res = {"packets": b.n, "frame_bytes": frame, "header_bytes": b.header_bytes(), "rotate": a.rotate,
           "steps": a.steps, "rounds": a.rounds}

    def line(ms, by):
        med, mn = statistics.median(ms), min(ms)
        return {"us_per_launch_median": round(1e3 * med, 2), "us_per_launch_min": round(1e3 * mn, 2),
                "rounds_us": [round(1e3 * x, 2) for x in ms], "bytes_per_launch": by,
                "frac_of_8TBps_median": round(by / (med * 1e-3) / HBM_PEAK, 4),
                "mpkts_per_s_median": round(b.n / (med * 1e-3) / 1e6, 1)}

    for key, sel, opt in (("plain", 0, 0), ("checksums", 0xF, 0x3C)):
        c.set_pktin_opt(opt)
        use = bufs[a.rotate:] if sel else bufs[:a.rotate]
        p_args = [(pk, po, pl, b.n, PROTO_ETH, LAYER_ALL, sel, op, stream) for pk, po, pl, op, _ in use]
        c_args = [(pk, po, pl, b.n, oc, stream) for pk, po, pl, _, oc in use]
        span_ms(torch, cur, 2 * a.rotate, p.parse_device, p_args)
        span_ms(torch, cur, 2 * a.rotate, c.classify_device, c_args)
        p_ms, c_ms = [], []
        for _ in range(a.rounds):
            p_ms.append(span_ms(torch, cur, a.steps, p.parse_device, p_args))
            c_ms.append(span_ms(torch, cur, a.steps, c.classify_device, c_args))
        ll = c.last_launch()
        pl = p.last_launch()
        k0 = 5 * a.rotate if sel else 0
        got = keep[k0 + 3].cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE)
        ref = keep[k0 + 4].cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE)
        same = all(np.array_equal(got[f], ref[f]) for f in ("in_flags", "err", "l3_offset", "l4_offset"))
        by = (frame + 22 * b.n) if sel else b.header_bytes()
        res[key] = {"parse": dict(line(p_ms, by), kernel=f"mi_cls_parse_kernel<ETH, CK={pl[5]}>",
                                  chksums=hex(sel), grid=pl[6]),
                    "classify": dict(line(c_ms, by), kernel=ll["name"], pktin_opt=hex(opt), grid=ll["grid"]),
                    "parse_fields_equal": bool(same),
                    "l4_chksum_done": int((got["in_flags"] >> 31).sum()),
                    "checksum_errors": int((got["err"] & 0x44 != 0).sum())}
        res[key]["parse_over_classify_median"] = round(
            res[key]["parse"]["us_per_launch_median"] / res[key]["classify"]["us_per_launch_median"], 3)
    res["one_packet_call"] = one_packet_call(p, b)
    p.close()
    c.close()
    s = json.dumps(res)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
