#!/usr/bin/env python3
"""Wall time of the LSO path, recorded (not a pass criterion):

  (a) one mi_cls_lso_segment_host call on page-locked memory (sources,
      segments, descriptors, segment table and status bytes: the kernel works
      in place over the host link) for 1 x 9000 B, 64 x 9000 B and
      64 x 65535 B sources cut into 1448-B segments behind a 64-B header,
      custom profile (one 2-byte ADD_SEGMENT_NUM);
  (b) one odp_pktout_send_lso burst of 64 x 9000 B through a loop pktio
      (tests/_bin/lso_driver bench): plan, allocation, the launch and the send.

Per case: median and min over the rounds of the mean call time of a round,
and the bytes a call moves over the host link (read: every segment's header
and payload, 24 B of descriptors per source, 8 B per segment; written: the
segments and a status byte per source).

  python tools/lso_bench.py [--rounds 7] [--steps 50] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HDR, PAY = 64, 1448


def host_case(ctx, n, length, a):
    from odp_amd.cls import LSO_ADD_SEGMENT_NUM, LSO_PROTO_CUSTOM, PinnedArray, lso_profiles
    from tests import lso_model as M
    profiles = [(LSO_PROTO_CUSTOM, [(LSO_ADD_SEGMENT_NUM, 16, 2)])]
    rng = np.random.default_rng(n + length)
    frames = [bytes(rng.integers(0, 256, length).astype(np.uint8)) for _ in range(n)]
    lay = M.Layout([(f, HDR, PAY, 0, M.L3_INVALID) for f in frames], profiles, src_res=lambda i: 0,
                   dst_res=lambda i, k: 0, gap=64)
    exp, _ = M.apply(lay.buf, lay.off, lay.len, lay.desc, lay.seg, profiles)
    ns = len(lay.seg)
    pins = [PinnedArray(lay.buf.nbytes), PinnedArray(4 * n), PinnedArray(2 * n), PinnedArray(16 * n),
            PinnedArray(8 * ns), PinnedArray(n)]
    try:
        buf, off, ln = pins[0].u8, pins[1].view(np.uint32, n), pins[2].view(np.uint16, n)
        desc, seg, st = pins[3].view(M.DESC_DTYPE, n), pins[4].view(M.SEG_DTYPE, ns), pins[5].u8
        buf[:], off[:], ln[:], desc[:], seg[:] = lay.buf, lay.off, lay.len, lay.desc, lay.seg
        prof = lso_profiles(profiles)

        def call():
            rc = ctx.segment_host(buf, off, ln, desc, buf, seg, prof, st)
            if rc:
                raise RuntimeError(f"mi_cls_lso_segment_host: {rc}")

        for _ in range(a.warmup):
            call()
        us = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call()
            us.append((time.perf_counter() - t0) / a.steps * 1e6)
        ok = bool(np.array_equal(buf, exp)) and not st[:n].any()
    finally:
        for p in pins:
            p.close()
    seg_bytes = int(sum(HDR + min(PAY, length - HDR - k * PAY) for k in range(ns // n))) * n
    med = statistics.median(us)
    return {"sources": n, "source_bytes": length, "segments": ns, "us_per_call_median": round(med, 1),
            "us_per_call_min": round(min(us), 1), "rounds_us": [round(x, 1) for x in us],
            "host_link_bytes_read": seg_bytes + 24 * n + 8 * ns, "host_link_bytes_written": seg_bytes + n,
            "gbytes_per_s_written_median": round(seg_bytes / med / 1e3, 2), "bytes_equal_model": ok}


def send_case(a):
    drv = os.path.join(ROOT, "tests", "_bin", "lso_driver")
    r = subprocess.run([drv, "bench", "64", "9000", str(HDR), str(PAY), str(a.rounds * 3)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    if r.returncode:
        raise RuntimeError(f"lso_driver rc={r.returncode}: {r.stderr[-500:]}")
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("B ")]
    us = [int(w[1]) / 1e3 for w in rows]
    return {"sources": 64, "source_bytes": 9000, "us_per_call_median": round(statistics.median(us), 1),
            "us_per_call_min": round(min(us), 1), "calls": len(us),
            "all_sent": all(w[2] == "64" for w in rows), "segments_received": sorted({int(w[3]) for w in rows})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    from odp_amd import _build
    from odp_amd.cls import LsoContext, lib
    _build.build()
    if lib().mi_cls_device_count() <= 0:
        raise SystemExit("lso_bench: no GPU")
    ctx = LsoContext(0)
    res = {"header_bytes": HDR, "segment_payload": PAY, "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup,
           "segment_host": [host_case(ctx, n, length, a) for n, length in ((1, 9000), (64, 9000), (64, 65535))]}
    ctx.close()
    res["pktout_send_lso"] = send_case(a)
    s = json.dumps(res)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
