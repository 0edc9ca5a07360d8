#!/usr/bin/env python3
"""Register, scratch and LDS figures of every kernel of the library, from the
compiler alone (no GPU): each kernel translation unit is compiled for the
device with -Rpass-analysis=kernel-resource-usage and the remarks are printed
as one line per kernel, sorted by name.

  python tools/kernel_resources.py [--src DIR] [--out FILE]

--src: a copy of odp_amd/csrc to measure instead (e.g. another commit's, to
compare two trees: diff the two outputs).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from odp_amd import _build as B  # noqa: E402

KEYS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"),
        ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
        ("LDS Size [bytes/block]", "lds"))


def unit(src, src_dir, tmp):
    cmd = [B.HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-I", B.INC, "-I", src_dir, "-I", tmp,
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, src]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stdout)
    rows, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur:
            for k, short in KEYS:
                if t.startswith(k + ":"):
                    rows[cur][short] = t.split(":", 1)[1].strip()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=B.SRC)
    ap.add_argument("--out")
    a = ap.parse_args()
    srcs = sorted(glob.glob(os.path.join(a.src, "mi_cls_k*.hip")))
    tmp = tempfile.mkdtemp(prefix="mi_cls_res_")
    B.write_src_inc(os.path.join(tmp, "mi_cls_src.inc"), (), a.src)
    rows = {}
    with cf.ThreadPoolExecutor(max_workers=min(16, len(srcs))) as ex:
        for r in ex.map(lambda s: unit(s, a.src, tmp), srcs):
            rows.update(r)
    try:
        dem = subprocess.run(["c++filt"] + list(rows), stdout=subprocess.PIPE,
                             text=True).stdout.splitlines()
    except OSError:
        dem = list(rows)
    lines = []
    for name, d in zip(dem if len(dem) == len(rows) else list(rows), rows):
        v = rows[d]
        lines.append(f"{name}: " + " ".join(f"{s}={v.get(s, '?')}" for _, s in KEYS))
    text = "\n".join(sorted(lines)) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
