#!/usr/bin/env python3
"""Writes tests/golden/tx_reference.json: about 300 cases of the transmit
corpus (tests/tx_ref_cases.py golden_slice(), drawn from every group) with
what the reference's own compiled transmit code makes of them
(oracle/_ref/libodp_ref.so: loopback_fix_checksums, get_dest_queue) -- the
output frame per pktout option row, in this project's layout (ref_output),
and the six queue indices per hash_proto row.  tests/test_tx_vs_reference.py
holds the models to it where the library was not built, and the library to it
where it was.

Needs the library: run odp_amd._build.build() where the reference tree is.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import tx_model as TX          # noqa: E402
from tests import tx_ref_cases as TC      # noqa: E402

OPTS = (TX.ALL_TX, TX.CK_UDP | TX.CK_IPV4, 0)
HPS = (63, 10, 0)
INDEX = 5


def main():
    idx = TC.golden_slice()
    cs = [TC.cases()[i] for i in idx]
    outs = {opt: TC.ref_fix(cs, opt) for opt in OPTS}
    res = {hp: TC.ref_queues(cs, hp, index=INDEX) for hp in HPS}
    doc = {
        "moduli": list(TC.MODULI), "opts": list(OPTS), "hash_protos": list(HPS), "index": INDEX,
        "cases": [{"i": i, "group": c.group, "frame": c.frame.hex(), "l3": c.l3, "l4": c.l4, "flags": c.flags,
                   "out": [None if outs[o][k] == c.frame else outs[o][k].hex() for o in OPTS],
                   "queues": [res[h][k].tolist() for h in HPS]}
                  for k, (i, c) in enumerate(zip(idx, cs))],
    }
    path = os.path.join(ROOT, "tests", "golden", "tx_reference.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(cs)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
