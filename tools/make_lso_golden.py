#!/usr/bin/env python3
"""Generate tests/golden/lso_frames.json from the reference tree's LSO test
data (data only, no code):

    tools/make_lso_golden.py <reference tree>

  * test/common/test_packet_custom.h, test_packet_ipv4.h -- the three frames
    of the LSO validation suite (test/validation/api/pktio/lso.c:77-79);
  * the LSO_TEST_* offsets, masks and values of lso.c:22-41;
  * the nine (frame, max_payload) cases of the suite (lso.c:1139-1153), each
    run there with per-packet metadata and with an opt argument.
The output is committed; tests read only the output.
"""
import json
import os
import re
import sys

from make_golden import c_arrays

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
FRAMES = {"test_packet_custom_eth_1": "test_packet_custom.h",
          "test_packet_ipv4_udp_325": "test_packet_ipv4.h",
          "test_packet_ipv4_udp_1500": "test_packet_ipv4.h"}
# (suite entry without its _pkt_meta / _opt suffix, frame, max_payload): lso.c:1105-1153, 973-1004
CASES = [("lso_send_ipv4_325_700", "test_packet_ipv4_udp_325", 700),
         ("lso_send_ipv4_1500_1000", "test_packet_ipv4_udp_1500", 1000),
         ("lso_send_ipv4_1500_700", "test_packet_ipv4_udp_1500", 700),
         ("lso_send_custom_eth_723_800", "test_packet_custom_eth_1", 800),
         ("lso_send_custom_eth_723_500", "test_packet_custom_eth_1", 500),
         ("lso_send_custom_eth_723_288", "test_packet_custom_eth_1", 288)]


def defines(path):
    """The LSO_TEST_* constants, evaluated (they are integer expressions of
    literals and of each other)."""
    out = {}
    for m in re.finditer(r"#define (LSO_TEST_\w+)\s+(.*?)\s*(?:/\*.*)?$", open(path).read(), re.M):
        expr = re.sub(r"LSO_TEST_\w+", lambda k: str(out[k.group(0)]), m.group(2))
        if re.fullmatch(r"[0-9a-fA-Fx()<>| ]+", expr):
            out[m.group(1)] = int(eval(expr))   # noqa: S307 (digits, shifts and ors only)
    return out


def main():
    ref = sys.argv[1]
    frames = {}
    for name, hdr in FRAMES.items():
        frames[name] = c_arrays(os.path.join(ref, "test/common", hdr))[name]
    lso_c = os.path.join(ref, "test/validation/api/pktio/lso.c")
    listed = re.findall(r"ODP_TEST_INFO_CONDITIONAL\((lso_send_\w+?)_(pkt_meta|opt),", open(lso_c).read())
    assert sorted({n for n, _ in listed}) == sorted(c[0] for c in CASES), listed
    # the nine pairs: the suite's twelve send entries name six (frame, payload)
    # pairs; the IPv4 ones run twice (as stored and with DF set, lso.c:1062-1083)
    cases = []
    for name, frame, mp in CASES:
        ipv4 = "ipv4" in name
        for df in ((False, True) if ipv4 else (False,)):
            cases.append({"suite_entry": name, "frame": frame, "max_payload": mp, "set_df": df,
                          "proto": "ipv4" if ipv4 else "custom",
                          "hdr_len": 34 if ipv4 else 22, "l3_offset": 14 if ipv4 else 0})
    assert len(cases) == 9
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "lso_frames.json"), "w") as f:
        json.dump({"source": "test/common/test_packet_{custom,ipv4}.h; test/validation/api/pktio/lso.c",
                   "frames": frames, "defines": defines(lso_c), "cases": cases}, f, indent=1, sort_keys=True)
    print({k: len(v) // 2 for k, v in frames.items()}, len(cases), "cases")


if __name__ == "__main__":
    main()
