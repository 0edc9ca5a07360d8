"""Input queues and the pktin flow hash of the loop pktio, CPU side: the
model's CRC and the runtime's odp_hash_crc32c held to CRCs recorded from the
reference's _odp_hash_crc32c_generic (tests/golden/txq_hash.json; called live
too where the reference library was built), the model's byte strings, the
runtime's API surface (capability, odp_pktin_queue_config rules, the queue
handles, the flag setters) and the host-side queue pick / run splitting under
the address and undefined-behaviour sanitizers -- none of it needs a GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np

from odp_amd import pktgen as pg
from tests import chksum_frames as CK
from tests import txq_model as TQ
from tests.rt_helpers import write_pcap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MQ_DRIVER = os.path.join(ROOT, "tests", "_bin", "mq_driver")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libodp_ref.so")


def _pairs():
    with open(os.path.join(ROOT, "tests", "golden", "txq_hash.json")) as f:
        pairs = [(bytes.fromhex(h), c) for h, c in json.load(f)["pairs"]]
    assert len(pairs) >= 300 and {len(s) for s, _ in pairs} == {0, 4, 8, 12, 32, 36}
    return pairs


def test_crc_against_reference_fixture(built):
    pairs = _pairs()
    for s, crc in pairs:
        assert TQ.crc32c_raw(s) == crc, s.hex()
    assert TQ.crc32c_raw(b"") == 0
    # the runtime's odp_hash_crc32c
    r = subprocess.run([MQ_DRIVER, "crc"], input="".join(s.hex() + "\n" for s, _ in pairs),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-1000:]
    got = [int(ln.split()[1], 16) for ln in r.stdout.splitlines() if ln.startswith("C ")]
    assert got == [c for _, c in pairs]
    # and the reference's own compiled code, where it was built
    if os.path.exists(REFLIB):
        f = ctypes.CDLL(REFLIB)._odp_hash_crc32c_generic
        f.restype, f.argtypes = ctypes.c_uint32, [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
        for s, crc in pairs:
            assert f(s, len(s), 0) == crc, s.hex()


def test_model_strings():
    """get_dest_queue's string: the L4 step, then the L3 step, each by the
    metadata flags and the fit of its header."""
    rng = np.random.default_rng(2)
    u4, l3, l4 = CK.build(rng, 4, pg.IPPROTO_UDP, payload=b"x" * 30)
    t6, l36, l46 = CK.build(rng, 6, pg.IPPROTO_TCP, payload=b"y" * 30)
    U, T, V4, V6 = TQ.F_UDP, TQ.F_TCP, TQ.F_IPV4, TQ.F_IPV6
    hs = TQ.hash_string
    assert hs(u4, l3, l4, U | V4, TQ.HP_ALL) == u4[l4:l4 + 4] + u4[l3 + 12:l3 + 20]
    assert hs(u4, l3, l4, U | V4, TQ.HP_IPV4_UDP) == u4[l4:l4 + 4]          # ports alone
    assert hs(u4, l3, l4, U | V4, TQ.HP_IPV6_UDP) == u4[l4:l4 + 4]          # the IP version is not looked at
    assert hs(u4, l3, l4, U | V4, TQ.HP_IPV4) == u4[l3 + 12:l3 + 20]
    assert hs(u4, l3, l4, U | V4, TQ.HP_IPV4_TCP | TQ.HP_IPV6) == b""
    assert hs(t6, l36, l46, T | V6, TQ.HP_ALL) == t6[l46:l46 + 4] + t6[l36 + 8:l36 + 40]
    assert hs(t6, l36, l46, T | V6, TQ.HP_IPV4_UDP | TQ.HP_IPV4) == b""
    assert hs(u4[:l4 + 7], l3, l4, U | T | V4, TQ.HP_ALL) == u4[l3 + 12:l3 + 20]   # no TCP try after UDP
    assert hs(u4, TQ.INVALID, l4, U | V4, TQ.HP_ALL) == u4[l4:l4 + 4]
    assert hs(u4, l3, TQ.INVALID, U | V4, TQ.HP_ALL) == u4[l3 + 12:l3 + 20]
    assert TQ.flow_hash(u4, l3, l4, 0, TQ.HP_ALL) == (0, 0)
    assert TQ.dest_queue(0x12345678, 4, 0, 6) == 2 and TQ.dest_queue(0x12345679, 4, 63, 6) == 1


def test_api_surface(built, tmp_path):
    pcap = str(tmp_path / "one.pcap")
    write_pcap(pcap, [CK.build(np.random.default_rng(1), 4, pg.IPPROTO_UDP)[0]])
    r = subprocess.run([MQ_DRIVER, "surface", pcap], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines()]
    caps = {p[1]: p[2:] for p in lines if p[0] == "CAP"}
    assert caps["loop"] == ["64", "0xf", "0x3"]      # loop.c:723-728
    assert caps["pcap"] == ["1", "0x0", "0x0"]
    cfg = {(p[1], p[2], int(p[3]), int(p[4])): (int(p[5]), int(p[6])) for p in lines if p[0] == "CFG"}
    for mode in ("direct", "sched"):
        assert cfg[("loop", mode, 4, 0)] == (0, 4)
        assert cfg[("loop", mode, 64, 0)] == (0, 64)
        assert cfg[("loop", mode, 2, 0)] == (0, 2)
        assert cfg[("loop", mode, 1, 0)] == (0, 1)
        assert cfg[("loop", mode, 0, 0)][0] == -1
        assert cfg[("loop", mode, 65, 0)][0] == -1
        assert cfg[("loop", mode, 4, 1)] == (0, 1)   # classifier on: one queue
        assert cfg[("loop", mode, 0, 1)] == (0, 1)
    assert cfg[("pcap", "direct", 1, 0)] == (0, 1)
    for n in (4, 64, 2, 0, 65):
        assert cfg[("pcap", "direct", n, 0)][0] == -1
    assert cfg[("pcap", "direct", 4, 1)] == (0, 1)
    # the handles: indices 0 .. n - 1; the event queues distinct (checked by the driver) and named
    qs = [p[1:] for p in lines if p[0] == "Q"]
    assert [str(i) for i in range(4)] in qs and [str(i) for i in range(64)] in qs
    es = [p[1:] for p in lines if p[0] == "E"]
    assert any(len(e) == 4 and [n.rsplit("-", 1)[1] for n in e] == ["0", "1", "2", "3"] and
               all(n.startswith("odp-pktin-") for n in e) for e in es)
    flags = [p[1:] for p in lines if p[0] == "FLAGS"][0]
    assert flags == ["1000", "1100", "1110", "1111", "0101", "0000"]


def test_queue_pick_and_runs_sanitized(tmp_path):
    """tests/rt/txq_unit.c over odp_amd/csrc/odp_txq.h, a stand-alone program
    built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "txq_unit")
    c = subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "odp_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "rt", "txq_unit.c")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert c.returncode == 0, c.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stderr[-3000:])
