"""pktout checksum insertion, CPU side: the model of the rules
(tests/tx_model.py) pinned against frames whose checksums are valid by
construction and against the oracle's receive validation, and the runtime's
API surface on a loop pktio (capability, config, the override setters) --
none of it needs a GPU."""
import os
import subprocess

import numpy as np
import pytest

from odp_amd import pktgen as pg
from oracle import oracle as O
from tests import chksum_frames as CK
from tests import tx_model as TX
from tests.rt_helpers import write_pcap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_DRIVER = os.path.join(ROOT, "tests", "_bin", "tx_driver")


def test_offsets_match_builder():
    rng = np.random.default_rng(1)
    for ver in (4, 6):
        for proto in (pg.IPPROTO_UDP, pg.IPPROTO_TCP, pg.IPPROTO_SCTP):
            for vlan in (False, True):
                fr, l3, l4 = CK.build(rng, ver, proto, vlan=vlan, ipopt=ver == 4)
                assert TX.offsets_of(fr) == (l3, l4)


def test_model_restores_valid_frames(built):
    """Scramble the checksum fields of valid frames, apply the model with all
    four defaults on: the original bytes come back (a UDP zero checksum
    becomes the computed one), and the oracle's receive validation passes
    every checksum."""
    seen = set()
    frames = TX.valid_frames()
    assert len(frames) >= 400
    for fr, udp_zero in frames:
        l3, l4 = TX.offsets_of(fr)
        bad = TX.scramble(fr, l3, l4)
        assert bad != fr
        got, done = TX.insert(bad, l3, l4, 0, TX.ALL_TX)
        v4 = fr[l3] >> 4 == 4
        proto = fr[l3 + 9] if v4 else fr[l3 + 6]
        want = (TX.DONE_IPV4 if v4 else 0) | {17: TX.DONE_UDP, 6: TX.DONE_TCP, 132: TX.DONE_SCTP}[proto]
        assert done == want, fr.hex()
        seen.add((v4, proto))
        if udp_zero:
            assert got[:l4 + 6] == fr[:l4 + 6] and got[l4 + 8:] == fr[l4 + 8:]
            assert got[l4 + 6:l4 + 8] != b"\x00\x00"
        else:
            assert got == fr, fr.hex()
        r, f, e, _, pl3, pl4 = O.parse(got, CK.ALL_CK)
        assert (pl3, pl4) == (l3, l4)
        assert r == 0 and e == 0, fr.hex()
        assert f & CK.L4_DONE and (not v4 or f & CK.L3_DONE), fr.hex()
        # the scrambled frame does fail: the test sees the difference
        r, f, e, _, _, _ = O.parse(bad, CK.ALL_CK)
        assert e & (CK.E_L3CK | CK.E_L4CK), fr.hex()
    assert len(seen) == 6


def test_model_decisions():
    """Defaults, overrides and the leave-unchanged rules of the model."""
    rng = np.random.default_rng(5)
    fr, l3, l4 = CK.build(rng, 4, pg.IPPROTO_UDP)
    bad = TX.scramble(fr, l3, l4)
    assert TX.insert(bad, l3, l4, 0, 0) == (bad, 0)
    assert TX.insert(bad, l3, l4, TX.L3_SET | TX.L3_CK | TX.L4_SET | TX.L4_CK, 0) == \
        (fr, TX.DONE_IPV4 | TX.DONE_UDP)
    assert TX.insert(bad, l3, l4, TX.L3_SET | TX.L4_SET, TX.ALL_TX) == (bad, 0)
    assert TX.insert(bad, l3, l4, TX.L3_CK | TX.L4_CK, 0) == (bad, 0)   # _set bits off
    assert TX.insert(bad, l3, l4, 0, TX.ALL_ENA) == (bad, 0)            # _ena not consulted
    assert TX.insert(bad, TX.INVALID, l4, 0, TX.ALL_TX) == (bad, 0)
    got, done = TX.insert(bad, l3, TX.INVALID, 0, TX.ALL_TX)
    assert done == TX.DONE_IPV4 and got[l4:] == bad[l4:]
    got, done = TX.insert(bad, l3, l4, 0, TX.CK_TCP | TX.CK_SCTP)
    assert (got, done) == (bad, 0)
    # TCP: stored at l4 + 16 (the deviation), never at l4 + 6
    fr, l3, l4 = CK.build(rng, 6, pg.IPPROTO_TCP)
    bad = TX.scramble(fr, l3, l4)
    got, done = TX.insert(bad, l3, l4, 0, TX.CK_TCP)
    assert (got, done) == (fr, TX.DONE_TCP) and got[l4 + 4:l4 + 8] == bad[l4 + 4:l4 + 8]


@pytest.fixture(scope="module")
def surface(built, tmp_path_factory):
    rng = np.random.default_rng(2)
    pcap = str(tmp_path_factory.mktemp("tx") / "one.pcap")
    write_pcap(pcap, [CK.build(rng)[0]])
    r = subprocess.run([TX_DRIVER, "surface", pcap], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()]


def test_loop_capability_reports_pktout_checksums(surface):
    caps = {p[1]: int(p[2], 16) for p in surface if p[0] == "CAP"}
    assert caps["loop"] == TX.all_bits(TX.ALL_TX | TX.ALL_ENA) == 0x1FE
    assert caps["pcap"] == 0


def test_loop_config_accepts_pktout_checksums(surface):
    cfg = {(p[1], int(p[2], 16)): int(p[3]) for p in surface if p[0] == "CFG"}
    for opt in (TX.ALL_TX | TX.ALL_ENA, TX.CK_IPV4, TX.CK_UDP, TX.CK_TCP, TX.CK_SCTP, TX.ALL_ENA):
        bits = TX.all_bits(opt)
        assert cfg[("loop", bits)] == 0, hex(bits)
        assert cfg[("pcap", bits)] == -1, hex(bits)
    # the bits are the reference header's: ipv4_chksum is bit 5 (bit 0 is ts_ena)
    assert [TX.all_bits(o) for o in (TX.CK_IPV4, TX.CK_SCTP, TX.ALL_ENA)] == [0x20, 0x100, 0x1E]
    # no_packet_refs (bit 9) and ts_ena (bit 0) are not offered
    for bits in (0x200, TX.TS_ENA, TX.TS_ENA | TX.all_bits(TX.ALL_TX | TX.ALL_ENA)):
        assert cfg[("loop", bits)] == -1 and cfg[("pcap", bits)] == -1, hex(bits)


def test_override_setters_exist(surface):
    assert ["OVR", "ok"] in surface
