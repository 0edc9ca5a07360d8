"""LSO without a GPU: the model (tests/lso_model.py) against the reference
validation suite's own expectations on its frames, mi_cls_lso_plan against
the model, and the runtime's LSO API through tests/rt/lso_driver.c
(capability, profile create / destroy, the per-packet request, enable_lso)."""
import json
import os
import struct
import subprocess

import pytest

from tests import lso_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSO_DRIVER = os.path.join(ROOT, "tests", "_bin", "lso_driver")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "lso_frames.json")))
G = GOLD["defines"]
SEGNUM = (M.ADD_SEGMENT_NUM, G["LSO_TEST_CUSTOM_ETH_SEGNUM_OFFSET"], 2)
BITS = (M.WRITE_BITS, G["LSO_TEST_CUSTOM_ETH_BITS_OFFSET"], 1,
        (G["LSO_TEST_FIRST_SEG_MASK"], G["LSO_TEST_MIDDLE_SEG_MASK"], G["LSO_TEST_LAST_SEG_MASK"]),
        (G["LSO_TEST_FIRST_SEG_VALUE"], G["LSO_TEST_MIDDLE_SEG_VALUE"], G["LSO_TEST_LAST_SEG_VALUE"]))


# ---- the suite's expectations (lso.c:855-895, 1024-1044), applied to the
# original header for segment seg_num at payload offset seg_offset
def suite_segnum(hdr, seg_num, num_segs):
    struct.pack_into("!H", hdr, G["LSO_TEST_CUSTOM_ETH_SEGNUM_OFFSET"],
                     (seg_num + G["LSO_TEST_CUSTOM_ETH_SEGNUM"]) & 0xFFFF)


def suite_bits(hdr, seg_num, num_segs):
    o = G["LSO_TEST_CUSTOM_ETH_BITS_OFFSET"]
    w = "FIRST" if seg_num == 0 else ("MIDDLE" if seg_num < num_segs - 1 else "LAST")
    m, v = G[f"LSO_TEST_{w}_SEG_MASK"], G[f"LSO_TEST_{w}_SEG_VALUE"]
    hdr[o] = (hdr[o] & ~m & 0xFF) | (v & m)


def suite_ipv4(hdr, seg_num, num_segs, seg_offset, seg_len):
    l3 = 14
    f = (struct.unpack_from("!H", hdr, l3 + 6)[0] + seg_offset // 8) & 0xFFFF
    if seg_num < num_segs - 1:
        f |= G["LSO_TEST_IPV4_FLAG_MF"]
    struct.pack_into("!H", hdr, l3 + 2, seg_len - l3)
    struct.pack_into("!H", hdr, l3 + 6, f)
    hdr[l3 + 10:l3 + 12] = b"\0\0"
    s = sum(struct.unpack("!10H", bytes(hdr[l3:l3 + 20])))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    struct.pack_into("!H", hdr, l3 + 10, ~s & 0xFFFF)


def golden_frame(c):
    fr = bytearray(bytes.fromhex(GOLD["frames"][c["frame"]]))
    if c["proto"] == "ipv4" and c["set_df"]:
        struct.pack_into("!H", fr, 20, struct.unpack_from("!H", fr, 20)[0] | G["LSO_TEST_IPV4_FLAG_DF"])
    if c["proto"] == "custom":
        struct.pack_into("!H", fr, SEGNUM[1], G["LSO_TEST_CUSTOM_ETH_SEGNUM"])
    return bytes(fr)


def test_golden_fixture():
    assert {k: len(v) // 2 for k, v in GOLD["frames"].items()} == {
        "test_packet_custom_eth_1": 723, "test_packet_ipv4_udp_325": 325, "test_packet_ipv4_udp_1500": 1500}
    assert len(GOLD["cases"]) == 9
    assert (SEGNUM[1], BITS[1]) == (16, 16) and G["LSO_TEST_CUSTOM_ETH_SEGNUM"] == 0xAAFE


@pytest.mark.parametrize("ci", range(9))
def test_model_against_the_suite(ci):
    """What lso_test / pktin_recv_lso check (lso.c:755-848): the segments'
    payloads concatenate to the original's, every custom segment but the last
    is full, every header is the original's after the suite's own update,
    and the IPv4 header checksum verifies."""
    c = GOLD["cases"][ci]
    fr, hdr_len, mp = golden_frame(c), c["hdr_len"], c["max_payload"]
    if c["proto"] == "ipv4":
        variants = [((M.PROTO_IPV4, []), None)]
    else:
        variants = [((M.PROTO_CUSTOM, [SEGNUM]), (suite_segnum,)), ((M.PROTO_CUSTOM, [BITS]), (suite_bits,)),
                    ((M.PROTO_CUSTOM, [SEGNUM, BITS]), (suite_segnum, suite_bits))]
    for prof, upd in variants:
        st, segs = M.segments(fr, hdr_len, mp, prof, c["l3_offset"] if c["proto"] == "ipv4" else M.L3_INVALID)
        assert st == 0
        if hdr_len + mp > len(fr):
            assert segs == [fr]          # no segmentation: the packet itself
            continue
        assert len(segs) >= (3 if mp in (700, 288) else 2)
        assert b"".join(s[hdr_len:] for s in segs) == fr[hdr_len:]
        off = 0
        for k, s in enumerate(segs):
            pay = len(s) - hdr_len
            assert 0 < pay <= mp
            if c["proto"] == "custom" and k < len(segs) - 1:
                assert pay == mp
            exp = bytearray(fr[:hdr_len])
            if c["proto"] == "ipv4":
                suite_ipv4(exp, k, len(segs), off, len(s))
                assert M.inet_csum(s[14:34]) == 0
                if k < len(segs) - 1:
                    assert pay % 8 == 0
            else:
                for u in upd:
                    u(exp, k, len(segs))
            assert s[:hdr_len] == bytes(exp), (c["suite_entry"], k)
            off += pay


def plan_grid():
    for proto in (M.PROTO_CUSTOM, M.PROTO_IPV4):
        for hdr in (0, 14, 20, 33, 34, 127, 128, 129):
            for mp in (0, 1, 7, 8, 9, 15, 16, 100, 1448, 65535, 70000):
                for extra in (0, 1, 7, 8, 63 * 8, 64 * 8, 64 * 8 + 1, 9000, 65535):
                    for l3 in (0, 14, 15, hdr, M.L3_INVALID):
                        yield (hdr + extra if extra < 65535 else 65535, hdr, mp, proto, l3)
    yield (10, 11, 4, M.PROTO_CUSTOM, 0)          # hdr_len > len
    yield (64 * 3 + 20, 20, 3, M.PROTO_CUSTOM, 0)     # 64 segments
    yield (64 * 3 + 21, 20, 3, M.PROTO_CUSTOM, 0)     # 65


def test_plan_matches_model(built):
    from odp_amd.cls import lso_plan
    n = 0
    seen = set()
    for length, hdr, mp, proto, l3 in plan_grid():
        exp = M.plan(length, hdr, mp, proto, l3)
        assert lso_plan(length, hdr, mp, proto, l3) == exp, (length, hdr, mp, proto, l3)
        seen.add(min(exp[0], 2))
        n += 1
    assert seen == {-M.EINVAL, 1, 2} and n > 5000
    # the documented deviation: a payload length of 0 is an error, not a division
    assert lso_plan(100, 20, 0, M.PROTO_CUSTOM, 0)[0] == -M.EINVAL
    assert lso_plan(100, 34, 7, M.PROTO_IPV4, 14)[0] == -M.EINVAL
    assert lso_plan(100, 34, 8, M.PROTO_IPV4, 14) == (9, 8, 2)
    assert lso_plan(100, 34, 70, M.PROTO_IPV4, 14) == (1, 70, 0)     # goes out whole: not rounded


def test_segment_entries_without_a_gpu(built):
    """A null context: -ENODEV where there is no device; a bad profile table:
    -EINVAL before that."""
    import ctypes as C
    import numpy as np
    from odp_amd.cls import lib, lso_profiles
    nodev = -19 if lib().mi_cls_device_count() == 0 else -22     # with a device: a null context
    lay = M.Layout([(bytes(200), 22, 40, 0, M.L3_INVALID)], [(M.PROTO_CUSTOM, [])])
    st = np.zeros(1, np.uint8)

    def host(prof):
        return lib().mi_cls_lso_segment_host(None, lay.buf.ctypes.data, lay.buf.nbytes, lay.off.ctypes.data,
                                             lay.len.ctypes.data, lay.desc.ctypes.data, 1, lay.buf.ctypes.data,
                                             lay.buf.nbytes, lay.seg.ctypes.data, len(lay.seg),
                                             C.cast(prof, C.c_void_p), len(prof), st.ctypes.data)

    assert host(lso_profiles([(M.PROTO_CUSTOM, [])])) == nodev
    assert host(lso_profiles([(3, [])])) == -22
    assert host(lso_profiles([(M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, 0, 3)])])) == -22


@pytest.fixture(scope="module")
def surface(built, tmp_path_factory):
    from tests.rt_helpers import write_pcap
    pcap = str(tmp_path_factory.mktemp("lso") / "one.pcap")
    write_pcap(pcap, [bytes(64)])
    r = subprocess.run([LSO_DRIVER, "surface", pcap], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        p = line.split()
        out[(p[0], p[1])] = p[2:]
    return out


def test_capability(surface):
    """odp_packet_io.c:1566-1577, the same for every driver."""
    for drv in ("loop", "pcap"):
        mtu = int(surface[("MTU", drv)][0])
        assert surface[("CAP", drv)] == ["16", "16", "1", "64", str(mtu - 14), "128", "8", "1100000", "1001"]


def test_enable_lso_is_accepted(surface):
    assert surface[("CFG", "loop")] == ["0"] and surface[("CFG", "pcap")] == ["0"]


def test_profile_create_and_destroy(surface):
    ok = {"proto1", "proto2", "segnum1", "segnum2", "segnum4", "segnum8", "bits1", "custom8", "ipv4_ignores_custom",
          "slot_reused"}
    bad = {"none", "proto3", "proto4", "proto5", "proto6", "proto7", "segnum3", "segnum0", "segnum16", "offset129",
           "bits2", "bits_offset129", "payload_len", "payload_offset", "op0", "op6", "custom9", "seventeenth"}
    got = {k[1]: v for k, v in surface.items() if k[0] == "PROF"}
    assert set(got) == ok | bad | {"sixteen"}
    for name in ok:
        assert got[name] == ["1"], name
    for name in bad:
        assert got[name] == ["0"], name
    assert got["sixteen"] == ["16"]
    assert surface[("INIT", "0")] == ["0"]
    assert surface[("DESTROY", "live")] == ["0"]
    assert surface[("DESTROY", "stale")] == ["-1"] and surface[("DESTROY", "invalid")] == ["-1"]


def test_packet_request(surface):
    inv = "65535"
    assert surface[("REQ", "fresh")] == ["0", inv]
    assert surface[("REQ", "ok")] == ["0", "1", "34"]
    assert surface[("REQ", "clr")] == ["0", "34"]             # the payload offset stays
    assert surface[("REQ", "offset_set")] == ["0", "77"]
    assert surface[("REQ", "past_packet")] == ["-1", "0"]
    assert surface[("REQ", "at_end")] == ["0"]
    assert surface[("REQ", "offset129")] == ["-1"] and surface[("REQ", "offset128")] == ["0"]
    assert surface[("REQ", "invalid_profile")] == ["-1", "0"] and surface[("REQ", "stale_profile")] == ["-1"]
    assert surface[("REQ", "realloc")] == ["0", inv]
    # the setter keeps 16 bits: a value that does not fit, or that is the INVALID value, is refused
    assert surface[("REQ", "offset_set_65535")] == ["-1", "77"] and surface[("REQ", "offset_set_wide")] == ["-1", "77"]
    assert surface[("REQ", "offset_set_65534")] == ["0", "65534"]


def test_send_lso_on_a_pktio_that_is_not_started(surface):
    """Where there is no GPU no pktio starts: the call returns -1 (num <= 0 and
    a missing request too), with per-packet metadata and with opt, and the
    packet stays with the caller as it was."""
    assert surface[("SEND", "num0")] == ["-1"] and surface[("SEND", "norequest")] == ["-1"]
    assert surface[("SEND", "notstarted")] == ["0", "-1", "-1"]
    assert surface[("SEND", "kept")] == ["1", "400"]
