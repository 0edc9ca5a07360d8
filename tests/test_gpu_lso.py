"""LSO segmentation on the GPU (mi_cls_lso_segment, its host entries and
odp_pktout_send_lso on the loop pktio) vs the model of the reference's rules
(tests/lso_model.py): the whole buffer byte for byte -- sources, segments and
the guard bytes between them, so a stray store shows -- and the st bytes.
All comparisons are exact."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import lso_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSO_DRIVER = os.path.join(ROOT, "tests", "_bin", "lso_driver")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "lso_frames.json")))
G = GOLD["defines"]

SEGNUM = (M.ADD_SEGMENT_NUM, G["LSO_TEST_CUSTOM_ETH_SEGNUM_OFFSET"], 2)
BITS = (M.WRITE_BITS, G["LSO_TEST_CUSTOM_ETH_BITS_OFFSET"], 1,
        (G["LSO_TEST_FIRST_SEG_MASK"], G["LSO_TEST_MIDDLE_SEG_MASK"], G["LSO_TEST_LAST_SEG_MASK"]),
        (G["LSO_TEST_FIRST_SEG_VALUE"], G["LSO_TEST_MIDDLE_SEG_VALUE"], G["LSO_TEST_LAST_SEG_VALUE"]))
# the profile table of most tests: IPv4, the suite's three custom profiles, none
P_IPV4, P_SEGNUM, P_BITS, P_BOTH, P_NONE = range(5)
PROFILES = [(M.PROTO_IPV4, []), (M.PROTO_CUSTOM, [SEGNUM]), (M.PROTO_CUSTOM, [BITS]),
            (M.PROTO_CUSTOM, [SEGNUM, BITS]), (M.PROTO_CUSTOM, [])]


@pytest.fixture(scope="module")
def lso(built, gpu):
    from odp_amd.cls import LsoContext
    c = LsoContext(0)
    yield c
    c.close()


def check(lso, items, profiles=PROFILES, what="", want_st=None, **layout):
    """GPU == model over the whole buffer, and the st bytes."""
    from odp_amd.cls import lso_profiles
    lay = M.Layout(items, profiles, **layout)
    exp, exp_st = M.apply(lay.buf, lay.off, lay.len, lay.desc, lay.seg, profiles)
    buf, st = lso.segment(lay.buf, lay.off, lay.len, lay.desc, lay.seg, lso_profiles(profiles))
    assert np.array_equal(st, exp_st), (what, st.tolist()[:16], exp_st.tolist()[:16])
    if want_st is not None:
        assert st.tolist() == list(want_st), (what, st.tolist())
    bad = np.nonzero(buf != exp)[0]
    if bad.size:
        o = int(bad[0])
        j = int(np.searchsorted(lay.seg["off"], o, side="right")) - 1
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {o} (segment entry {j} + "
                             f"{o - int(lay.seg['off'][j])}, source {int(lay.seg['src'][j])}, "
                             f"desc {lay.desc[int(lay.seg['src'][j])]}): gpu {buf[o]:#x} model {exp[o]:#x}")
    return lay, buf, st


def rand_frame(rng, length):
    return bytes(rng.integers(0, 256, length).astype(np.uint8))


def ip_frame(rng, length, l3=14, frag=0, ver_ihl=0x45):
    """Random bytes with an IPv4 header's first byte and fragment word at l3."""
    b = bytearray(rand_frame(rng, length))
    b[l3] = ver_ihl
    struct.pack_into("!H", b, l3 + 6, frag)
    return bytes(b)


def golden_items():
    """The suite's cases that segment, IPv4 as stored and with DF, the custom
    frame with the suite's segment number in place, under each of its three
    profiles (lso.c:921-971, 1062-1083)."""
    items = []
    for c in GOLD["cases"]:
        fr = bytearray(bytes.fromhex(GOLD["frames"][c["frame"]]))
        if c["proto"] == "ipv4":
            if c["set_df"]:
                f = struct.unpack_from("!H", fr, 20)[0] | G["LSO_TEST_IPV4_FLAG_DF"]
                struct.pack_into("!H", fr, 20, f)
                fr[24:26] = b"\0\0"       # and the header checksum again (lso.c:1046-1060)
                struct.pack_into("!H", fr, 24, M.inet_csum(bytes(fr[14:34])))
            profs = [P_IPV4]
        else:
            struct.pack_into("!H", fr, SEGNUM[1], G["LSO_TEST_CUSTOM_ETH_SEGNUM"])
            profs = [P_SEGNUM, P_BITS, P_BOTH]
        for p in profs:
            l3 = c["l3_offset"] if c["proto"] == "ipv4" else M.L3_INVALID
            items.append((bytes(fr), c["hdr_len"], c["max_payload"], p, l3))
    return items


def test_golden_cases(lso):
    items = golden_items()
    assert len(items) == 6 + 9
    one = [it for it in items if M.plan(len(it[0]), it[1], it[2], PROFILES[it[3]][0], it[4])[0] == 1]
    many = [it for it in items if it not in one]
    assert len(one) == 2 + 3 and len(many) == 4 + 6     # 325/700 and 723/800 go out whole
    check(lso, many, what="golden", want_st=[0] * len(many))
    assert lso.last_launch()[0] == 68


@pytest.mark.parametrize("hdr", [14, 15, 22, 34, 63, 64, 65, 127, 128])
def test_hdr_len(lso, hdr):
    rng = np.random.default_rng(hdr)
    prof = [(M.PROTO_IPV4, []), (M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, hdr - 2, 2), (M.ADD_SEGMENT_NUM, 0, 4)]),
            (M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, hdr - 8, 8)])]
    items = []
    for pay, left in ((40, 3), (200, 0), (16, 15)):
        ln = hdr + 2 * pay + left
        items.append((rand_frame(rng, ln), hdr, pay, 1, M.L3_INVALID))
        items.append((rand_frame(rng, ln), hdr, pay, 2, M.L3_INVALID))
        for l3 in ({0, hdr - 20} if hdr >= 20 else ()):
            items.append((ip_frame(rng, ln, l3), hdr, pay, 0, l3))
    check(lso, items, prof, f"hdr {hdr}", want_st=[0] * len(items))


@pytest.mark.parametrize("pay", [1, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 1448])
def test_payload_and_left_over(lso, pay):
    rng = np.random.default_rng(pay)
    items = []
    for left in sorted({0, 1, 15, 16, pay - 1}):
        if left >= pay:
            continue
        for hdr in (22, 34):
            ln = hdr + 2 * pay + left
            items.append((rand_frame(rng, ln), hdr, pay, P_BOTH, M.L3_INVALID))
            if pay % 8 == 0 and hdr == 34:   # max_payload rounds down to pay
                items.append((ip_frame(rng, ln), hdr, pay + 5, P_IPV4, 14))
    check(lso, items, what=f"payload {pay}", want_st=[0] * len(items), src_res=lambda i: 3 * i,
          dst_res=lambda i, k: 5 * i + 7 * k)


@pytest.mark.parametrize("nseg", [2, 3, 63, 64])
def test_nseg(lso, nseg):
    rng = np.random.default_rng(nseg)
    items = []
    for pay, left in ((8, 0), (24, 5), (17, 16)):
        ln = 34 + (nseg - (1 if left else 0)) * pay + left
        items.append((rand_frame(rng, ln), 34, pay, P_BOTH, M.L3_INVALID))
        if pay % 8 == 0:
            items.append((ip_frame(rng, ln), 34, pay, P_IPV4, 14))
    lay, _, _ = check(lso, items, what=f"nseg {nseg}", want_st=[0] * len(items))
    assert (lay.desc["nseg"] == nseg).all()


def test_every_alignment(lso):
    """Source and destination offsets at every pair of residues mod 16, with
    segments short enough to end inside the head and long enough for the
    16-byte pieces and a tail."""
    rng = np.random.default_rng(5)
    items = []
    for i in range(256):
        pay = (40, 200, 129, 16)[i % 4]
        ln = 34 + 2 * pay + (i % 7)
        items.append((ip_frame(rng, ln) if pay % 8 == 0 else rand_frame(rng, ln), 34, pay,
                      P_IPV4 if pay % 8 == 0 else P_BOTH, 14))
    check(lso, items, what="alignment", want_st=[0] * 256, src_res=lambda i: i % 16,
          dst_res=lambda i, k: (i // 16 + 5 * k) % 16, gap=3)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(lso, n):
    rng = np.random.default_rng(n)
    items = []
    for i in range(n):
        p = i % 5
        pay = int(rng.integers(1, 40)) * 8
        ln = 34 + int(rng.integers(pay + 1, 4 * pay))
        items.append((ip_frame(rng, ln) if p == P_IPV4 else rand_frame(rng, ln), 34, pay, p,
                      14 if p == P_IPV4 else M.L3_INVALID))
    check(lso, items, what=f"n={n}", want_st=[0] * n)


def test_65535_byte_source(lso):
    """The longest frame the batch contract admits (lengths are 16 bits, so
    seg_len - l3 always fits tot_len: nothing is truncated): 46 segments of
    1448 bytes, two of 32768, and 64 custom ones behind a 128-byte header --
    the most 16-byte rounds per wave and the largest offsets."""
    rng = np.random.default_rng(65535)
    items = [(ip_frame(rng, 65535), 34, 1448, P_IPV4, 14), (ip_frame(rng, 65535), 34, 32768, P_IPV4, 14),
             (rand_frame(rng, 65535), 128, 1024, P_BOTH, M.L3_INVALID)]
    lay, _, _ = check(lso, items, what="65535", want_st=[0, 0, 0])
    assert lay.desc["nseg"].tolist() == [46, 2, 64]


def test_fragment_word_inputs(lso):
    """DF, MF, a nonzero offset, and an offset whose sum carries into the flag
    bits (16-bit arithmetic, odp_packet_io.c:3005-3012)."""
    rng = np.random.default_rng(6)
    items = [(ip_frame(rng, 34 + 3 * 64 + 9, frag=f), 34, 64, P_IPV4, 14)
             for f in (0x4000, 0x2000, 0x0123, 0x6005, 0x1FFF, 0xFFFF, 0x9FF8)]
    lay, buf, _ = check(lso, items, what="fragment word", want_st=[0] * len(items))
    o = int(lay.seg["off"][int(lay.desc["first_seg"][4]) + 1]) + 14 + 6
    assert struct.unpack_from("!H", bytes(buf[o:o + 2]))[0] == ((0x1FFF + 8) | 0x2000)   # carried into MF


def test_ihl_fails_the_packet(lso):
    rng = np.random.default_rng(7)
    mk = lambda b: (ip_frame(rng, 34 + 100, ver_ihl=b), 34, 40, P_IPV4, 14)   # noqa: E731
    items = [mk(0x45), mk(0x46), mk(0x45), mk(0x44), mk(0x45), mk(0x4F), mk(0x40)]
    check(lso, items, what="ihl", want_st=[0, M.ST_IHL, 0, M.ST_IHL, 0, M.ST_IHL, M.ST_IHL])


def test_field_edges(lso):
    """A field straddling hdr_len (its tail bytes are payload bytes of the
    segment), a field ending exactly at the short last segment's end, and
    one byte past it (the packet fails; its neighbours are intact)."""
    rng = np.random.default_rng(8)
    prof = [(M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, 20, 4)]),     # hdr 22: bytes 22, 23 are payload
            (M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, 124, 8)]),    # hdr 128: reaches 132
            (M.PROTO_CUSTOM, [(M.WRITE_BITS, 128, 1, (0xF0,) * 3, (0xA0, 0xB0, 0xC0)),
                              (M.ADD_SEGMENT_NUM, 128, 8)])]    # offset 128, to 136
    items = [(rand_frame(rng, 22 + 2 * 50 + 2), 22, 50, 0, M.L3_INVALID),      # last: 24 bytes: ends at it
             (rand_frame(rng, 22 + 2 * 50 + 1), 22, 50, 0, M.L3_INVALID),      # last: 23 bytes: past it
             (rand_frame(rng, 128 + 2 * 50 + 4), 128, 50, 1, M.L3_INVALID),
             (rand_frame(rng, 128 + 2 * 50 + 3), 128, 50, 1, M.L3_INVALID),
             (rand_frame(rng, 128 + 3 * 20 + 8), 128, 20, 2, M.L3_INVALID),
             (rand_frame(rng, 128 + 3 * 20 + 7), 128, 20, 2, M.L3_INVALID),
             (rand_frame(rng, 22 + 2 * 50 + 30), 22, 50, 0, M.L3_INVALID)]
    check(lso, items, prof, "field edges", want_st=[0, M.ST_FIELD, 0, M.ST_FIELD, 0, M.ST_FIELD, 0],
          dst_res=lambda i, k: 9 + k)


def test_add_carry_and_wrap(lso):
    rng = np.random.default_rng(9)
    prof = [(M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, 3, 8), (M.ADD_SEGMENT_NUM, 12, 1), (M.ADD_SEGMENT_NUM, 13, 2),
                              (M.ADD_SEGMENT_NUM, 17, 4)])]
    fr = bytearray(rand_frame(rng, 30 + 9 * 16 + 1))
    fr[3:11] = bytes.fromhex("00fffffffffffffe")     # carries through seven bytes at k = 2
    fr[12] = 0xFD                                    # wraps at k = 3
    fr[13:15] = b"\xff\xfc"
    fr[17:21] = b"\xff\xff\xff\xfb"
    lay, buf, _ = check(lso, [(bytes(fr), 30, 16, 0, M.L3_INVALID)], prof, "carry", want_st=[0])
    o = int(lay.seg["off"][5])
    assert bytes(buf[o + 3:o + 11]) == bytes.fromhex("0100000000000003") and buf[o + 12] == 2
    assert bytes(buf[o + 13:o + 15]) == b"\x00\x01" and bytes(buf[o + 17:o + 21]) == b"\x00\x00\x00\x00"


def test_bits_and_add_on_one_byte(lso):
    """A later field sees what an earlier one wrote, in both orders."""
    rng = np.random.default_rng(10)
    bits = (M.WRITE_BITS, 16, 1, (0x0F, 0xF0, 0xFF), (0x05, 0xA0, 0xFE))
    add = (M.ADD_SEGMENT_NUM, 16, 1)
    prof = [(M.PROTO_CUSTOM, [bits, add]), (M.PROTO_CUSTOM, [add, bits]), (M.PROTO_CUSTOM, [add, bits, add, bits])]
    fr = bytearray(rand_frame(rng, 22 + 4 * 10))
    fr[16] = 0xFF
    lay, buf, _ = check(lso, [(bytes(fr), 22, 10, p, M.L3_INVALID) for p in range(3)], prof, "same byte",
                        want_st=[0, 0, 0])
    at = lambda i, k: int(buf[int(lay.seg["off"][int(lay.desc["first_seg"][i]) + k]) + 16])   # noqa: E731
    assert [at(0, 3), at(1, 3)] == [(0xFE + 3) & 0xFF, 0xFE]
    assert at(0, 0) == 0xF5 and at(1, 0) == 0xF5


def test_device_form_refuses_bad_descriptors(lso):
    """Descriptors mi_cls_lso_plan never makes: st tells, nothing is written."""
    from odp_amd.cls import lso_profiles
    rng = np.random.default_rng(11)
    items = [(rand_frame(rng, 22 + 100), 22, 40, P_BOTH, M.L3_INVALID) for _ in range(5)]
    lay = M.Layout(items, PROFILES)
    lay.desc["profile"][1] = 9            # no such profile
    lay.desc["seg_payload"][2] = 30       # 3 x 30 < 100: the last segment would be too long
    lay.desc["hdr_len"][3] = 129
    exp, _ = M.apply(lay.buf, lay.off[[0, 4]], lay.len[[0, 4]], lay.desc[[0, 4]], lay.seg, PROFILES)
    buf, st = lso.segment(lay.buf, lay.off, lay.len, lay.desc, lay.seg, lso_profiles(PROFILES))
    assert st.tolist() == [0, 3, 3, 3, 0]
    assert np.array_equal(buf, exp)


def test_parameter_errors(lso):
    from odp_amd.cls import lso_profiles
    rng = np.random.default_rng(12)
    lay = M.Layout([(rand_frame(rng, 22 + 100), 22, 40, 0, M.L3_INVALID)], [(M.PROTO_CUSTOM, [])])
    st = np.zeros(1, np.uint8)

    def host(prof, desc=lay.desc, seg=lay.seg, buf=None):
        b = lay.buf.copy() if buf is None else buf
        return lso.segment_host(b, lay.off, lay.len, desc, b, seg, lso_profiles(prof), st)

    assert host([(M.PROTO_CUSTOM, [])]) == 0
    for bad in ([(3, [])], [(M.PROTO_CUSTOM, [(2, 0, 2)])], [(M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, 0, 3)])],
                [(M.PROTO_CUSTOM, [(M.WRITE_BITS, 0, 2, (1, 1, 1), (1, 1, 1))])],
                [(M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, 129, 1)])], [(M.PROTO_CUSTOM, [])] * 17,
                [(M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, 0, 1)] * 9)]):
        assert host(bad) == -22, bad
    for field, value in (("profile", 1), ("nseg", 65), ("nseg", 1), ("hdr_len", 129), ("first_seg", 1),
                         ("seg_payload", 0)):
        d = lay.desc.copy()
        d[field][0] = value
        assert host([(M.PROTO_CUSTOM, [])], desc=d) == -22, field
    s = lay.seg.copy()
    s["off"][2] = lay.buf.nbytes - 10     # a segment past the destination
    assert host([(M.PROTO_CUSTOM, [])], seg=s) == -22
    s = lay.seg.copy()
    s["src"][1] = 1
    assert host([(M.PROTO_CUSTOM, [])], seg=s) == -22
    assert host([(M.PROTO_CUSTOM, [])], desc=lay.desc[:0], seg=lay.seg[:0]) == 0      # n == 0


@pytest.mark.parametrize("submit", [False, True])
def test_host_entries(lso, submit):
    """Pageable (staged) and page-locked (in place) host forms: both give the
    device entry's bytes, one failed packet's segments left alone."""
    from odp_amd.cls import PinnedArray, lso_profiles
    rng = np.random.default_rng(13)
    items = golden_items()
    items = [it for it in items if M.plan(len(it[0]), it[1], it[2], PROFILES[it[3]][0], it[4])[0] > 1]
    items.insert(3, (ip_frame(rng, 34 + 100, ver_ihl=0x46), 34, 40, P_IPV4, 14))
    items += [(rand_frame(rng, 9000), 64, 1448, P_BOTH, M.L3_INVALID)]
    lay, dev_buf, dev_st = check(lso, items, what="device", src_res=lambda i: i, dst_res=lambda i, k: i + k)
    assert dev_st[3] == M.ST_IHL
    prof = lso_profiles(PROFILES)
    n, ns = len(lay.desc), len(lay.seg)
    # pageable, one buffer
    buf, st = lay.buf.copy(), np.full(n, 0xEE, np.uint8)
    assert lso.segment_host(buf, lay.off, lay.len, lay.desc, buf, lay.seg, prof, st, submit=submit) == 0
    assert np.array_equal(buf, dev_buf) and np.array_equal(st, dev_st)
    # pageable, the destination another buffer (the same offsets)
    src, dst = lay.buf.copy(), np.full(lay.buf.nbytes, M.Layout.GUARD, np.uint8)
    st[:] = 0xEE
    assert lso.segment_host(src, lay.off, lay.len, lay.desc, dst, lay.seg, prof, st, submit=submit) == 0
    exp = dev_buf.copy()
    for o, ln in zip(lay.off, lay.len):
        exp[int(o):int(o) + int(ln)] = M.Layout.GUARD
    assert np.array_equal(dst, exp) and np.array_equal(src, lay.buf) and np.array_equal(st, dev_st)
    # page-locked
    pins = [PinnedArray(lay.buf.nbytes), PinnedArray(4 * n), PinnedArray(2 * n), PinnedArray(16 * n),
            PinnedArray(8 * ns), PinnedArray(n)]
    try:
        pbuf, poff, plen = pins[0].u8, pins[1].view(np.uint32, n), pins[2].view(np.uint16, n)
        pdesc, pseg, pst = pins[3].view(M.DESC_DTYPE, n), pins[4].view(M.SEG_DTYPE, ns), pins[5].u8
        pbuf[:], poff[:], plen[:], pdesc[:], pseg[:], pst[:] = lay.buf, lay.off, lay.len, lay.desc, lay.seg, 0xEE
        assert lso.segment_host(pbuf, poff, plen, pdesc, pbuf, pseg, prof, pst, submit=submit) == 0
        assert np.array_equal(pbuf, dev_buf) and np.array_equal(pst[:n], dev_st)
    finally:
        for p in pins:
            p.close()


# ------------------------------------------------- odp_pktout_send_lso round trip
def run_flow(tmp_path, lines, env=None):
    """Run a tests/rt/lso_driver.c flow script; its output lines as (tag, fields)."""
    script = tmp_path / "flow.txt"
    script.write_text("\n".join(lines) + "\n")
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([LSO_DRIVER, "flow", str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120, env=e)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [(ln.split()[0], ln.split()[1:]) for ln in r.stdout.splitlines()]


def prof_line(profile):
    proto, fields = profile
    if proto == M.PROTO_IPV4:
        return "prof ipv4 0"
    out = [f"prof custom {len(fields)}"]
    for f in fields:
        m, v = (f[3], f[4]) if len(f) > 3 else ((0, 0, 0), (0, 0, 0))
        out.append(f"{f[0]} {f[1]} {f[2]} {m[0]} {m[1]} {m[2]} {v[0]} {v[1]} {v[2]}")
    return " ".join(out)


def l3_arg(l3):
    return -1 if l3 == M.L3_INVALID else l3


def flow_head(num=4096, length=1856, pktout=0, pktin=0):
    return [f"pool {num} {length}", f"cfg {pktout:x} {pktin:x}"] + [prof_line(p) for p in PROFILES]


def expect_segments(items):
    out = []
    for fr, hdr, mp, p, l3 in items:
        st, segs = M.segments(fr, hdr, mp, PROFILES[p], l3)
        assert st == 0
        out.append(segs)
    return out


def received(ev):
    return [(int(f[0]), int(f[1]), int(f[2]), int(f[3]), bytes.fromhex(f[4])) for t, f in ev if t == "P"]


@pytest.mark.parametrize("use_opt", [False, True], ids=["pkt_meta", "opt"])
def test_runtime_suite_flow(built, gpu, tmp_path, use_opt):
    """The reference suite's flow (lso.c:755-848) on a loop pktio: every golden
    case sent with per-packet metadata (one call, one launch) or with an opt
    argument (a call each); the segments arrive in order with the model's
    bytes, IPv4 ones with their L3 offset, none carrying a request; the
    originals of segmented packets are freed (the pool is whole again)."""
    items = golden_items()
    lines = flow_head() + ["free"]
    for fr, hdr, mp, p, l3 in items:
        if use_opt:
            lines += [f"pkt {fr.hex()} {l3_arg(l3)}", f"send {p} {hdr} {mp}"]
        else:
            lines.append(f"pkt {fr.hex()} {l3_arg(l3)} {p} {hdr} {mp}")
    if not use_opt:
        lines.append("send none")
    lines += ["recv", "free", "stats"]
    ev = run_flow(tmp_path, lines)
    assert [f for t, f in ev if t == "H"] == [["1"]] * len(PROFILES)
    assert [int(f[0]) for t, f in ev if t == "R"] == ([1] * len(items) if use_opt else [len(items)])
    exp = expect_segments(items)
    got = received(ev)
    assert [g[4] for g in got] == [s for segs in exp for s in segs]
    assert all(g[1] == 0 and g[3] == 0 for g in got)
    pos = 0
    for (fr, hdr, mp, p, l3), segs in zip(items, exp):
        if p == P_IPV4:
            assert all(g[0] == 14 for g in got[pos:pos + len(segs)])
        pos += len(segs)
    free = [int(f[0]) for t, f in ev if t == "F"]
    assert free[0] == free[1] == 4096
    nseg = sum(1 for segs in exp if len(segs) > 1)
    assert [f for t, f in ev if t == "T"] == [[str(nseg if use_opt else 1), "0", "0"]]


def test_runtime_whole_packets_make_no_launch(built, gpu, tmp_path):
    items = [it for it in golden_items() if M.plan(len(it[0]), it[1], it[2], PROFILES[it[3]][0], it[4])[0] == 1]
    lines = flow_head() + [f"pkt {fr.hex()} {l3_arg(l3)} {p} {hdr} {mp}" for fr, hdr, mp, p, l3 in items]
    ev = run_flow(tmp_path, lines + ["send none", "recv", "free", "stats"])
    assert [f for t, f in ev if t == "R"] == [[str(len(items))]]
    assert [g[4] for g in received(ev)] == [it[0] for it in items]
    assert [f for t, f in ev if t == "T"] == [["0", "0", "0"]] and [f for t, f in ev if t == "F"] == [["4096"]]


def test_runtime_pool_too_small(built, gpu, tmp_path):
    """Three packets of five segments each from a pool of 12: the second
    packet's segments cannot all be taken -- 1 is returned, only the first
    packet's segments arrive, and nothing leaks."""
    rng = np.random.default_rng(21)
    items = [(rand_frame(rng, 22 + 4 * 100 + 30), 22, 100, P_BOTH, M.L3_INVALID) for _ in range(3)]
    lines = flow_head(num=12) + [f"pkt {fr.hex()} -1 {p} {hdr} {mp}" for fr, hdr, mp, p, l3 in items]
    ev = run_flow(tmp_path, lines + ["send none", "recv", "free", "stats"])
    assert [f for t, f in ev if t == "R"] == [["1"]]
    assert [g[4] for g in received(ev)] == expect_segments(items[:1])[0]
    assert [f for t, f in ev if t == "F"] == [["12"]] and [f for t, f in ev if t == "T"] == [["1", "0", "0"]]


def test_runtime_list_ends_at_unrequested_and_failed_packets(built, gpu, tmp_path):
    """opt == NULL with a packet without a request in the middle; an IPv4
    packet with IP options (the kernel's st) in the middle; a plan error
    (payload offset inside the IP header) in the middle."""
    rng = np.random.default_rng(22)
    ok = lambda: (ip_frame(rng, 34 + 3 * 64 + 9), 34, 64, P_IPV4, 14)   # noqa: E731
    a, b, c = ok(), ok(), ok()
    req = lambda it: f"pkt {it[0].hex()} {l3_arg(it[4])} {it[3]} {it[1]} {it[2]}"   # noqa: E731
    opt6 = (ip_frame(rng, 34 + 3 * 64 + 9, ver_ihl=0x46), 34, 64, P_IPV4, 14)
    lines = flow_head() + [req(a), f"pkt {b[0].hex()} 14", req(c), "send none", "recv", "free",
                           req(a), req(opt6), req(c), "send none", "recv", "free",
                           req(a), f"pkt {b[0].hex()} 14 {P_IPV4} 30 64", req(c), "send none", "recv", "free",
                           f"pkt {b[0].hex()} 14", req(a), "send none", "recv", "free"]
    ev = run_flow(tmp_path, lines)
    assert [f for t, f in ev if t == "R"] == [["1"], ["1"], ["1"], ["-1"]]
    assert [g[4] for g in received(ev)] == expect_segments([a])[0] * 3
    assert [f for t, f in ev if t == "F"] == [["4096"]] * 4


@pytest.mark.parametrize("env", [None, {"ODP_AMD_PAGEABLE_POOLS": "pktio_pool"}], ids=["pinned_pool", "pageable_pool"])
def test_runtime_segments_pass_checksum_validation(built, gpu, tmp_path, env):
    """pktout.ipv4_chksum and the pktin IPv4 checksum validation configured:
    the segments' header checksums, written by the LSO kernel and again by
    the checksum insertion of the send, verify on receive.  The pageable pool
    takes both through their bounce buffers, with the same bytes."""
    items = [it for it in golden_items() if it[3] == P_IPV4]
    lines = flow_head(pktout=0x20, pktin=0x4) + [f"pkt {fr.hex()} {l3_arg(l3)} {p} {hdr} {mp}"
                                                for fr, hdr, mp, p, l3 in items]
    ev = run_flow(tmp_path, lines + ["send none", "recv", "free", "stats"], env=env)
    assert [f for t, f in ev if t == "R"] == [[str(len(items))]]
    got = received(ev)
    assert [g[4] for g in got] == [s for segs in expect_segments(items) for s in segs]
    assert all(g[1] == 0 and g[2] == 2 for g in got)       # no error, L3 checksum OK
    assert [f for t, f in ev if t == "F"] == [["4096"]]
    assert [f for t, f in ev if t == "T"] == [["1", "1" if env else "0", "1"]]


def test_runtime_two_senders_on_one_pktio(built, gpu):
    """Two threads in odp_pktout_send_lso on one pktio at once, each call with
    a packet the kernel refuses between two good ones: the pktio's descriptor
    and status arrays are shared, so a call must take its verdicts while it
    holds them.  Every call returns 1, and only whole, correct segments of the
    good first packets (four each) reach the queue."""
    iters = 150
    r = subprocess.run([LSO_DRIVER, "mt", str(iters)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    mt = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("MT ")]
    assert mt == [["0", str(2 * iters * 4), "0"]]


def test_runtime_send_lso_on_a_pcap_pktio(built, gpu, tmp_path):
    """LSO is common code over every driver (the capability is advertised for
    pcap too): the golden cases sent on a pcap pktio land in its dump file as
    the model's segments, in order, and nothing leaks."""
    items = golden_items()
    dump = tmp_path / "lso_out.pcap"
    lines = flow_head()
    lines[1] = f"cfg 0 0 pcap:out={dump}"
    lines += [f"pkt {fr.hex()} {l3_arg(l3)} {p} {hdr} {mp}" for fr, hdr, mp, p, l3 in items]
    ev = run_flow(tmp_path, lines + ["send none", "free", "stats"])
    assert [f for t, f in ev if t == "R"] == [[str(len(items))]]
    data = dump.read_bytes()
    frames, o = [], 24
    while o < len(data):
        n = struct.unpack_from("<I", data, o + 8)[0]
        frames.append(data[o + 16:o + 16 + n])
        o += 16 + n
    assert frames == [s for segs in expect_segments(items) for s in segs]
    assert [f for t, f in ev if t == "F"] == [["4096"]] and [f for t, f in ev if t == "T"] == [["1", "0", "0"]]
