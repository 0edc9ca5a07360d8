"""mi_cls_parse / odp_packet_parse on the GPU against the CPU model
(tests/parse_model.py): every record bit for bit, `outcome` included.

Frames: the zoo and chksum_frames.frame_set(seed=7, n=400) (valid and
single-bit-corrupted checksums), each behind one of the reference's L2
offsets (packet.c:3722), cycled per packet, so parse starts are unaligned.
IP starts begin at each frame's own L3 offset (from an ETH parse of the
model); every frame is parsed "as IPv4" and "as IPv6" whatever it holds, which
exercises the version / IHL errors.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import chksum_frames as CK
from tests import parse_model as PM
from tests import rt_helpers as H
from tests import zoo
from tests.helpers import assert_same, gpu_run
from tests.parse_model import FLAG_BITS, result_word, types_of

pytestmark = pytest.mark.gpu

SELECTIONS = (0, 1, 2, 4, 8, 0xF)
PARSE_DRIVER = os.path.join(H.ROOT, "tests", "_bin", "parse_driver")


@pytest.fixture(scope="module")
def ctx(built, gpu):
    from odp_amd.cls import ParseContext
    c = ParseContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus(built):
    """[(frame behind its offset filler, ETH parse offset, L3 offset)]: the
    zoo and the checksum frames, offsets cycled per packet."""
    frames = [f for _, f in zoo.all_frames()] + [f for f, _, _ in CK.frame_set(seed=7, n=400)]
    out = []
    for i, f in enumerate(f for f in frames if len(f) > 0):
        o = PM.REF_OFFSETS[i % len(PM.REF_OFFSETS)]
        l3 = PM.parse(f, 0, PM.PROTO_ETH, PM.ALL, 0)[4]
        out.append((PM.shifted(f, o), o, o + l3))
    return out


def _starts(corpus, proto):
    """Frames and parse offsets for a start protocol (IP starts: the frames
    whose L3 offset lies inside them)."""
    if proto == PM.PROTO_ETH:
        return [f for f, _, _ in corpus], [o for _, o, _ in corpus]
    keep = [(f, l3) for f, _, l3 in corpus if l3 < len(f)]
    return [f for f, _ in keep], [l3 for _, l3 in keep]


@pytest.mark.parametrize("layer", [PM.L2, PM.L3, PM.L4, PM.ALL])
@pytest.mark.parametrize("proto", [PM.PROTO_ETH, PM.PROTO_IPV4, PM.PROTO_IPV6])
def test_matrix(ctx, corpus, proto, layer):
    """start x layer, under every checksum selection."""
    frames, offs = _starts(corpus, proto)
    assert len(frames) > 700
    batch = PM.batch_at(frames, offs)
    for sel in SELECTIONS:
        got = ctx.parse(batch, proto, layer, sel)
        exp = PM.records(frames, offs, proto, layer, sel)
        assert_same(got, exp, batch, f"proto {proto} layer {layer} chksums {sel:#x}")
        info = ctx.last_launch()
        eff = 0 if layer == PM.L2 else (sel & 1 if layer == PM.L3 else sel)
        assert info[0] == 4 and info[3] == 0 and info[5] == (1 if eff else 0), info


def _geometry_frames():
    rng = np.random.default_rng(11)
    F = []
    # a tile of frames all <= 64 B, then one mixing 60 B with 65-96 B and > 96 B
    F += [pg.udp4_frame(size=60 + (i & 3), sport=1000 + i) for i in range(64)]
    for i in range(64):
        size = (60, 65 + (i % 32), 97 + 11 * (i % 40))[i % 3]
        F.append(pg.tcp4_frame(size=size, sport=2000 + i) if i & 1 else pg.udp4_frame(size=size))
    # QinQ + IPv6 HBH / routing chain + TCP: L4 fields come from past the window
    ch = pg.ipv6_ext(43, 0) + pg.ipv6_ext(43, 2) + pg.ipv6_ext(pg.IPPROTO_TCP, 0)
    for hl in (5, 4):
        F.append(pg.pad_to(pg.eth(ethtype=pg.ETH_IPV6, tags=(0x123, 0x456)) +
                           pg.ipv6(next_hdr=0, payload_len=len(ch) + 20) + ch + pg.tcp(7, 8, hl=hl), 160))
    # one byte short of the L4 header: outcome drop with err 0 at L4, ENQ at L3
    E = pg.eth()
    # (the IP lengths say so too: no IP error)
    def v4(**kw):   # with a valid header checksum
        h = bytearray(pg.ipv4(**kw))
        h[10:12] = b"\0\0"
        h[10:12] = CK.inet_csum(bytes(h)).to_bytes(2, "big")
        return bytes(h)
    F += [E + v4(tot_len=20 + 7) + pg.udp()[:7],
          E + v4(proto=6, tot_len=20 + 19) + pg.tcp()[:19],
          E + v4(proto=132, tot_len=20 + 11) + pg.sctp()[:11],
          pg.eth(ethtype=pg.ETH_IPV6) + pg.ipv6(next_hdr=6, payload_len=19) + pg.tcp()[:19]]
    # SCTP of 65, 128 and 129 bytes from L4; one past the cooperative CRC's reach
    for n in (65, 128, 129, 16400):
        F.append(CK.build(rng, 4, pg.IPPROTO_SCTP, payload=bytes(rng.integers(0, 256, n - 12).astype(np.uint8)))[0])
        F.append(CK.corrupt(rng, F[-1], 14 + 20 + 12, len(F[-1])))
    return F


@pytest.fixture(scope="module")
def geometry():
    frames = _geometry_frames()
    offs = [PM.REF_OFFSETS[i % len(PM.REF_OFFSETS)] for i in range(len(frames))]
    frames = [PM.shifted(f, o) for f, o in zip(frames, offs)]
    # len - offset of 1, 13 and 14
    for rest in (1, 13, 14):
        f = pg.udp4_frame(size=60)
        frames.append(f)
        offs.append(len(f) - rest)
    return frames, offs


@pytest.mark.parametrize("layer,sel", [(PM.ALL, 0), (PM.ALL, 0xF), (PM.L4, 8), (PM.L3, 0xF), (PM.L2, 0xF)])
def test_geometry(ctx, geometry, layer, sel):
    frames, offs = geometry
    batch = PM.batch_at(frames, offs)
    got = ctx.parse(batch, PM.PROTO_ETH, layer, sel)
    exp = PM.records(frames, offs, PM.PROTO_ETH, layer, sel)
    assert_same(got, exp, batch, f"geometry layer {layer} chksums {sel:#x}")
    # the frames cut one byte short of their L4 header (after the two tiles
    # and the two chain frames)
    cut = got[130:134]
    if layer >= PM.L4:
        assert (cut["outcome"] == R.OUT_PARSE_DROP).all() and (cut["err"] == 0).all()
    elif layer == PM.L3:
        assert (cut["outcome"] == R.OUT_ENQ).all()
    if layer == PM.ALL and sel == 0xF:
        big = got[134 + 6:134 + 8]   # the 16400-byte SCTP frame, valid and corrupted
        assert big["err"][0] == 0 and big["err"][1] == CK.E_SCTP | CK.E_L4CK
        assert (big["in_flags"] & CK.L4_DONE).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(ctx, corpus, n):
    """A tile edge and a 4-wave-block edge."""
    frames, offs = _starts(corpus, PM.PROTO_ETH)
    frames, offs = frames[40:40 + n], offs[40:40 + n]
    batch = PM.batch_at(frames, offs)
    for sel in (0, 0xF):
        got = ctx.parse(batch, PM.PROTO_ETH, PM.ALL, sel)
        assert_same(got, PM.records(frames, offs, PM.PROTO_ETH, PM.ALL, sel), batch, f"n {n}")


def test_parameters(ctx):
    """n == 0 and the parameter checks of the device entry."""
    from odp_amd.cls import ParseParam
    import ctypes as C
    L = ctx.L
    assert ctx.parse_device(0, 0, 0, 0, PM.PROTO_ETH, PM.ALL, 0, 0) == 0
    for proto, layer in ((0, 4), (4, 4), (1, 0), (1, 5)):
        assert ctx.parse_device(0, 0, 0, 0, proto, layer, 0, 0) == -22
        pp = ParseParam(proto, layer, 0)
        assert L.mi_cls_parse_host(ctx.ctx, None, 0, None, None, 0, C.byref(pp), None) == -22


def _host_arrays(batch, pinned):
    from odp_amd.cls import PinnedArray
    n = batch.n
    if not pinned:
        return (np.ascontiguousarray(batch.buf), batch.off.astype(np.uint32), batch.len.astype(np.uint16),
                np.zeros(n, R.RESULT_DTYPE), [])
    keep = [PinnedArray(batch.buf.nbytes), PinnedArray(4 * n), PinnedArray(2 * n), PinnedArray(16 * n)]
    buf, off, ln = keep[0].view(np.uint8), keep[1].view(np.uint32, n), keep[2].view(np.uint16, n)
    out = keep[3].view(R.RESULT_DTYPE, n)
    buf[:] = batch.buf
    off[:] = batch.off
    ln[:] = batch.len
    return buf, off, ln, out, keep


@pytest.mark.parametrize("pinned", [False, True])
def test_host_batches(ctx, corpus, pinned):
    """ParseContext over pageable (staged) and page-locked (in place) batches."""
    frames, offs = _starts(corpus, PM.PROTO_ETH)
    frames, offs = frames[:300], offs[:300]
    buf, off, ln, out, keep = _host_arrays(PM.batch_at(frames, offs), pinned)
    try:
        for layer, sel in ((PM.ALL, 0xF), (PM.L3, 1)):
            out[:] = np.zeros((), R.RESULT_DTYPE)
            ctx.parse_host(buf, off, ln, out, PM.PROTO_ETH, layer, sel)
            assert_same(np.array(out), PM.records(frames, offs, PM.PROTO_ETH, layer, sel), None,
                        f"host pinned={pinned}")
    finally:
        for k in keep:
            k.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_submit_wait_two_in_flight(ctx, corpus, pinned):
    frames, offs = _starts(corpus, PM.PROTO_ETH)
    a = _host_arrays(PM.batch_at(frames[:200], offs[:200]), pinned)
    b = _host_arrays(PM.batch_at(frames[200:330], offs[200:330]), pinned)
    try:
        ta = ctx.submit_host(*a[:4], PM.PROTO_ETH, PM.ALL, 0xF)
        tb = ctx.submit_host(*b[:4], PM.PROTO_ETH, PM.L4, 0)
        assert tb == ta + 1
        ctx.wait(tb)
        ctx.wait(ta)
        assert_same(np.array(a[3]), PM.records(frames[:200], offs[:200], PM.PROTO_ETH, PM.ALL, 0xF))
        assert_same(np.array(b[3]), PM.records(frames[200:330], offs[200:330], PM.PROTO_ETH, PM.L4, 0))
    finally:
        for k in a[4] + b[4]:
            k.close()


@pytest.mark.parametrize("sel", [0, 0xF])
def test_equals_classify_kernel(ctx, corpus, sel):
    """ETH, offset 0, ALL: the parse fields of the classification kernel under
    a default-CoS-only program with the selection as pktin option, for the
    records that kernel does not drop."""
    frames = [f[o:] for f, o, _ in corpus]
    batch = pg.batch_from_frames(frames)
    cls = gpu_run([R.cos("d", queue=1), ("default", 0)], batch, pktin_opt=sel << 2)
    got = ctx.parse(batch, PM.PROTO_ETH, PM.ALL, sel)
    keep = cls["outcome"] != R.OUT_PARSE_DROP
    assert keep.sum() > 700
    for field in ("in_flags", "err", "l3_offset", "l4_offset"):
        assert np.array_equal(got[field][keep], cls[field][keep]), field


# ------------------------------------------------------------------ runtime
# what each reference case sets (packet.c:3745-4541): parse_eth_ipv4_udp and
# parse_eth_snap_ipv4_udp ALL with all checksums, parse_eth_ipv6_tcp ALL with
# none, every other Ethernet case L4 with none; parse_ipv4_udp (:3827) starts
# from IPv4 at + 14, L4, none
REF_PARAMS = {"test_packet_ipv4_udp": (PM.ALL, 0xF), "test_packet_snap_ipv4_udp": (PM.ALL, 0xF),
              "test_packet_ipv6_tcp": (PM.ALL, 0)}


def _cases():
    """The reference's odp_packet_parse() suite with each case's own
    parameters, then every golden frame under ETH / ALL / all checksums and
    the plain IPv4 / IPv6 frames from their IP headers.
    [(case, fixture frame, proto, layer, chksums, plus, frame)]"""
    with open(os.path.join(H.ROOT, "tests", "golden", "parse_frames.json")) as f:
        d = json.load(f)["frames"]
    cases = []
    for name, v in sorted(d.items()):
        layer, sel = REF_PARAMS.get(name, (PM.L4, 0))
        cases.append((name, name, PM.PROTO_ETH, layer, sel, 0, bytes.fromhex(v["frame"])))
    v4, v6 = (bytes.fromhex(d[k]["frame"]) for k in ("test_packet_ipv4_udp", "test_packet_ipv6_udp"))
    cases.append(("parse_ipv4_udp", None, PM.PROTO_IPV4, PM.L4, 0, 14, v4))
    for name, v in sorted(d.items()):
        cases.append((name + ".all", name, PM.PROTO_ETH, PM.ALL, 0xF, 0, bytes.fromhex(v["frame"])))
    cases.append(("parse_ipv4_udp.all", None, PM.PROTO_IPV4, PM.ALL, 0xF, 14, v4))
    cases.append(("parse_ipv6_udp.all", None, PM.PROTO_IPV6, PM.L4, 0xF, 14, v6))
    return d, cases


def _run_driver(tmp_path, env_extra=None):
    d, cases = _cases()
    script = tmp_path / "cases.txt"
    bad = pg.pad_to(pg.eth() + pg.ipv4(ver=5, payload_len=8) + pg.udp(), 60)
    with open(script, "w") as f:
        for name, _, proto, layer, sel, plus, frame in cases:
            f.write(f"C {name} {proto} {layer} {sel} {plus} {frame.hex()}\n")
        f.write(f"M {cases[0][6].hex()} {bad.hex()}\n")
    env = dict(os.environ)
    env.update(env_extra or {})
    r = subprocess.run([PARSE_DRIVER, "run", str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return d, cases, [ln.split() for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def driver(built, gpu, tmp_path_factory):
    return _run_driver(tmp_path_factory.mktemp("parse"))


def _check_cases(d, cases, lines):
    rets = {p[1]: (int(p[2]), int(p[3])) for p in lines if p[0] == "R"}
    pk = {}
    for p in lines:
        if p[0] == "P":
            pk.setdefault(p[1], []).append(p[2:])
    for name, fixture, proto, layer, sel, plus, frame in cases:
        assert rets[name] == (0, 9), (name, rets[name])
        assert len(pk[name]) == 10
        for i, p in enumerate(pk[name]):
            o = PM.REF_OFFSETS[i]
            idx, flags, err, l2, l3, l4, t2, t3, t4, s3, s4, word, len_, pre3, pre4 = (int(x, 0) for x in p)
            ret, efl, eerr, el2, el3, el4 = PM.parse(PM.shifted(frame, o), o + plus, proto, layer, sel)
            assert ret == 0 and idx == i
            assert (flags, err, l2, l3, l4) == (efl, eerr, el2, el3, el4), (name, i)
            assert (pre3, pre4) == (0, 0)          # UNKNOWN before the parse (packet.c:3756-3761)
            assert s3 == (0 if not efl >> 30 & 1 else 1 if eerr & 0x04 else 2), (name, i)
            assert s4 == (0 if not efl >> 31 & 1 else 1 if eerr & 0x40 else 2), (name, i)
            assert (t2, t3, t4) == types_of(efl), (name, i)
            assert word == result_word(efl, eerr) and len_ == len(frame) + o
            if fixture:
                for flag, want in d[fixture]["expect"].items():
                    assert (flags >> FLAG_BITS[flag]) & 1 == want, (name, i, flag)
    # the golden frames carry valid checksums: OK after the parse (packet.c:3756-3761 ff.)
    assert all(int(p[9], 0) == 2 and int(p[10], 0) == 2 for p in pk["test_packet_ipv4_udp"])
    assert all(int(p[10], 0) == 2 for p in pk["test_packet_ipv4_sctp.all"])
    assert all(int(p[9], 0) == 0 and int(p[10], 0) == 2 for p in pk["test_packet_ipv6_tcp.all"])
    assert all(int(p[9], 0) == 0 and int(p[10], 0) == 0 for p in pk["test_packet_ipv6_tcp"])   # none asked


def test_runtime_reference_suite(driver):
    _check_cases(*driver)


def test_runtime_multi_stops_at_failure(driver):
    """A failing packet at index 3 of 8: the call returns 3, the packet
    carries its record's metadata, packets 4-7 keep the sentinel offsets."""
    _, cases, lines = driver
    assert ["M", "3"] in lines
    mp = [[int(x, 0) for x in p[1:]] for p in lines if p[0] == "MP"]
    assert len(mp) == 8
    good = PM.parse(cases[0][6], 0, PM.PROTO_ETH, PM.ALL, 0xF)
    bad = PM.parse(pg.pad_to(pg.eth() + pg.ipv4(ver=5, payload_len=8) + pg.udp(), 60), 0, PM.PROTO_ETH,
                   PM.ALL, 0xF)
    assert bad[0] == -1 and bad[2] != 0
    for i, (idx, flags, err, l2, l3, l4) in enumerate(mp):
        if i < 3:
            assert (flags, err, l2, l3, l4) == good[1:], i
        elif i == 3:
            assert (flags, err, l2, l3, l4) == bad[1:], i
        else:
            assert (flags, err, l2, l3, l4) == (0, 0, 0, 5, 7), i   # as allocated, the sentinels


def test_runtime_keeps_user_ptr_and_override(driver):
    assert ["U", "1", "0xc"] in driver[2]   # user pointer kept; l4_chksum_set | l4_chksum


def test_runtime_none_and_offset(driver):
    assert ["N", "-1", "-1", "-1", "0", "0", "0"] in driver[2]


def test_runtime_two_threads(driver):
    _, cases, lines = driver
    frame = cases[0][6]
    th = [[int(x, 0) for x in p[1:]] for p in lines if p[0] == "T"]
    assert len(th) == 2 * 10
    for t, i, ret, flags, err, l2, l3, l4 in th:
        o = PM.REF_OFFSETS[i]
        assert (0, flags, err, l2, l3, l4) == PM.parse(PM.shifted(frame, o), o, PM.PROTO_ETH, PM.ALL, 0xF)
        assert ret == 0


def test_runtime_pageable_pool(driver, tmp_path):
    """Packets of a pageable pool take the bounce buffer: same output."""
    _, _, lines = driver
    _, _, paged = _run_driver(tmp_path, {"ODP_AMD_PAGEABLE_POOLS": "parse_pool"})
    strip = lambda L: [p for p in L if p[0] != "B"]  # noqa: E731
    assert strip(paged) == strip(lines)
    assert ["B", "0"] in lines and ["B", "1"] in paged   # in place / bounced


# ---- whole calls of any size over one or two pools (parse_driver batch): the
# gather of odp_packet_parse_multi -- arrays that grow, a call that mixes a
# page-locked and a pageable pool
def _run_batch(tmp_path, calls, env_extra=None):
    """calls: [(packets, pools)].  Returns the golden frames and, per call,
    ((return, calls counted, bounced), [(flags, err, l2, l3, l4)])."""
    d, _ = _cases()
    frames = [bytes.fromhex(v["frame"]) for _, v in sorted(d.items())]
    script = tmp_path / "batch.txt"
    with open(script, "w") as f:
        for fr in frames:
            f.write(f"F {fr.hex()}\n")
        for n, pools in calls:
            f.write(f"B {n} {pools}\n")
    env = dict(os.environ)
    env.update(env_extra or {})
    r = subprocess.run([PARSE_DRIVER, "batch", str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = []
    for p in (ln.split() for ln in r.stdout.splitlines()):
        if p[0] == "Q":
            out.append((tuple(int(x) for x in p[1:]), []))
        elif p[0] == "QP":
            assert int(p[1]) == len(out[-1][1])
            out[-1][1].append(tuple(int(x, 0) for x in p[2:]))
    assert [len(pk) for _, pk in out] == [n for n, _ in calls]
    return frames, out


def _batch_model(frames, n):
    memo = {}
    for i in range(n):
        key = (i % len(frames), i % len(PM.REF_OFFSETS))
        if key not in memo:
            o = PM.REF_OFFSETS[key[1]]
            ret, *meta = PM.parse(PM.shifted(frames[key[0]], o), o, PM.PROTO_ETH, PM.ALL, 0xF)
            assert ret == 0
            memo[key] = tuple(meta)
    return [memo[(i % len(frames), i % len(PM.REF_OFFSETS))] for i in range(n)]


def test_runtime_burst_mixing_pools(built, gpu, tmp_path):
    """One call over 16 packets that alternate between a page-locked and a
    pageable pool: the output of the same frames from one page-locked pool;
    one call counted, and it bounced."""
    frames, one = _run_batch(tmp_path, [(16, 1)])
    _, mixed = _run_batch(tmp_path, [(16, 2)], {"ODP_AMD_PAGEABLE_POOLS": "parse_pool2"})
    assert one[0][0] == (16, 1, 0) and mixed[0][0] == (16, 1, 1)
    assert mixed[0][1] == one[0][1] == _batch_model(frames, 16)


@pytest.mark.parametrize("pageable", [False, True])
def test_runtime_arrays_grow(built, gpu, tmp_path, pageable):
    """8 packets, then 1025 (past the 1024-entry minimum of the arrays; the
    pageable pool's bounce buffer grows too) in one process."""
    frames, out = _run_batch(tmp_path, [(8, 1), (1025, 1)],
                             {"ODP_AMD_PAGEABLE_POOLS": "parse_pool"} if pageable else None)
    for (stat, pk), n in zip(out, (8, 1025)):
        assert stat == (n, 1, int(pageable))
        assert pk == _batch_model(frames, n)
