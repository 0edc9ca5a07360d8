"""pktout checksum insertion on the GPU (mi_cls_chksum_insert, its host
entries and the loop pktio's send path) vs the model of the rules
(tests/tx_model.py): the whole buffer byte for byte -- so a stray store
shows -- and the done bytes, over the protocol / configuration matrix, the
kernel's geometry (batch sizes, piece boundaries, long frames, unaligned
offsets, odd L3 offsets, tags, IP options), the decision edges, IMIX traffic
checked again by the receive validation, and a loop pktio round trip."""
import os
import struct
import subprocess

import numpy as np
import pytest

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import chksum_frames as CK
from tests import tx_model as TX
from tests.helpers import gpu_run
from tests.rt_helpers import write_pcap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_DRIVER = os.path.join(ROOT, "tests", "_bin", "tx_driver")
ALL_OVR = TX.L3_SET | TX.L3_CK | TX.L4_SET | TX.L4_CK


@pytest.fixture(scope="module")
def tx(built, gpu):
    from odp_amd.cls import TxContext
    c = TxContext(0)
    yield c
    c.close()


def check(tx, batch, desc, opt, what=""):
    """GPU == model over the whole buffer, and the done bytes."""
    exp_buf, exp_done = TX.apply(batch.buf, batch.off, batch.len, desc, opt)
    buf, done = tx.insert(batch, desc, opt)
    bad = np.nonzero(buf != exp_buf)[0]
    if bad.size:
        o = int(bad[0])
        i = int(np.searchsorted(batch.off, o, side="right")) - 1
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {o} = frame {i} + "
                             f"{o - int(batch.off[i])} (len {int(batch.len[i])}, desc {desc[i]}): "
                             f"gpu {buf[o]:#x} model {exp_buf[o]:#x}")
    assert np.array_equal(done, exp_done), (what, np.nonzero(done != exp_done)[0][:8])
    return buf, done


def framed(items, flags=0):
    """Batch + descriptors of [(frame, l3, l4)]."""
    b = pg.batch_from_frames([f for f, _, _ in items])
    return b, TX.make_desc([l3 for _, l3, _ in items], [l4 for _, _, l4 in items], flags)


_matrix = {}


def matrix_items():
    """The frame_set frames (valid and corrupted ones), checksum fields scrambled."""
    if "items" not in _matrix:
        out = []
        for fr, _, _ in CK.frame_set(seed=7, n=400):
            l3, l4 = TX.offsets_of(fr)
            out.append((TX.scramble(fr, l3, l4), l3, l4))
        _matrix["items"] = out
    return _matrix["items"]


MATRIX = {
    "all_defaults": (TX.ALL_TX, 0),
    "ipv4_only": (TX.CK_IPV4, 0),
    "udp_only": (TX.CK_UDP, 0),
    "tcp_only": (TX.CK_TCP, 0),
    "sctp_only": (TX.CK_SCTP, 0),
    "defaults_off_ovr_on": (TX.ALL_ENA, ALL_OVR),
    "defaults_on_ovr_off": (TX.ALL_TX | TX.ALL_ENA, TX.L3_SET | TX.L4_SET),
    "mixed_overrides": (TX.CK_UDP | TX.CK_IPV4, None),
}


@pytest.mark.parametrize("name", sorted(MATRIX))
def test_protocol_matrix(tx, name):
    """The reference's _ovr / _no_ovr / _pktio cases for IPv4, UDP and SCTP
    (pktio.c:4719-5014), plus TCP, each single default, and per-packet
    override mixes inside one tile."""
    opt, flags = MATRIX[name]
    items = matrix_items()
    if flags is None:
        flags = np.random.default_rng(3).integers(0, 16, len(items)).astype(np.uint8)
    b, desc = framed(items, flags)
    _, done = check(tx, b, desc, opt, name)
    if name == "all_defaults":
        assert (done != 0).all()
        for bit in (TX.DONE_IPV4, TX.DONE_UDP, TX.DONE_TCP, TX.DONE_SCTP):
            assert (done & bit).any()
    if name == "defaults_on_ovr_off":
        assert not done.any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(tx, n):
    b, desc = framed(matrix_items()[:n])
    check(tx, b, desc, TX.ALL_TX, f"n={n}")


def boundary_items():
    """Every protocol / IP version at frame lengths around the 64-B piece
    boundaries (the L4 range ends at 63 .. 129 bytes of the frame), odd and
    even, with and without a VLAN tag and IPv4 options."""
    rng = np.random.default_rng(17)
    out = []
    for ver in (4, 6):
        for proto in (pg.IPPROTO_UDP, pg.IPPROTO_TCP, pg.IPPROTO_SCTP):
            for vlan, ipopt in ((False, False), (True, False), (False, ver == 4)):
                fr0, l3, l4 = CK.build(rng, ver, proto, payload=b"", vlan=vlan, ipopt=ipopt)
                for total in (63, 64, 65, 66, 127, 128, 129, 131, 191, 192, 193):
                    k = total - len(fr0)
                    if k < 0:
                        continue
                    pay = bytes(rng.integers(0, 256, k).astype(np.uint8))
                    fr, l3, l4 = CK.build(rng, ver, proto, payload=pay, vlan=vlan, ipopt=ipopt)
                    assert len(fr) == total
                    out.append((TX.scramble(fr, l3, l4), l3, l4))
    return out


def test_piece_boundaries(tx):
    items = boundary_items()
    assert len(items) > 150
    b, desc = framed(items)
    _, done = check(tx, b, desc, TX.ALL_TX, "piece boundaries")
    assert (done & (TX.DONE_UDP | TX.DONE_TCP | TX.DONE_SCTP) != 0).all()


def test_odd_l3(tx):
    """One byte in front of the L2 header: l3 and l4 are odd frame offsets."""
    items = [(b"\xa5" + f, l3 + 1, l4 + 1) for f, l3, l4 in boundary_items() + matrix_items()[:200]]
    b, desc = framed(items)
    _, done = check(tx, b, desc, TX.ALL_TX, "odd l3")
    assert (done != 0).all()


def test_unaligned_offsets(tx):
    """Frames at arbitrary byte offsets of the batch."""
    items = boundary_items() + matrix_items()[:150]
    rng = np.random.default_rng(8)
    off, pos = [], 1
    for f, _, _ in items:
        off.append(pos)
        pos += len(f) + int(rng.integers(0, 40))
    buf = np.zeros(pos + 64, np.uint8)
    for o, (f, _, _) in zip(off, items):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    b = pg.Batch(buf, np.array(off, np.uint32), np.array([len(f) for f, _, _ in items], np.uint16))
    desc = TX.make_desc([l3 for _, l3, _ in items], [l4 for _, _, l4 in items], 0)
    check(tx, b, desc, TX.ALL_TX, "unaligned")


def _built(lens, ipver, proto, ntags=None, seed=3):
    n = len(lens)
    rng = np.random.default_rng(seed)
    return pg.build_batch(np.asarray(lens), ipver=np.asarray(ipver), l4proto=np.asarray(proto),
                          sip4=rng.integers(0, 2**32, n).astype(np.uint64),
                          dip4=rng.integers(0, 2**32, n).astype(np.uint64),
                          sip6=rng.integers(0, 256, (n, 16), dtype=np.uint8),
                          dip6=rng.integers(0, 256, (n, 16), dtype=np.uint8),
                          sport=rng.integers(1, 65535, n), dport=rng.integers(1, 65535, n),
                          ntags=None if ntags is None else np.asarray(ntags),
                          vid0=np.full(n, 5), vid1=np.full(n, 6), seed=seed)


def _built_desc(b, ipver, ntags=None):
    ntags = np.zeros(b.n, np.int64) if ntags is None else np.asarray(ntags)
    l3 = 14 + 4 * ntags
    return TX.make_desc(l3, l3 + np.where(np.asarray(ipver) == 4, 20, 40), 0)


def test_jumbo_udp_among_small(tx):
    """One 9000-B UDP frame (more than 64 pieces: several rounds of the
    cooperative sum) among 60-B frames of one tile."""
    lens = [60] * 37 + [9000] + [60] * 26 + [61, 9001]
    ipver = [4, 6] * 33
    b = _built(lens, ipver, [pg.IPPROTO_UDP] * 66)
    _, done = check(tx, b, _built_desc(b, ipver), TX.ALL_TX, "jumbo udp")
    assert (done & TX.DONE_UDP != 0).all()


def test_sctp_long_frames(tx):
    """SCTP frames longer than 64 (CRC_ZN - 1) = 16320 bytes take the
    one-lane CRC, beside frames on the cooperative path."""
    lens = [60, 98, 16320, 16321, 16400, 131, 20001, 1514, 99]
    ipver = [4, 6, 4, 4, 6, 4, 4, 6, 6]
    b = _built(lens, ipver, [pg.IPPROTO_SCTP] * len(lens))
    desc = _built_desc(b, ipver)
    _, done = check(tx, b, desc, TX.CK_SCTP, "sctp long")
    assert (done == TX.DONE_SCTP).all()
    # the same frames behind 1 and 3 more bytes of L2: the one-lane CRC with l4
    # at 3 and 1 mod 4 (a 15-byte L2), the cooperative one at odd l4
    for pad in (1, 3):
        items = [(b"\xa5" * pad + b.frame(i), int(desc["l3"][i]) + pad, int(desc["l4"][i]) + pad)
                 for i in range(b.n)]
        bp, dp = framed(items)
        _, done = check(tx, bp, dp, TX.CK_SCTP, f"sctp long, l4 + {pad}")
        assert (done == TX.DONE_SCTP).all()


def test_vlan_qinq(tx):
    rng = np.random.default_rng(23)
    n = 192
    lens = rng.integers(60, 400, n)
    ipver = rng.choice([4, 6], n)
    proto = rng.choice([pg.IPPROTO_UDP, pg.IPPROTO_TCP, pg.IPPROTO_SCTP], n)
    ntags = rng.integers(0, 3, n)
    b = _built(lens, ipver, proto, ntags)
    _, done = check(tx, b, _built_desc(b, ipver, ntags), TX.ALL_TX, "vlan / qinq")
    assert (done != 0).all()


def _edit(frame, **at):
    b = bytearray(frame)
    for k, v in at.items():
        o = int(k[1:])
        b[o:o + len(v)] = v
    return bytes(b)


def test_decision_edges(tx):
    """Every rule of the decision that leaves a packet, or one of its
    checksums, alone; the done bits say which branch each frame took."""
    rng = np.random.default_rng(29)
    pay = bytes(rng.integers(0, 256, 40).astype(np.uint8))
    u4, l3, l4 = CK.build(rng, 4, pg.IPPROTO_UDP, payload=pay)
    t4, _, _ = CK.build(rng, 4, pg.IPPROTO_TCP, payload=pay)
    s4, _, _ = CK.build(rng, 4, pg.IPPROTO_SCTP, payload=pay)
    u6, l36, l46 = CK.build(rng, 6, pg.IPPROTO_UDP, payload=pay)
    s6, _, _ = CK.build(rng, 6, pg.IPPROTO_SCTP, payload=pay)
    u4o, l3o, l4o = CK.build(rng, 4, pg.IPPROTO_UDP, payload=pay, ipopt=True)
    sc = TX.scramble
    inv = TX.INVALID
    ip, udp, tcp, sctp = TX.DONE_IPV4, TX.DONE_UDP, TX.DONE_TCP, TX.DONE_SCTP
    # a UDP frame whose computed checksum is 0: the last payload word makes
    # the folded sum 0xFFFF
    z = bytearray(u4)
    z[l4 + 6:l4 + 8] = b"\x00\x00"
    z[-2:] = b"\x00\x00"
    s = CK.ones_sum(bytes(z[l3 + 12:l3 + 20]) + struct.pack("!BBH", 0, 17, len(z) - l4) + bytes(z[l4:]))
    z[-2:] = struct.pack("!H", 0xFFFF - s)
    z = bytes(z)
    assert CK.inet_csum(z[l3 + 12:l3 + 20] + struct.pack("!BBH", 0, 17, len(z) - l4) + z[l4:]) == 0
    cases = [
        (sc(u4, l3, l4), inv, l4, 0),                       # l3 invalid
        (sc(u4, l3, l4), l3, inv, ip),                      # l4 invalid
        (sc(u4, l3, l4), len(u4), l4, 0),                   # l3 at the frame's end
        (_edit(sc(u4, l3, l4), **{f"o{l3}": b"\x55"}), l3, l4, 0),   # version 5
        (_edit(sc(u6, l36, l46), **{f"o{l36}": b"\x70"}), l36, l46, 0),
        (sc(u4, l3, l4)[:l3 + 19], l3, l4, 0),              # len - l3 = 19
        (sc(u6, l36, l46)[:l36 + 39], l36, l46, 0),         # len - l3 = 39
        (_edit(sc(u4, l3, l4), **{f"o{l3}": b"\x44"}), l3, l4, udp),  # IHL 4: no IPv4 sum
        (_edit(sc(u4, l3, l4), **{f"o{l3}": b"\x4f"})[:l4 + 12], l3, l4, udp),  # header past len
        (_edit(sc(u4, l3, l4), **{f"o{l3 + 6}": b"\x20\x00"}), l3, l4, ip),     # MF
        (_edit(sc(t4, l3, l4), **{f"o{l3 + 6}": b"\x00\x05"}), l3, l4, ip),     # fragment offset
        (_edit(sc(u4, l3, l4), **{f"o{l3 + 6}": b"\xc0\x00"}), l3, l4, ip | udp),   # DF / reserved only
        (_edit(sc(u6, l36, l46), **{f"o{l36 + 6}": b"\x00"}), l36, l46, 0),     # IPv6 hop-by-hop
        (_edit(sc(u4, l3, l4), **{f"o{l4 + 4}": b"\x12\x34"}), l3, l4, ip | udp),   # UDP length differs
        (_edit(sc(u6, l36, l46), **{f"o{l46 + 4}": b"\x00\x07"}), l36, l46, udp),
        (sc(z, l3, l4), l3, l4, ip | udp),                  # computed 0 -> 0xFFFF
        (sc(u4, l3, l4)[:l4 + 7], l3, l4, ip),              # checksum fields past len
        (sc(t4, l3, l4)[:l4 + 17], l3, l4, ip),
        (sc(s4, l3, l4)[:l4 + 11], l3, l4, ip),
        (sc(s6, l36, l46)[:l46 + 11], l36, l46, 0),
        (sc(u4, l3, l4)[:l4 + 8], l3, l4, ip | udp),        # fields ending at len
        (sc(t4, l3, l4)[:l4 + 18], l3, l4, ip | tcp),
        (sc(s4, l3, l4)[:l4 + 12], l3, l4, ip | sctp),
        (sc(u4, l3, l4), l3, l4 + 1, ip),                   # l4 - l3 odd
        (sc(u4, l3, l4), l3, l4 - 2, ip),                   # l4 - l3 below the IP header
        (sc(u6, l36, l46), l36, l46 - 2, 0),
        (sc(u4, l3, l4), l3, l4 + 2, ip | udp),             # the given l4 is used as it is
        (sc(u4o, l3o, l4o), l3o, l4o, ip | udp),            # IPv4 options
        (sc(u4o, l3o, l4o), l3o, l3o + 20, ip | udp),       # l4 inside the options
    ]
    items = [(f, a, b_) for f, a, b_, _ in cases]
    b, desc = framed(items)
    buf, done = check(tx, b, desc, TX.ALL_TX, "decision edges")
    assert done.tolist() == [d for _, _, _, d in cases]
    zi = [i for i, c in enumerate(cases) if c[0] == sc(z, l3, l4)][0]
    o = int(b.off[zi]) + l4 + 6
    assert bytes(buf[o:o + 2]) == b"\xff\xff"


def test_imix_insert_then_validate(tx):
    """IMIX traffic with every checksum field zero: after the insert the
    buffer is pg.set_checksums of the same batch, and the receive path with
    every validation and drop option on finds no error and drops nothing."""
    n = 4096
    rng = np.random.default_rng(51)
    lens = pg.imix_lens(rng, n)
    lens = np.where(rng.random(n) < 0.2, rng.integers(61, 1514, n), lens)
    ipver = rng.choice([4, 6], n)
    proto = rng.choice([pg.IPPROTO_UDP, pg.IPPROTO_TCP, pg.IPPROTO_SCTP], n)
    b = _built(lens, ipver, proto, seed=13)
    exp = pg.set_checksums(pg.Batch(b.buf.copy(), b.off, b.len))
    buf, done = tx.insert(b, _built_desc(b, ipver), TX.ALL_TX)
    assert np.array_equal(buf, exp.buf)
    want = np.where(ipver == 4, TX.DONE_IPV4, 0) | np.where(
        proto == pg.IPPROTO_UDP, TX.DONE_UDP, np.where(proto == pg.IPPROTO_TCP, TX.DONE_TCP, TX.DONE_SCTP))
    assert np.array_equal(done, want.astype(np.uint8))
    got = gpu_run([R.cos("d", queue=1), ("default", 0)], pg.Batch(buf, b.off, b.len),
                  pktin_opt=CK.ALL_CK | CK.ALL_DROP)
    assert not (got["err"] & (CK.E_L3CK | CK.E_L4CK | CK.E_IP | CK.E_UDP | CK.E_TCP | CK.E_SCTP)).any()
    assert (got["outcome"] == R.OUT_ENQ).all()
    assert ((got["in_flags"] >> 31) & 1).all()
    assert np.array_equal(((got["in_flags"] >> 30) & 1).astype(bool), ipver == 4)


@pytest.mark.parametrize("submit", [False, True])
def test_host_entries(tx, submit):
    """mi_cls_chksum_insert_host from page-locked memory (in place) and from
    pageable memory (staged): both equal the device entry's result."""
    from odp_amd.cls import PinnedArray
    items = boundary_items()[:100] + matrix_items()[:90]
    b, desc = framed(items)
    dev_buf, dev_done = check(tx, b, desc, TX.ALL_TX, "device")
    n = b.n
    # pageable
    buf, off, ln = b.buf.copy(), b.off.astype(np.uint32), b.len.astype(np.uint16)
    d, done = desc.copy(), np.zeros(n, np.uint8)
    tx.insert_host(buf, off, ln, d, TX.ALL_TX, done, submit=submit)
    assert np.array_equal(buf, dev_buf) and np.array_equal(done, dev_done)
    # page-locked: buffer, descriptors and done bytes
    pins = [PinnedArray(b.buf.nbytes), PinnedArray(4 * n), PinnedArray(2 * n), PinnedArray(8 * n),
            PinnedArray(n)]
    try:
        pbuf, poff, plen = pins[0].u8, pins[1].view(np.uint32, n), pins[2].view(np.uint16, n)
        pdesc, pdone = pins[3].view(TX.DESC_DTYPE, n), pins[4].u8
        pbuf[:] = b.buf
        poff[:] = off
        plen[:] = ln
        pdesc[:] = desc
        pdone[:] = 0
        tx.insert_host(pbuf, poff, plen, pdesc, TX.ALL_TX, pdone, submit=submit)
        assert np.array_equal(pbuf, dev_buf) and np.array_equal(pdone[:n], dev_done)
        # without done bytes
        pbuf[:] = b.buf
        tx.insert_host(pbuf, poff, plen, pdesc, TX.ALL_TX, None, submit=submit)
        assert np.array_equal(pbuf, dev_buf)
    finally:
        for p in pins:
            p.close()
    tx.insert_host(buf, off[:0], ln[:0], d[:0], TX.ALL_TX, None, submit=submit)   # n == 0


# ------------------------------------------------------------ loop round trip
def _round_trip(tmp_path, pktout, pktin, ovr, env=None):
    frames = [fr for fr, _ in TX.valid_frames(seed=9, n=150)]
    items = []
    for fr in frames:
        l3, l4 = TX.offsets_of(fr)
        items.append((TX.scramble(fr, l3, l4), l3, l4))
    pcap = str(tmp_path / "tx.pcap")
    write_pcap(pcap, [f for f, _, _ in items])
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([TX_DRIVER, "loop", pcap, hex(TX.all_bits(pktout)), hex(pktin), str(ovr)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    pk, stats, sends = [], None, None
    for line in r.stdout.splitlines():
        p = line.split()
        if p[0] == "P":
            pk.append((int(p[1]), int(p[2]), int(p[3]), bytes.fromhex(p[4])))
        elif p[0] == "S":
            stats = (int(p[1]), int(p[2]))
        elif p[0] == "T":
            sends = (int(p[1]), int(p[2]))   # sends that ran the kernel, of them bounced
    assert len(pk) == len(items)
    _round_trip.sends = sends
    return items, pk, stats


OK, BAD = 2, 1


def _expect_inserted(items, pk, stats, l4_off=lambda i: False):
    """Every packet arrives with the model's bytes and OK statuses (l4_off(i):
    its L4 checksum was left alone -- BAD)."""
    for i, ((fr, l3, l4), (s3, s4, err, data)) in enumerate(zip(items, pk)):
        v4 = fr[l3] >> 4 == 4
        flags = TX.L4_SET if l4_off(i) else 0
        exp, _ = TX.insert(fr, l3, l4, flags, TX.ALL_TX)
        assert data == exp, i
        assert s3 == (OK if v4 else 0), i
        assert s4 == (BAD if l4_off(i) else OK), i
        assert err == int(l4_off(i)), i
    nbad = sum(1 for i in range(len(items)) if l4_off(i))
    assert stats == (len(items) - nbad, nbad)


def test_loop_round_trip_inserts(built, gpu, tmp_path):
    """All four pktout defaults and all pktin validations on: garbage
    checksum fields are sent, every packet is received OK, in_errors 0."""
    items, pk, stats = _round_trip(tmp_path, TX.ALL_TX, CK.ALL_CK, 0)
    _expect_inserted(items, pk, stats)
    # page-locked pool: every send ran the kernel on the frames in place
    assert _round_trip.sends[0] >= 1 and _round_trip.sends[1] == 0


def test_loop_round_trip_defaults_off_is_bad(built, gpu, tmp_path):
    """The same traffic without the pktout defaults: received unchanged and
    BAD -- the IPv4 header checksum on IPv4 (the parse stops there: L4
    unknown), the L4 checksum on IPv6."""
    items, pk, stats = _round_trip(tmp_path, 0, CK.ALL_CK, 0)
    for (fr, l3, _), (s3, s4, err, data) in zip(items, pk):
        assert data == fr
        assert (s3, s4) == ((BAD, 0) if fr[l3] >> 4 == 4 else (0, BAD)) and err == 1
    assert stats == (0, len(items))
    assert _round_trip.sends == (0, 0)   # nothing asked for a checksum: no GPU call


def test_loop_round_trip_l4_override_off(built, gpu, tmp_path):
    """odp_packet_l4_chksum_insert(pkt, 0) on every odd packet."""
    items, pk, stats = _round_trip(tmp_path, TX.ALL_TX, CK.ALL_CK, 1)
    _expect_inserted(items, pk, stats, l4_off=lambda i: i % 2 == 1)


def test_loop_round_trip_override_on(built, gpu, tmp_path):
    """Defaults off, odp_packet_l3/l4_chksum_insert(pkt, 1) on every packet."""
    items, pk, stats = _round_trip(tmp_path, TX.ALL_ENA, CK.ALL_CK, 2)
    _expect_inserted(items, pk, stats)


def test_loop_round_trip_receive_clears_overrides(built, gpu, tmp_path):
    """Every packet is sent with odp_packet_l4_chksum_insert(pkt, 0), received
    (L4 BAD), and sent again as it came back: a received packet carries no
    override, so the second send inserts the L4 checksum under the defaults."""
    items, pk, stats = _round_trip(tmp_path, TX.ALL_TX, CK.ALL_CK, 3)
    for i, ((fr, l3, l4), (s3, s4, err, data)) in enumerate(zip(items, pk)):
        exp, _ = TX.insert(fr, l3, l4, 0, TX.ALL_TX)
        assert data == exp, i
        assert (s3, s4, err) == (OK if fr[l3] >> 4 == 4 else 0, OK, 0), i
    assert stats == (len(items), len(items))   # first pass: every L4 BAD


@pytest.mark.parametrize("env", [{"ODP_AMD_PAGEABLE_POOLS": "pktio_pool"}, {"ODP_AMD_PINNED_POOLS": "0"}],
                         ids=["pageable_pool", "no_pinned_pools"])
def test_loop_round_trip_pageable_pool(built, gpu, tmp_path, env):
    """The pool in ordinary memory: the send goes through the bounce buffer."""
    items, pk, stats = _round_trip(tmp_path, TX.ALL_TX, CK.ALL_CK, 0, env=env)
    _expect_inserted(items, pk, stats)
    # every send that ran the kernel took the bounce path, none the in-place one
    assert _round_trip.sends[0] >= 1 and _round_trip.sends[1] == _round_trip.sends[0]
