"""The pktin flow hash on the GPU (mi_cls_tx_hash, its host entries and the
loop pktio's input queues) vs the model of get_dest_queue
(tests/txq_model.py): all 32 bits of every hash word, the hash buffer
poisoned before every launch, over every hash_proto value, the fit edges of
every header, metadata that contradicts the bytes, the batch sizes, and what
the two instantiations may write: the hash alone no frame byte, the hash
with checksums exactly what mi_cls_chksum_insert writes."""
import os
import subprocess

import numpy as np
import pytest

from odp_amd import pktgen as pg
from tests import chksum_frames as CK
from tests import parse_model as PM
from tests import tx_model as TX
from tests import txq_model as TQ
from tests.rt_helpers import write_pcap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MQ_DRIVER = os.path.join(ROOT, "tests", "_bin", "mq_driver")
POISON = 0xA5A5A5A5


@pytest.fixture(scope="module")
def tx(built, gpu):
    from odp_amd.cls import TxContext
    c = TxContext(0)
    yield c
    c.close()


def parsed(frame, front=0):
    """(frame, l3, l4, metadata flags) as odp_packet_parse leaves them; front:
    bytes in front of the Ethernet header (a 15-byte L2 for front = 1)."""
    fr = b"\xa5" * front + frame
    _, fl, _, _, l3, l4 = PM.parse(fr, front, PM.PROTO_ETH, PM.ALL, 0)
    return fr, l3, l4, TQ.meta_flags(fl)


_set = {}


def mixed_items():
    """About 200 frames: UDP, TCP, SCTP, ICMP over IPv4 and IPv6, and ARP;
    with and without a VLAN tag, IPv4 options, a 15-byte L2."""
    if "items" in _set:
        return _set["items"]
    rng = np.random.default_rng(41)
    out = []
    k = 0
    for rep in range(8):
        for ver in (4, 6):
            for proto in (pg.IPPROTO_UDP, pg.IPPROTO_TCP, pg.IPPROTO_SCTP, "icmp"):
                for vlan, ipopt in ((False, False), (True, False), (False, ver == 4)):
                    if proto == "icmp":
                        e = pg.eth(ethtype=pg.ETH_IPV4 if ver == 4 else pg.ETH_IPV6, tags=(7,) if vlan else ())
                        src = bytes(rng.integers(0, 256, 4 if ver == 4 else 16).astype(np.uint8))
                        dst = bytes(rng.integers(0, 256, 4 if ver == 4 else 16).astype(np.uint8))
                        body = pg.icmp() + bytes(rng.integers(0, 256, 24).astype(np.uint8))
                        ip = (pg.ipv4(src=src, dst=dst, proto=1, payload_len=len(body),
                                      options=b"\x01\x01\x01\x00" if ipopt else b"") if ver == 4 else
                              pg.ipv6(src=src, dst=dst, next_hdr=58, payload_len=len(body)))
                        fr = bytes(e) + bytes(ip) + body
                    else:
                        fr, _, _ = CK.build(rng, ver, proto, vlan=vlan, ipopt=ipopt)
                    out.append(parsed(fr, front=1 if k % 4 == 3 else 0))
                    k += 1
    for i in range(8):
        arp = bytes(pg.eth(ethtype=0x0806)) + bytes(rng.integers(0, 256, 28).astype(np.uint8)) + bytes(18)
        out.append(parsed(arp, front=i & 1))
    flags = [f for _, _, _, f in out]
    for bit in (TQ.F_UDP, TQ.F_TCP, TQ.F_IPV4, TQ.F_IPV6):
        assert sum(1 for f in flags if f & bit) >= 20
    assert sum(1 for f in flags if f == 0) >= 8 and sum(1 for _, l3, _, _ in out if l3 & 1) >= 30
    _set["items"] = out
    return out


def framed(items, low=0):
    """Batch + descriptors of [(frame, l3, l4, metadata flags)]; low: the
    checksum override bits (a value or one per packet)."""
    b = pg.batch_from_frames([f for f, _, _, _ in items])
    fl = np.array([m for _, _, _, m in items], np.uint8) | np.asarray(low, np.uint8)
    return b, TX.make_desc([a for _, a, _, _ in items], [c for _, _, c, _ in items], fl)


def unaligned(items, low=0, seed=8):
    """The same at arbitrary byte offsets of the batch."""
    rng = np.random.default_rng(seed)
    off, pos = [], 1
    for f, _, _, _ in items:
        off.append(pos)
        pos += len(f) + int(rng.integers(0, 40))
    buf = np.zeros(pos + 64, np.uint8)
    for o, (f, _, _, _) in zip(off, items):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    b = pg.Batch(buf, np.array(off, np.uint32), np.array([len(f) for f, _, _, _ in items], np.uint16))
    _, desc = framed(items, low)
    return b, desc


def check_hash(tx, b, desc, hp, what=""):
    """The hash alone: GPU == model on all 32 bits, no frame byte written,
    done bytes zero."""
    exp, ln = TQ.apply(b.buf, b.off, b.len, desc, hp)
    buf, done, h = tx.hash(b, desc, hp, poison=POISON)
    bad = np.nonzero(h != exp)[0]
    assert bad.size == 0, (what, hp, bad[:8], [hex(int(x)) for x in h[bad[:4]]],
                           [hex(int(x)) for x in exp[bad[:4]]], ln[bad[:8]], desc[bad[:4]])
    assert np.array_equal(buf, b.buf), (what, "the hash alone wrote a frame byte")
    assert not done.any()
    return h, ln


def test_every_hash_proto(tx):
    """All 63 non-zero values of hash_proto over the mixed set, frames packed
    at 16-B slots and at arbitrary byte offsets."""
    items = mixed_items()
    assert 180 <= len(items) <= 260
    for b, desc in (framed(items), unaligned(items)):
        seen = set()
        for hp in range(1, 64):
            _, ln = check_hash(tx, b, desc, hp, "every bit")
            seen |= set(int(x) for x in ln)
        assert seen == {0, 4, 8, 12, 32, 36}


def edge_items():
    """Each fit condition on both sides, invalid offsets, and metadata that
    contradicts the bytes (the hash follows the metadata)."""
    rng = np.random.default_rng(43)
    pay = bytes(rng.integers(0, 256, 48).astype(np.uint8))
    u4, l3, l4 = CK.build(rng, 4, pg.IPPROTO_UDP, payload=pay)
    t4, _, _ = CK.build(rng, 4, pg.IPPROTO_TCP, payload=pay)
    u6, l36, l46 = CK.build(rng, 6, pg.IPPROTO_UDP, payload=pay)
    t6, _, _ = CK.build(rng, 6, pg.IPPROTO_TCP, payload=pay)
    U, T, V4, V6 = TQ.F_UDP, TQ.F_TCP, TQ.F_IPV4, TQ.F_IPV6
    inv = TQ.INVALID
    return [
        (u4[:l4 + 8], l3, l4, U | V4), (u4[:l4 + 7], l3, l4, U | V4),          # UDP header fits / not
        (u6[:l46 + 8], l36, l46, U | V6), (u6[:l46 + 7], l36, l46, U | V6),
        (t4[:l4 + 20], l3, l4, T | V4), (t4[:l4 + 19], l3, l4, T | V4),        # TCP
        (t6[:l46 + 20], l36, l46, T | V6), (t6[:l46 + 19], l36, l46, T | V6),
        (u4[:l3 + 20], l3, l4, U | V4), (u4[:l3 + 19], l3, l4, U | V4),        # IPv4
        (u6[:l36 + 40], l36, l46, U | V6), (u6[:l36 + 39], l36, l46, U | V6),  # IPv6
        (u4, l3, inv, U | V4), (u4, inv, l4, U | V4), (u4, inv, inv, U | V4),  # invalid offsets
        (u6, l36, inv, U | V6), (t6, inv, l46, T | V6),
        (t4, l3, l4, U | V4),            # has_udp on a TCP frame
        (u4, l3, l4, T | V4),            # has_tcp on a UDP frame
        (u4, l3, l4, U | V6),            # has_ipv6 on an IPv4 frame (32 bytes from l3 + 8 fit)
        (u6, l36, l46, U | V4),          # has_ipv4 on an IPv6 frame
        (t4, l3, l4, U | T | V4),        # both L4 flags: UDP wins
        (t4[:l4 + 12], l3, l4, U | T | V4),   # ... also where only it fits
        (t4[:l4 + 7], l3, l4, U | T | V4),    # ... and where it does not: TCP is not tried
        (u4, l3, l4, U | V4 | V6),       # both L3 flags: IPv4 wins
        (u4[:l3 + 19], l3, l4, V4 | V6),      # ... and where it does not fit IPv6 is not tried
        (u4, l3, l4, 0),                 # no metadata: the empty string
        (u4, l3, l4 + 3, U | V4), (u6, l36 + 1, l46, U | V6),   # the given offsets are used as they are
    ]


def test_fit_edges_in_one_tile(tx):
    edges = edge_items()
    ordinary = mixed_items()
    items = ordinary[:18] + edges + ordinary[18:64 - len(edges)]
    assert len(items) == 64
    for b, desc in (framed(items), unaligned(items, seed=9)):
        for hp in (63, 1, 2, 4, 32, 8 | 16, 1 | 32, 2 | 4, 36):
            h, ln = check_hash(tx, b, desc, hp, "edges")
            if hp == 63:
                e = ln[18:18 + len(edges)].tolist()
                # fits / does not: ports + addresses, addresses alone, ...
                assert e[:12] == [12, 8, 36, 32, 12, 8, 36, 32, 8, 0, 32, 0]
                assert e[12:17] == [8, 4, 0, 32, 4]
                assert e[17:] == [12, 12, 36, 12, 12, 12, 8, 12, 0, 0, 12, 36]
                assert h[18 + 26] == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(tx, n):
    b, desc = framed(mixed_items()[:n])
    check_hash(tx, b, desc, 63, f"n={n}")
    check_both(tx, b, desc, 63, TX.ALL_TX, f"n={n}")


def check_both(tx, b, desc, hp, opt, what=""):
    """The hash with checksums: the buffer and the done bytes are those of
    the checksum model (and so of mi_cls_chksum_insert), the hash the model's
    over the frames as the insertion leaves them (the reference fixes the
    checksums, then picks the queue: loop.c:581-582)."""
    exp_buf, exp_done = TX.apply(b.buf, b.off, b.len, desc, opt)
    exp, _ = TQ.apply(exp_buf, b.off, b.len, desc, hp)
    buf, done, h = tx.hash(b, desc, hp, opt=opt, chksum=True, poison=POISON)
    assert np.array_equal(buf, exp_buf), (what, np.nonzero(buf != exp_buf)[0][:8])
    assert np.array_equal(done, exp_done), (what, np.nonzero(done != exp_done)[0][:8])
    assert np.array_equal(h, exp), (what, np.nonzero(h != exp)[0][:8])
    return buf, done


@pytest.mark.parametrize("row", ["all_defaults", "mixed_overrides"])
def test_with_checksums_writes_what_insert_writes(tx, row):
    items = [(TX.scramble(f, l3, l4) if l4 != TX.INVALID and m & (TQ.F_IPV4 | TQ.F_IPV6) else f, l3, l4, m)
             for f, l3, l4, m in mixed_items()] + edge_items()
    if row == "all_defaults":
        opt, low = TX.ALL_TX, 0
    else:
        opt, low = TX.CK_UDP | TX.CK_IPV4, np.random.default_rng(3).integers(0, 16, len(items)).astype(np.uint8)
    for b, desc in (framed(items, low), unaligned(items, low)):
        buf, done = check_both(tx, b, desc, 63, opt, row)
        ibuf, idone = tx.insert(b, desc, opt)
        assert np.array_equal(buf, ibuf) and np.array_equal(done, idone)
        assert done.any()
        check_both(tx, b, desc, 5, opt, row)


def checksum_in_string_items():
    """Metadata that puts a checksum field of the same launch into the hash
    string, on frames whose checksum fields hold garbage: has_ipv6 on IPv4
    frames (the 32 bytes from l3 + 8 hold the IPv4 header checksum and, past
    the 20-byte header, the UDP / TCP / SCTP field, whole or cut by the
    string's end), and an l4 inside the IPv4 header (the ports dword holds
    the IPv4 header checksum)."""
    rng = np.random.default_rng(47)
    pay = bytes(rng.integers(0, 256, 48).astype(np.uint8))
    U, T, V4, V6 = TQ.F_UDP, TQ.F_TCP, TQ.F_IPV4, TQ.F_IPV6
    out = []
    for proto in (pg.IPPROTO_UDP, pg.IPPROTO_TCP, pg.IPPROTO_SCTP):
        for ipopt in (False, True):
            fr, l3, l4 = CK.build(rng, 4, proto, payload=pay, ipopt=ipopt)
            sc = TX.scramble(fr, l3, l4)
            out += [(sc, l3, l4, U | V6), (sc, l3, l4, T | V6), (sc, l3, l4, V6), (b"\xa5" + sc, l3 + 1, l4 + 1, U | V6)]
            # the application's l4: inside the IPv4 header, every overlap of the
            # ports dword with the header checksum at l3 + 10
            out += [(sc, l3, l3 + d, U | V4) for d in (6, 7, 8, 9, 10, 11, 12)]
            out += [(sc, l3, l3 + 8, U | V6)]
        # an l4 the parse would not give: the SCTP / UDP field cut by the string's end
        fr, l3, l4 = CK.build(rng, 4, proto, payload=pay)
        for d in (22, 24, 26, 28, 30, 32, 34):
            sc = TX.scramble(fr, l3, l3 + d)
            out.append((sc, l3, l3 + d, U | T | V6))
    return out


@pytest.mark.parametrize("row", ["all_defaults", "mixed_overrides"])
def test_hash_follows_the_inserted_checksums(tx, row):
    """The hash is of the bytes after insertion, also where contradicting
    metadata makes a checksum field part of the string; the test input does
    have such strings, and their hash changes with the insertion."""
    items = checksum_in_string_items() + mixed_items()[:30]
    if row == "all_defaults":
        opt, low = TX.ALL_TX, 0
    else:
        opt, low = TX.CK_UDP | TX.CK_IPV4, np.random.default_rng(5).integers(0, 16, len(items)).astype(np.uint8)
    for b, desc in (framed(items, low), unaligned(items, low, seed=11)):
        for hp in (63, 32, 1 | 32, 8, 2 | 32):
            before, _ = TQ.apply(b.buf, b.off, b.len, desc, hp)
            after, _ = TQ.apply(TX.apply(b.buf, b.off, b.len, desc, opt)[0], b.off, b.len, desc, hp)
            if hp in (63, 32):
                assert (before != after).sum() >= 30
            check_both(tx, b, desc, hp, opt, row)
            check_hash(tx, b, desc, hp, row)   # alone: nothing is inserted, the bytes as they are


@pytest.mark.parametrize("submit", [False, True])
def test_host_entries(tx, submit):
    """mi_cls_tx_hash_host in place (everything page-locked), staged
    (pageable), and as the submit / wait pair: the device entry's hashes."""
    from odp_amd.cls import PinnedArray
    items = mixed_items()[:150] + edge_items()
    b, desc = framed(items)
    n = b.n
    ck_buf, ck_done = TX.apply(b.buf, b.off, b.len, desc, TX.ALL_TX)
    exp_by = {False: TQ.apply(b.buf, b.off, b.len, desc, 63)[0], True: TQ.apply(ck_buf, b.off, b.len, desc, 63)[0]}
    off, ln = b.off.astype(np.uint32), b.len.astype(np.uint16)
    for ck in (False, True):
        exp = exp_by[ck]
        # pageable: staged
        buf, d = b.buf.copy(), desc.copy()
        h, done = np.full(n, POISON, np.uint32), np.full(n, 0xEE, np.uint8)
        tx.hash_host(buf, off, ln, d, 63, h, opt=TX.ALL_TX, chksum=ck, done=done, submit=submit)
        assert np.array_equal(h, exp)
        assert np.array_equal(buf, ck_buf if ck else b.buf)
        assert np.array_equal(done, ck_done if ck else np.zeros(n, np.uint8))
        # page-locked: in place
        pins = [PinnedArray(b.buf.nbytes), PinnedArray(4 * n), PinnedArray(2 * n), PinnedArray(8 * n),
                PinnedArray(n), PinnedArray(4 * n)]
        try:
            pbuf, poff, plen = pins[0].u8, pins[1].view(np.uint32, n), pins[2].view(np.uint16, n)
            pdesc, pdone, ph = pins[3].view(TX.DESC_DTYPE, n), pins[4].u8, pins[5].view(np.uint32, n)
            pbuf[:] = b.buf
            poff[:] = off
            plen[:] = ln
            pdesc[:] = desc
            pdone[:] = 0xEE
            ph[:] = POISON
            tx.hash_host(pbuf, poff, plen, pdesc, 63, ph, opt=TX.ALL_TX, chksum=ck, done=pdone, submit=submit)
            assert np.array_equal(ph, exp)
            assert np.array_equal(pbuf, ck_buf if ck else b.buf)
            assert np.array_equal(pdone[:n], ck_done if ck else np.zeros(n, np.uint8))
            # a pageable hash array alone sends the call through the staging buffers
            pbuf[:] = b.buf
            h[:] = POISON
            tx.hash_host(pbuf, poff, plen, pdesc, 63, h, opt=TX.ALL_TX, chksum=ck, done=None, submit=submit)
            assert np.array_equal(h, exp) and np.array_equal(pbuf, ck_buf if ck else b.buf)
        finally:
            for p in pins:
                p.close()
    tx.hash_host(b.buf.copy(), off[:0], ln[:0], desc[:0], 63, np.zeros(1, np.uint32), submit=submit)   # n == 0


def test_argument_checks(tx):
    b, desc = framed(mixed_items()[:4])
    off, ln = b.off.astype(np.uint32), b.len.astype(np.uint16)
    h = np.zeros(4, np.uint32)
    args = (tx.ctx, b.buf.ctypes.data, b.buf.nbytes, off.ctypes.data, ln.ctypes.data, desc.ctypes.data, 4, 0, None)
    assert tx.L.mi_cls_tx_hash_host(*args, 0, h.ctypes.data, 0) == -22     # hash_proto 0
    assert tx.L.mi_cls_tx_hash_host(*args, 64, h.ctypes.data, 0) == -22    # more than six bits
    assert tx.L.mi_cls_tx_hash_host(*args, 63, None, 0) == -22             # hash_out is required
    assert tx.L.mi_cls_tx_hash_host(*args[:2], 8, *args[3:], 63, h.ctypes.data, 0) == -22   # frames past `bytes`


# ------------------------------------------------- loop pktio, input queues
_rt = {}


def rt_items():
    """Frames for the runtime round trip (no filler in front: the driver
    parses each from its first byte), with their metadata by the parse model;
    all different, and by the model all four queues get some."""
    if "items" not in _rt:
        items = [it for it in mixed_items() if it[1] & 1 == 0]
        for f, _, _, _ in items:
            assert PM.parse(f, 0, PM.PROTO_ETH, PM.ALL, 0)[0] == 0
        assert len(set(f for f, _, _, _ in items)) == len(items) and 100 <= len(items) <= 200
        _rt["items"] = items
    return _rt["items"]


def model_queues(items, hp, nq):
    return [TQ.flow_hash(f, l3, l4, m, hp)[0] % nq for f, l3, l4, m in items]


def mq_run(tmp_path, frames, mode, nq, hp, nout=1, pktout=0, qsize=0, env=None):
    pcap = str(tmp_path / "mq.pcap")
    write_pcap(pcap, frames)
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([MQ_DRIVER, "loop", pcap, mode, str(nq), hex(hp), str(nout), hex(TX.all_bits(pktout)),
                        str(qsize)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2000:])
    out = {"P": [], "SENT": [], "QS": {}, "OS": {}, "U": None}
    for line in r.stdout.splitlines():
        p = line.split()
        if p[0] == "P":
            out["P"].append((int(p[1]), bytes.fromhex(p[2])))
        elif p[0] == "SENT":
            out["SENT"].append((int(p[1]), int(p[2]), int(p[3])))
        elif p[0] in ("QS", "OS"):
            out[p[0]][int(p[1])] = (int(p[2]), int(p[3]))
        elif p[0] == "U":
            out["U"] = (int(p[1]), int(p[2]))
        elif p[0] in ("S", "T"):
            out[p[0]] = tuple(int(x) for x in p[1:])
    return out


def check_arrivals(out, frames, queues, nq, nout_share=None):
    """Every sent frame arrived on its queue, each queue's in send order, and
    the per-queue and pktio statistics add up."""
    per = {q: [f for f, qq in zip(frames, queues) if qq == q] for q in range(nq)}
    for q in range(nq):
        assert [f for qi, f in out["P"] if qi == q] == per[q], q
    assert len(out["P"]) == len(frames)
    for q in range(nq):
        assert out["QS"][q] == (len(per[q]), sum(len(f) for f in per[q])), q
    tot = (len(frames), sum(len(f) for f in frames))
    assert out["S"] == tot + tot
    assert (sum(v[0] for v in out["OS"].values()), sum(v[1] for v in out["OS"].values())) == tot


@pytest.mark.parametrize("mode", ["direct", "sched"])
def test_loop_four_hashed_queues(built, gpu, tmp_path, mode):
    """4 input queues, all six protocol bits, one send call: every packet on
    model_hash % 4 (in SCHED mode from odp_pktin_event_queue()[i]), one launch."""
    items = rt_items()
    queues = model_queues(items, 63, 4)
    assert all(queues.count(q) >= 8 for q in range(4))   # a condition on the input
    frames = [f for f, _, _, _ in items]
    out = mq_run(tmp_path, frames, mode, 4, 63)
    assert out["SENT"] == [(0, len(frames), len(frames))]
    check_arrivals(out, frames, queues, 4)
    assert out["OS"][0][0] == len(frames)
    assert out["T"] == (1, 0, 1)   # one launch for the call: the hash alone, in place


def test_loop_ports_only_bits(built, gpu, tmp_path):
    """Only ipv4_udp: UDP packets hash their ports alone, the rest go to queue 0."""
    items = rt_items()
    queues = model_queues(items, TQ.HP_IPV4_UDP, 3)
    assert len(set(queues)) == 3 and queues.count(0) > len(items) // 2
    frames = [f for f, _, _, _ in items]
    out = mq_run(tmp_path, frames, "direct", 3, TQ.HP_IPV4_UDP)
    check_arrivals(out, frames, queues, 3)


def test_loop_hash_off_uses_pktout_index(built, gpu, tmp_path):
    """hash_enable 0, 4 input and 3 pktout queues: a send on pktout j arrives
    on input queue j % 4, with no launch."""
    frames = [f for f, _, _, _ in rt_items()]
    n = len(frames)
    out = mq_run(tmp_path, frames, "direct", 4, 0, nout=3)
    shares = [(n * j // 3, n * (j + 1) // 3) for j in range(3)]
    assert out["SENT"] == [(j, hi - lo, hi - lo) for j, (lo, hi) in enumerate(shares)]
    queues = [j for j, (lo, hi) in enumerate(shares) for _ in range(hi - lo)]
    check_arrivals(out, frames, queues, 4)
    assert out["QS"][3] == (0, 0)
    for j, (lo, hi) in enumerate(shares):
        assert out["OS"][j] == (hi - lo, sum(len(f) for f in frames[lo:hi]))
    assert out["T"] == (0, 0, 0)


def test_loop_hash_and_checksums_one_launch(built, gpu, tmp_path):
    """pktout checksums configured beside 4 hashed queues: one launch per send
    call, the frames arrive with the model's checksums on the model's queues."""
    items = [(TX.scramble(f, l3, l4) if l4 != TX.INVALID and m & (TQ.F_IPV4 | TQ.F_IPV6) else f, l3, l4, m)
             for f, l3, l4, m in rt_items()]
    exp = [TX.insert(f, l3, l4, 0, TX.ALL_TX)[0] for f, l3, l4, _ in items]
    queues = model_queues([(x, l3, l4, m) for x, (_, l3, l4, m) in zip(exp, items)], 63, 4)   # after insertion
    assert sum(1 for (f, _, _, _), x in zip(items, exp) if f != x) > len(items) // 2
    out = mq_run(tmp_path, [f for f, _, _, _ in items], "direct", 4, 63, pktout=TX.ALL_TX)
    check_arrivals(out, exp, queues, 4)
    assert out["T"] == (1, 0, 1)
    # the pool in ordinary memory: the same through the bounce buffer
    out = mq_run(tmp_path, [f for f, _, _, _ in items], "direct", 4, 63, pktout=TX.ALL_TX,
                 env={"ODP_AMD_PAGEABLE_POOLS": "pktio_pool"})
    check_arrivals(out, exp, queues, 4)
    assert out["T"] == (1, 1, 1)


def test_loop_small_queue_returns_leading_count(built, gpu, tmp_path):
    """queue_size 16: the send stops at the first packet whose queue is full
    (loop.c:583-591), returns the count before it, and the rest stay valid."""
    items = rt_items()
    queues = model_queues(items, 63, 4)
    held = [0] * 4
    sent = len(items)
    for i, q in enumerate(queues):
        if held[q] == 16:
            sent = i
            break
        held[q] += 1
    assert 16 < sent < len(items)
    frames = [f for f, _, _, _ in items]
    out = mq_run(tmp_path, frames, "direct", 4, 63, qsize=16)
    assert out["SENT"] == [(0, sent, len(frames))]
    assert out["U"] == (len(frames) - sent, len(frames) - sent)
    check_arrivals(out, frames[:sent], queues[:sent], 4)


def test_single_queue_send_unchanged(built, gpu, tmp_path):
    """One input queue, hash_enable set: no hash is computed, and a checksum
    send makes the launches and bounces of the same send through tx_driver
    (a pktio configured as before this feature)."""
    items = [(TX.scramble(f, l3, l4), l3, l4, m) for f, l3, l4, m in rt_items()
             if l4 != TX.INVALID and m & (TQ.F_IPV4 | TQ.F_IPV6)]
    frames = [f for f, _, _, _ in items]
    out = mq_run(tmp_path, frames, "direct", 1, 63, pktout=TX.ALL_TX)
    exp = [TX.insert(f, l3, l4, 0, TX.ALL_TX)[0] for f, l3, l4, _ in items]
    check_arrivals(out, exp, [0] * len(frames), 1)
    pcap = str(tmp_path / "mq.pcap")
    r = subprocess.run([os.path.join(ROOT, "tests", "_bin", "tx_driver"), "loop", pcap, hex(TX.all_bits(TX.ALL_TX)),
                        "0", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                       env=dict(os.environ, TX_COUNT_ONLY="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    t = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("T ")][0]
    assert t == (1, 0) and out["T"] == t + (0,)
    out = mq_run(tmp_path, frames, "direct", 1, 63)   # nothing asks for a checksum: no launch at all
    assert out["T"] == (0, 0, 0)


def test_single_sized_queue_counts_what_was_sent(built, gpu, tmp_path):
    """One input queue of 16: the send returns 16 and the pktio and pktout
    counters hold those 16 packets' octets."""
    frames = [f for f, _, _, _ in rt_items()]
    out = mq_run(tmp_path, frames, "direct", 1, 0, qsize=16)
    assert out["SENT"] == [(0, 16, len(frames))] and out["U"] == (len(frames) - 16,) * 2
    check_arrivals(out, frames[:16], [0] * 16, 1)
    assert out["OS"][0] == (16, sum(len(f) for f in frames[:16]))
