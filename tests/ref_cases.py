"""Corpora and comparison rules shared by the tests that compare the oracle
(tests/test_oracle_vs_reference.py) and the kernels
(tests/test_gpu_vs_reference.py) with the reference's own compiled code
(oracle/reflib.py).  Nothing here reads the reference tree.

Field masking (by outcome only, never per frame) -- the one rule:

  cos, outcome COS_DROP   _odp_cls_classify_packet returns 1 for a drop CoS
                          (odp_classification.c:1754-1755) before it stores
                          pkt_hdr->cos (:1761): the reference does not say
                          which CoS dropped the packet.

Every other field of every outcome is compared: the parser's flags, error
bits and offsets stay in the packet header after a parse drop and after a
discard, and the mark is stored by match_pmr_cos before the drop.  `hops` has
no counterpart in the reference and is never compared.
"""
import functools

import numpy as np

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import chksum_frames as CK
from tests import parse_model as PM
from tests import zoo

LIMITS = (64, 256, 8)    # the reference's compile-time table sizes
FIELDS = ("in_flags", "err", "outcome", "cos", "queue", "mark", "l3_offset", "l4_offset")
# 24 fuzz seeds, chosen among 0..87 as those whose program the reference
# accepts (>= MIN_ACCEPTED of the PMR creates) and whose traffic reaches at
# least MIN_COS different CoS: with up to 64 CoS and at most 8 PMRs on each,
# many random programs hang nearly all their rules where no packet arrives.
FUZZ_SEEDS = (0, 5, 10, 13, 16, 17, 18, 19, 20, 23, 26, 28, 29, 36, 39, 40, 44, 63, 66, 76, 81, 82, 85, 87)
GPU_FUZZ_SEEDS = (10, 17, 40, 87)    # hash queues, drops, marks and 5+ CoS among them
DENSE_SEEDS = tuple(range(12))
MIN_ACCEPTED = 0.8
MIN_COS = 4

OPTS = {
    "all_ck": CK.ALL_CK,
    "all_ck_drop": CK.ALL_CK | CK.ALL_DROP,
    "ipv4_ck": CK.IPV4_CK,
    "drop_only": CK.ALL_DROP,
    "udp_ck_drop": CK.UDP_CK | CK.DROP_UDP,
    "sctp_tcp_ck": CK.SCTP_CK | CK.TCP_CK,
}


def comparable(rec):
    """The record array with everything the reference leaves undefined set
    to one value (see the module docstring)."""
    out = rec.copy()
    out["hops"] = 0
    out["cos"][out["outcome"] == R.OUT_COS_DROP] = 0xFF
    return out


def assert_same_ref(got, ref, batch=None, what="", who="oracle"):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g, r = comparable(got), comparable(ref)
    if np.array_equal(g, r):
        return
    bad = np.nonzero(g != r)[0]
    i = int(bad[0])
    fields = [f for f in FIELDS if g[f][i] != r[f][i]]
    msg = [f"{what}: {bad.size} of {g.size} records differ from the reference; first at {i} "
           f"in {', '.join(fields)}:", f"  {who:9s} {got[i]}", f"  reference {ref[i]}"]
    if batch is not None:
        msg.append(f"  frame     {batch.frame(i).hex()}")
    raise AssertionError("\n".join(msg))


@functools.lru_cache(maxsize=None)
def zoo_frames():
    return tuple(f for _, f in zoo.all_frames())


@functools.lru_cache(maxsize=None)
def edge_frames():
    """Header fields swept over the values a parser can tell apart, which
    random byte mutations reach too rarely: every flag / offset combination
    of the IPv4 fragment word and of the IPv6 fragment header (direct and
    behind a hop-by-hop header), QinQ and VLAN tag words, IHL and TCP data
    offset, UDP length, and IPv6 payload lengths around the extension chain."""
    import struct
    F = []
    E, E6 = pg.eth(), pg.eth(ethtype=pg.ETH_IPV6)
    for frag in (0x2000, 0x4000, 0x6000, 0x8000, 0x0001, 0x2001, 0x1FFF, 0x3FFF, 0xE000, 0xFFFF):
        for proto, l4 in ((17, pg.udp(1024, 2048, 26, bytes(18))), (6, pg.tcp(1024, 2048) + bytes(6)),
                          (132, pg.sctp(1024, 2048) + bytes(14))):
            F.append(pg.pad_to(E + pg.ipv4(proto=proto, frag=frag, payload_len=26) + l4, 60))
    for word in (0x0000, 0x0001, 0x0008, 0x0009, 0x0006, 0xFFF8, 0xFFF9, 0xFFFF):
        fh = struct.pack("!BBHI", pg.IPPROTO_UDP, 0, word, 0x12345678)
        u = pg.udp(1024, 2048, 16, bytes(8))
        F.append(pg.pad_to(E6 + pg.ipv6(next_hdr=44, payload_len=24) + fh + u, 90))
        F.append(pg.pad_to(E6 + pg.ipv6(next_hdr=0, payload_len=32) + pg.ipv6_ext(44, 0) + fh + u, 100))
        F.append(pg.pad_to(E6 + pg.ipv6(next_hdr=43, payload_len=32) + pg.ipv6_ext(44, 0) + fh + u, 100))
    for t0 in (0x0000, 0x0123, 0x0FFF, 0x1123, 0xE123, 0xF456):
        for t1 in (0x0456, 0x0123, 0xEFFF):
            F.append(pg.udp4_frame(tags=(t0, t1), size=68))
            F.append(pg.udp4_frame(tags=(t0, t1), tpids=[pg.ETH_VLAN, pg.ETH_VLAN], size=68))
            F.append(pg.udp4_frame(tags=(t0, t1), tpids=[pg.ETH_QINQ, pg.ETH_QINQ], size=68))
            F.append(pg.udp4_frame(tags=(t0, t1), tpids=[pg.ETH_VLAN, pg.ETH_QINQ], size=68))
        F.append(pg.udp4_frame(tags=(t0,), size=64))
        F.append(pg.udp4_frame(tags=(t0,), tpids=[pg.ETH_QINQ], size=64))
    for ihl in range(0, 16):
        opts = bytes([1]) * (4 * max(0, ihl - 5))
        h = bytearray(pg.ipv4(options=opts, payload_len=8))
        h[0] = 0x40 | ihl
        F.append(pg.pad_to(E + bytes(h) + pg.udp(1024, 2048), 100))
    for hl in range(0, 16):
        F.append(pg.pad_to(E + pg.ipv4(proto=6, payload_len=40) + pg.tcp(1024, 2048, hl=hl) + bytes(20), 80))
    for ulen in (0, 7, 8, 9, 26, 27, 0xFFFF):
        F.append(pg.pad_to(E + pg.ipv4(payload_len=26) + pg.udp(1024, 2048, ulen, bytes(18)), 60))
    for plen in (0, 7, 8, 9, 15, 16, 17, 24, 66, 67):
        F.append(pg.pad_to(E6 + pg.ipv6(next_hdr=0, payload_len=plen) + pg.ipv6_ext(pg.IPPROTO_UDP, 0) +
                           pg.udp(1024, 2048, 8), 120))
        F.append(pg.pad_to(E6 + pg.ipv6(next_hdr=17, payload_len=plen) + pg.udp(1024, 2048, 8), 120))
    return tuple(F)


def edge_program():
    """Rules over what the edge frames vary, an error CoS, marks, a hash CoS."""
    return [R.cos("default", queue=1), R.cos("err", queue=2), R.cos("vidx", queue=3), R.cos("vid0", queue=4),
            R.cos("udp", num_queue=5, hash_proto=R.HP_IPV4 | R.HP_IPV6 | R.HP_IPV4_UDP | R.HP_IPV6_UDP),
            R.cos("tcp", queue=6, stats=1), R.cos("pcp", queue=7), R.cos("ethx", queue=8),
            ("default", 0), ("error", 1),
            ("pmr", [R.t_be16(R.PMR_VLAN_ID_X, 0x456)], 0, 2, 1),
            ("pmr", [R.t_be16(R.PMR_VLAN_ID_0, 0x123)], 0, 3, 2),
            ("pmr", [R.t_u8(R.PMR_VLAN_PCP_0, 7)], 0, 6, 3),
            ("pmr", [R.t_be16(R.PMR_ETHTYPE_X, pg.ETH_VLAN)], 0, 7, 4),
            ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 2048)], 0, 4, 5),
            ("pmr", [R.t_be16(R.PMR_TCP_SPORT, 1024)], 0, 5, 6),
            ("pmr", [R.t_be16(R.PMR_UDP_SPORT, 1024)], 2, 4, 7),
            ("pmr", [R.t_be16(R.PMR_VLAN_ID_X, 0x123, 0x0FFF)], 3, 2, 8)]


@functools.lru_cache(maxsize=4)
def fuzz_case(seed, dense=False):
    """(program, frames) of one fuzz seed: the zoo plus 3000 mutations, a
    random program inside the reference's limits (8..64 CoS with 3 PMRs per
    CoS on average; dense: 4..9 CoS with 10, so that the CoS packets do reach
    carry full rule lists, creates past the 8th are refused and chains go
    deeper), deletes on, the term vocabulary alternately unlimited and 6
    kinds."""
    rng = np.random.default_rng((9000 if dense else 7000) + seed)
    base = list(zoo_frames())
    frames = base + zoo.mutate_frames(rng, base, 3000)
    n_cos = int(rng.integers(4, 10)) if dense else int(rng.integers(8, 65))
    n_rules = int(min(256, (10 if dense else 3) * (n_cos - 1)))
    prog = zoo.random_program(rng, base, n_cos=n_cos, n_rules=n_rules, with_deletes=True,
                              max_kinds=None if seed % 2 == 0 else 6)
    return defined_hashing(prog), frames


def defined_hashing(prog):
    """The program with every hash CoS that hashes ports also hashing the
    addresses of both IP versions.  Left out on purpose: ports without the
    packet's addresses make packet_rss_hash hash an uninitialised tuple word
    (odp_classification.c:1787-1811, undefined in the reference; DESIGN.md
    "Oracle", deviation "Hashing L4 without L3": we hash zero)."""
    l4 = R.HP_IPV4_UDP | R.HP_IPV4_TCP | R.HP_IPV6_UDP | R.HP_IPV6_TCP
    out = []
    for op in prog:
        if op[0] == "cos" and op[2]["num_queue"] > 1 and op[2]["hash_proto"] & l4:
            op = (op[0], op[1], dict(op[2], hash_proto=op[2]["hash_proto"] | R.HP_IPV4 | R.HP_IPV6))
        out.append(op)
    return out


@functools.lru_cache(maxsize=2)
def chksum_corpus(seed=21):
    """The checksum corpus of tests/test_gpu_chksum.py: valid and corrupted
    frames, the zoo, 1500 mutations of both."""
    rng = np.random.default_rng(seed)
    base = list(zoo_frames())
    fr = [f for f, _, _ in CK.frame_set(seed=seed, n=300)]
    return fr + base + zoo.mutate_frames(rng, base + fr, 1500)


def valid_chksum_batch(ipver, proto):
    """Valid L4 checksums (pktgen.set_checksums) at every L4 length 12..395
    (never shorter than the protocol's own header), then one byte flipped
    anywhere in every third frame."""
    rng = np.random.default_rng(300 + 10 * ipver + proto)
    l4 = 14 + (20 if ipver == 4 else 40)
    lens = np.arange(l4 + 12, l4 + 396)
    n = lens.size
    kw = dict(sip4=rng.integers(0, 2**32, n).astype(np.uint64),
              dip4=rng.integers(0, 2**32, n).astype(np.uint64)) if ipver == 4 else dict(
        sip6=rng.integers(0, 256, (n, 16), dtype=np.uint8),
        dip6=rng.integers(0, 256, (n, 16), dtype=np.uint8))
    b = pg.build_batch(lens, ipver=np.full(n, ipver), l4proto=np.full(n, proto),
                       sport=rng.integers(1, 65535, n), dport=rng.integers(1, 65535, n), seed=13, **kw)
    pg.set_checksums(b)
    for i in range(0, n, 3):
        b.buf[int(b.off[i]) + int(rng.integers(0, int(b.len[i])))] ^= 1 << int(rng.integers(0, 8))
    return b


# ---------------------------------------------------------- odp_packet_parse
def ref_parse_records(frames, offsets, proto, layer, chksums):
    """The reference's odp_packet_parse as the record mi_cls_parse writes
    (parse_model.records): offsets relative to the parse start."""
    from oracle import reflib
    out = np.zeros(len(frames), R.RESULT_DTYPE)
    for i, (f, o) in enumerate(zip(frames, offsets)):
        p = reflib.packet_parse(f, o, proto, layer, chksums)
        out["in_flags"][i], out["err"][i] = p.in_flags, p.err
        out["outcome"][i] = R.OUT_PARSE_DROP if p.ret else R.OUT_ENQ
        out["l3_offset"][i] = p.l3 - o if p.l3 != PM.INVALID else PM.INVALID
        out["l4_offset"][i] = p.l4 - o if p.l4 != PM.INVALID else PM.INVALID
    return out


@functools.lru_cache(maxsize=2)
def parse_frames(n_mut, seed=5):
    """The non-empty zoo frames, n_mut mutations of them, the edge frames."""
    rng = np.random.default_rng(seed)
    base = list(zoo_frames())
    return tuple(f for f in base + zoo.mutate_frames(rng, base, n_mut) + list(edge_frames()) if len(f) > 0)
