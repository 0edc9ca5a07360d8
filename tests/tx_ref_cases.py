"""The transmit corpus and the one statement of how a transmit result is
compared with the reference's own compiled code (oracle/_ref/libodp_ref.so:
loopback_fix_checksums and get_dest_queue of pktio/loop.c behind
oracle/ref_loop_shim.c).  Test infrastructure, used by the CPU tests
(tests/test_tx_vs_reference.py: the models) and the GPU tests
(tests/test_gpu_tx_vs_reference.py: the kernels, no model in between).

The corpus is seeded and deterministic.  A case is (frame, l3, l4, flags,
group): what a mi_cls_tx_desc_t says about one frame -- flags holds the four
checksum override bits (low) and the four metadata bits of the flow hash
(high) -- and the name of the group it was built for.
"""
import struct
from collections import Counter, namedtuple

import numpy as np

from odp_amd import pktgen as pg
from tests import chksum_frames as CK
from tests import tx_model as TX
from tests import txq_model as TQ

Case = namedtuple("Case", "frame l3 l4 flags group")

INVALID = 0xFFFF
UDP, TCP, SCTP = pg.IPPROTO_UDP, pg.IPPROTO_TCP, pg.IPPROTO_SCTP
KINDS = [(4, UDP), (4, TCP), (4, SCTP), (6, UDP), (6, TCP), (6, SCTP)]
L4_HDR = {UDP: 8, TCP: 20, SCTP: 12}

# pktout option rows (the option word of mi_cls_chksum_insert; the reference
# is given TX.all_bits() of it): nothing, each single default, all four, the
# _ena bits alone (never consulted on transmit), every bit
OPT_ROWS = (0, TX.CK_IPV4, TX.CK_UDP, TX.CK_TCP, TX.CK_SCTP, TX.ALL_TX, TX.ALL_ENA, 0xFF)
# hash_proto rows for the whole corpus; all 64 values go over HASH_SLICE cases
HP_ROWS = (0, 63, 1, 2, 4, 8, 16, 32)
HASH_SLICE = 200
MODULI = (64, 63, 61, 59, 55, 53)

# the floor of every group (asserted by cases())
FLOORS = {"valid": 400, "lengths": 1806, "long": 12, "fill": 24, "padded": 276, "udp_len": 40,
          "udp_zero": 8, "ihl": 100, "frag": 18, "fit": 40, "moved": 48, "odd_l3": 150, "invalid": 18,
          "meta16": 144, "cut": 16, "overrides": 384, "deviation": 60}


# ------------------------------------------------------------------ builders
def natural_meta(frame: bytes, l3: int, l4: int) -> int:
    """The metadata bits a parse of a well-formed frame would give: the IP
    version at l3 and UDP / TCP by the protocol byte in front of l4."""
    if l3 == INVALID or l3 >= len(frame):
        return 0
    ver = frame[l3] >> 4
    if ver == 4 and l3 + 20 <= len(frame):
        m, proto = TQ.F_IPV4, frame[l3 + 9]
    elif ver == 6 and l3 + 40 <= len(frame):
        m, proto = TQ.F_IPV6, frame[l3 + 6]
    else:
        return 0
    return m | (TQ.F_UDP if proto == UDP else TQ.F_TCP if proto == TCP else 0)


def _case(group, frame, l3, l4, low=0, meta=None):
    if meta is None:
        meta = natural_meta(frame, l3, l4)
    return Case(bytes(frame), l3, l4, (low & 0xF) | meta, group)


def _rand(rng, n):
    return bytes(rng.integers(0, 256, n).astype(np.uint8))


def _scrambled(rng, ver, proto, payload, **kw):
    fr, l3, l4 = CK.build(rng, ver, proto, payload=payload, **kw)
    return TX.scramble(fr, l3, l4, seed=int(rng.integers(0, 256))), l3, l4


def _with_options(frame, l3, nopt, rng):
    """The IPv4 frame with nopt random non-zero option dwords spliced in."""
    opts = bytes(b | 1 for b in _rand(rng, 4 * nopt))
    b = bytearray(frame[:l3 + 20] + opts + frame[l3 + 20:])
    b[l3] = 0x40 | (5 + nopt)
    struct.pack_into("!H", b, l3 + 2, len(b) - l3)
    return bytes(b)


def _edit(frame, at, data):
    b = bytearray(frame)
    b[at:at + len(data)] = data
    return bytes(b)


def solve_udp_zero(frame: bytes, l3: int, l4: int, at: int) -> bytes:
    """The UDP frame with the 16-bit word at `at` (an even distance behind l4,
    inside the payload) solved so that the computed checksum is 0: the folded
    sum of pseudo header and datagram, checksum field zero, is 0xFFFF."""
    assert (at - l4) % 2 == 0 and l4 + 8 <= at and at + 2 <= len(frame)
    b = bytearray(frame)
    b[l4 + 6:l4 + 8] = b"\x00\x00"
    b[at:at + 2] = b"\x00\x00"
    addrs = bytes(b[l3 + 12:l3 + 20]) if b[l3] >> 4 == 4 else bytes(b[l3 + 8:l3 + 40])
    s = CK.ones_sum(struct.pack("!H", CK.ones_sum(addrs)) + bytes([0, 17]) + bytes(b[l4 + 4:l4 + 6]) +
                    struct.pack("!H", CK.ones_sum(bytes(b[l4:]))))
    struct.pack_into("!H", b, at, 0xFFFF - s)
    b[l4 + 6:l4 + 8] = b"\x5a\xa5"      # garbage in the field, as everywhere
    return bytes(b)


def _other(rng, kind, front=0):
    """ICMP over IPv4 / IPv6 and ARP: frames with no L4 checksum to insert."""
    if kind == "arp":
        fr = bytes(pg.eth(ethtype=0x0806)) + _rand(rng, 28) + bytes(18)
        return b"\xa5" * front + fr, 14 + front, INVALID
    ver = 4 if kind == "icmp4" else 6
    body = pg.icmp() + _rand(rng, 24)
    e = pg.eth(ethtype=pg.ETH_IPV4 if ver == 4 else pg.ETH_IPV6)
    ip = (pg.ipv4(src=_rand(rng, 4), dst=_rand(rng, 4), proto=1, payload_len=len(body)) if ver == 4 else
          pg.ipv6(src=_rand(rng, 16), dst=_rand(rng, 16), next_hdr=58, payload_len=len(body)))
    return b"\xa5" * front + bytes(e) + bytes(ip) + body, 14 + front, 14 + front + len(ip)


# -------------------------------------------------------------------- corpus
_cache = {}


def cases():
    """The whole corpus, built once."""
    if "cases" in _cache:
        return _cache["cases"]
    rng = np.random.default_rng(0x7C5)
    out = []

    # ---- scrambled valid frames
    for fr, _ in TX.valid_frames():
        l3, l4 = TX.offsets_of(fr)
        out.append(_case("valid", TX.scramble(fr, l3, l4), l3, l4))
    for ver, proto in KINDS:                       # every L4 length: header .. header + 300
        for k in range(301):
            out.append(_case("lengths", *_scrambled(rng, ver, proto, _rand(rng, k))))
    for ver, proto in KINDS:
        for total in (1500, 9000):
            fr0, _, _ = CK.build(rng, ver, proto, payload=b"")
            fr, l3, l4 = _scrambled(rng, ver, proto, _rand(rng, total - len(fr0)))
            assert len(fr) == total
            out.append(_case("long", fr, l3, l4))
    for ver, proto in KINDS:
        for fill in (0x00, 0xFF):
            for k in (37, 128):
                out.append(_case("fill", *_scrambled(rng, ver, proto, bytes([fill]) * k)))

    # ---- padded: 1 .. 46 non-zero bytes behind the IP datagram
    for ver, proto in KINDS:
        for pad in range(1, 47):
            fr, l3, l4 = _scrambled(rng, ver, proto, _rand(rng, int(rng.integers(0, 24))))
            out.append(_case("padded", fr + bytes(b | 1 for b in _rand(rng, pad)), l3, l4))

    # ---- the UDP length field: shorter, longer, 0, odd
    for ver in (4, 6):
        for k in (0, 1, 22, 75):
            fr, l3, l4 = _scrambled(rng, ver, UDP, _rand(rng, k))
            for v in (8, 8 + k - 1 if k else 7, 8 + k + 5, 0, 9, 0xFFFF, 8 + k + 1):
                out.append(_case("udp_len", _edit(fr, l4 + 4, struct.pack("!H", v & 0xFFFF)), l3, l4))

    # ---- a computed UDP checksum of 0 (stored as 0xFFFF)
    for ver in (4, 6):
        for k, back in ((2, 2), (16, 2), (33, 3), (64, 40), (131, 1 + 64)):
            fr, l3, l4 = CK.build(rng, ver, UDP, payload=_rand(rng, k))
            at = len(fr) - back - ((len(fr) - back - l4) & 1)
            out.append(_case("udp_zero", solve_udp_zero(fr, l3, l4, at), l3, l4))

    # ---- the IPv4 header: IHL 0 .. 15
    for proto in (UDP, TCP, SCTP):
        for ihl in range(16):
            # the header really has that many dwords (below 5: only the nibble
            # says so), l4 behind it; the frame holds it, or ends inside it
            fr, l3, l4 = _scrambled(rng, 4, proto, _rand(rng, 30))
            if ihl > 5:
                fr, l4 = _with_options(fr, l3, ihl - 5, rng), l4 + 4 * (ihl - 5)
            else:
                fr = _edit(fr, l3, bytes([0x40 | ihl]))
            out.append(_case("ihl", fr, l3, l4))
            if ihl > 5:
                out.append(_case("ihl", fr[:l3 + 4 * ihl - 1], l3, l3 + 20))   # the header runs past the end
            # only the nibble changed on a 20-byte header: l4 = l3 + 20 lies
            # inside what IHL calls the header; a long and a short frame
            for k in (60, 4):
                fr, l3, l4 = _scrambled(rng, 4, proto, _rand(rng, k))
                c = _case("ihl", _edit(fr, l3, bytes([0x40 | ihl])), l3, l4)
                if tcp_exchange_ok(c):
                    out.append(c)
    # fragments: MF, an offset, both, the largest offset; DF / reserved are none
    for proto in (UDP, TCP, SCTP):
        for frag in (0x2000, 0x0005, 0x2005, 0x1FFF, 0x3FFF, 0x4000, 0x8000, 0xC000):
            fr, l3, l4 = _scrambled(rng, 4, proto, _rand(rng, 26))
            out.append(_case("frag", _edit(fr, l3 + 6, struct.pack("!H", frag)), l3, l4))

    # ---- headers that just fit or just do not
    for ver, proto in KINDS:
        fr, l3, l4 = _scrambled(rng, ver, proto, _rand(rng, 40))
        for nib in (0, 5, 7, 15, 10 - ver):         # not 4 / 6, and the other version
            out.append(_case("fit", _edit(fr, l3, bytes([(nib << 4) | (fr[l3] & 0xF)])), l3, l4))
        for rem in (19, 20, 39, 40):
            if rem >= (20 if ver == 4 else 40) or l4 == INVALID:
                out.append(_case("fit", fr[:l3 + rem], l3, l4))
            else:                                   # l4 behind the frame's end: no IP header there either
                out.append(_case("fit", fr[:l3 + rem], l3, l4, meta=TQ.F_IPV4 if ver == 4 else TQ.F_IPV6))
    for nh in (0, 43, 60, 44):                      # an IPv6 extension header in front of UDP
        fr, l3, l4 = CK.build(rng, 6, UDP, payload=_rand(rng, 20))
        ext = bytes([UDP, 0]) + bytes(b | 1 for b in _rand(rng, 6))
        b = bytearray(fr[:l4] + ext + fr[l4:])
        b[l3 + 6] = nh
        struct.pack_into("!H", b, l3 + 4, len(b) - l3 - 40)
        out.append(_case("fit", TX.scramble(bytes(b), l3, l4 + 8), l3, l4 + 8, meta=TQ.F_IPV6 | TQ.F_UDP))
        out.append(_case("fit", TX.scramble(bytes(b), l3, l4 + 8), l3, l4 + 8, meta=TQ.F_IPV6))

    # ---- metadata that contradicts the bytes
    for ver, proto in KINDS:                        # offsets moved (l4 moved down: see "deviation")
        for ipopt in (False, ver == 4):
            fr, l3, l4 = _scrambled(rng, ver, proto, _rand(rng, 44), ipopt=ipopt)
            m = natural_meta(fr, l3, l4)
            for d3, d4 in ((2, 0), (4, 0), (-2, 0), (-4, 0), (0, 2), (0, 4), (2, 2), (-4, -4)):
                out.append(_case("moved", fr, l3 + d3, l4 + d4, meta=m))
    src = [c for c in out if c.group in ("valid", "lengths")]
    for c in src[::len(src) // 160][:160]:          # a 15-byte L2: l3 and l4 odd
        out.append(Case(b"\xa5" + c.frame, c.l3 + 1, c.l4 + 1, c.flags, "odd_l3"))
    for ver, proto in KINDS:
        fr, l3, l4 = _scrambled(rng, ver, proto, _rand(rng, 33))
        m = natural_meta(fr, l3, l4)
        out += [_case("invalid", fr, INVALID, l4, meta=m), _case("invalid", fr, l3, INVALID, meta=m),
                _case("invalid", fr, INVALID, INVALID, meta=m)]
    others = []
    for ver, proto in KINDS:
        others.append(_scrambled(rng, ver, proto, _rand(rng, 28)))
    others += [_other(rng, "icmp4"), _other(rng, "icmp6", front=1), _other(rng, "arp")]
    for fr, l3, l4 in others:                       # all 16 combinations of the four metadata flags
        for m in range(16):
            out.append(_case("meta16", fr, l3, l4, meta=m << 4))
    for ver in (4, 6):                              # L4 / L3 headers one byte short, and just fitting
        fr, l3, l4 = _scrambled(rng, ver, UDP, _rand(rng, 30))
        m = natural_meta(fr, l3, l4)
        out += [_case("cut", fr[:l4 + 8], l3, l4, meta=m), _case("cut", fr[:l4 + 8], l3, l4, meta=m | TQ.F_TCP),
                _case("cut", fr[:l3 + (20 if ver == 4 else 40)], l3, INVALID, meta=m),
                _case("cut", fr[:l3 + (19 if ver == 4 else 39)], l3, INVALID, meta=m)]
        fr, l3, l4 = _scrambled(rng, ver, TCP, _rand(rng, 30))
        m = natural_meta(fr, l3, l4)
        out += [_case("cut", fr[:l4 + 20], l3, l4, meta=m), _case("cut", fr[:l4 + 19], l3, l4, meta=m),
                _case("cut", fr[:l4 + 19], l3, l4, meta=m | TQ.F_UDP),
                _case("cut", fr[:l4 + 18], l3, l4, meta=m)]

    # ---- all 16 values of the four override bits
    for ver, proto in KINDS:
        for k in (0, 9, 30, 101):
            fr, l3, l4 = _scrambled(rng, ver, proto, _rand(rng, k))
            for low in range(16):
                out.append(_case("overrides", fr, l3, l4, low=low))

    # ---- the documented deviations, built on purpose and
    # kept apart: l4 - l3 odd or below the fixed IP header, the checksum field
    # not inside the frame.  The field the reference writes stays clear of the
    # IPv4 header checksum (l4 - l3 > 5), see expected().
    for ver, proto in KINDS:
        fr, l3, l4 = _scrambled(rng, ver, proto, _rand(rng, 36))
        m = natural_meta(fr, l3, l4)
        fixed = 20 if ver == 4 else 40
        for d in (1, 3, -1):
            out.append(_case("deviation", fr, l3, l4 + d, meta=m))
        for at in (fixed - 2, fixed - 4, 8, 12):
            out.append(_case("deviation", fr, l3, l3 + at, meta=m))
        for cut in ({UDP: (7, 6, 3), TCP: (17, 16, 12, 8, 7, 0), SCTP: (11, 10, 8, 1)}[proto]):
            out.append(_case("deviation", fr[:l4 + cut], l3, l4, meta=m))
        for low in (TX.L4_SET | TX.L4_CK, TX.L4_SET):          # the override asks for it / forbids it
            out.append(_case("deviation", fr, l3, l4 + 1, low=low, meta=m))

    # ---- what the corpus must hold
    n = Counter(c.group for c in out)
    for g, floor in FLOORS.items():
        assert n[g] >= floor, (g, n[g], floor)
    assert set(n) == set(FLOORS)
    assert 3000 <= len(out) <= 6000, len(out)
    for c in out:
        assert len(c.frame) <= 0xFFFF and ref_defined(c), c
    v4len = {p: {len(c.frame) for c in out if c.group == "lengths" and c.frame[c.l3] >> 4 == 4 and
                 c.frame[c.l3 + 9] == p} for p in (UDP, TCP, SCTP)}
    for p in (UDP, TCP, SCTP):
        assert {63, 64, 65, 127, 128, 129} <= v4len[p]
    dev = sum(1 for c in out if deviation(c) is not None)
    assert dev * 10 <= len(out), (dev, len(out))
    assert all(deviation(c) is None or c.group in ("deviation", "moved", "cut", "ihl", "fit") for c in out)
    assert all(tcp_exchange_ok(c) for c in out)
    _cache["cases"] = out
    return out


def hash_slice():
    """HASH_SLICE cases spread over every group, for the 64 hash_proto values."""
    cs = cases()
    return cs[::max(1, len(cs) // HASH_SLICE)][:HASH_SLICE]


def golden_slice(n=300, max_len=200):
    """About n short cases drawn from every group, for tests/golden/tx_reference.json."""
    by = {}
    for i, c in enumerate(cases()):
        if len(c.frame) <= max_len:
            by.setdefault(c.group, []).append(i)
    pick = []
    per = max(4, n // len(by))
    for g in FLOORS:
        if g not in by:     # "long": its two shortest frames
            idx = sorted((i for i, c in enumerate(cases()) if c.group == g), key=lambda i: len(cases()[i].frame))
            pick += idx[:2]
            continue
        idx = by[g]
        pick += idx[::max(1, len(idx) // per) | 1][:per]    # an odd step: every flag combination comes up
    return sorted(pick)


# ------------------------------------------------------------ the comparison
def ip_info(frame: bytes, l3: int):
    """(is IPv4, L4 protocol) as the IP header at l3 says -- 255 for an IPv4
    fragment -- or None where there is no IPv4 / IPv6 header in the frame."""
    if l3 == INVALID or l3 >= len(frame):
        return None
    ver, rem = frame[l3] >> 4, len(frame) - l3
    if ver == 4 and rem >= 20:
        frag = struct.unpack_from("!H", frame, l3 + 6)[0] & 0x3FFF
        return True, 255 if frag else frame[l3 + 9]
    if ver == 6 and rem >= 40:
        return False, frame[l3 + 6]
    return None


def deviation(c):
    """Which documented deviation ("Insertion on frames outside
    the contract") applies to the L4 checksum of this case -- "odd", "below",
    "field" -- or None.  Decided from (len, l3, l4, the IP header's protocol)
    alone, never from either side's output."""
    info = ip_info(c.frame, c.l3)
    if info is None or info[1] not in L4_HDR or c.l4 == INVALID:
        return None
    v4, proto = info
    if (c.l4 - c.l3) % 2:
        return "odd"
    if c.l4 < c.l3 + (20 if v4 else 40):
        return "below"
    at, size = {UDP: (6, 2), TCP: (16, 2), SCTP: (8, 4)}[proto]
    if c.l4 + at + size > len(c.frame):
        return "field"
    return None


def ref_defined(c):
    """False where the reference itself runs out of bounds: an L4 checksum
    with l4 behind the frame's end (frame_len - l4 wraps, odp_packet.c
    :2002-2003).  No case may be such."""
    info = ip_info(c.frame, c.l3)
    return info is None or info[1] not in L4_HDR or c.l4 == INVALID or c.l4 <= len(c.frame)


def _tcp_exchange(c):
    info = ip_info(c.frame, c.l3)
    return info is not None and info[1] == TCP and c.l4 != INVALID and deviation(c) is None


def tcp_exchange_ok(c):
    """The exchange of expected() moves two words: an IPv4 header sum must
    hold both or neither (l4 inside a long options field can split them)."""
    if not _tcp_exchange(c) or c.frame[c.l3] >> 4 != 4:
        return True
    ihl = c.frame[c.l3] & 0xF
    end = c.l3 + 4 * ihl
    return ihl < 5 or end > len(c.frame) or end <= c.l4 + 6 or end >= c.l4 + 18


def _swap(frame: bytes, l4: int) -> bytes:
    b = bytearray(frame)
    b[l4 + 6:l4 + 8], b[l4 + 16:l4 + 18] = b[l4 + 16:l4 + 18], b[l4 + 6:l4 + 8]
    return bytes(b)


def ref_input(c) -> bytes:
    """The frame as it is given to the reference (see expected())."""
    return _swap(c.frame, c.l4) if _tcp_exchange(c) else c.frame


def ref_output(c, out: bytes) -> bytes:
    """The reference's output frame in this project's layout."""
    return _swap(out, c.l4) if _tcp_exchange(c) else out


def l4_wanted(c, opt):
    """Does the configuration ask for this case's L4 checksum?  From the
    inputs alone (override bits, option word, the IP header's protocol)."""
    info = ip_info(c.frame, c.l3)
    if info is None or info[1] not in L4_HDR:
        return False
    cfg = {UDP: TX.CK_UDP, TCP: TX.CK_TCP, SCTP: TX.CK_SCTP}[info[1]]
    return bool(c.flags & TX.L4_CK if c.flags & TX.L4_SET else opt & cfg)


def expected(c, ref_out: bytes):
    """What this project must produce for a case, from the reference's
    output frame (`ref_out`: ref_output() of what the reference made of
    ref_input()); returns (bytes, masked deviation or None).

    In contract: every byte equals the reference's.  The TCP checksum, which
    the reference stores at l4 + 6 inside the sequence number and this
    project at l4 + 16, is still compared exactly, not masked: the reference
    is given the frame with the 16-bit words at l4 + 6 and l4 + 16 exchanged,
    and they are exchanged back in its output.  Both offsets are even
    relative to l3, so the one's-complement sum does not see the exchange:
    the word the reference stores must equal ours, and every other byte must
    match.

    A deviation case (deviation(): decided from the inputs alone): this
    project leaves the L4 field of the affected protocol unchanged, so the
    bytes the reference's insertion writes (2 at l4 + 6 for UDP and TCP, 4 at
    l4 + 8 for SCTP, as far as the frame holds them) are expected as they
    were in the input; the rest of the frame -- the IPv4 header checksum and
    everything outside that field -- is the reference's."""
    kind = deviation(c)
    if kind is None:
        return ref_out, None
    proto = ip_info(c.frame, c.l3)[1]
    lo = c.l4 + (8 if proto == SCTP else 6)
    hi = min(len(c.frame), lo + (4 if proto == SCTP else 2))
    lo = min(lo, hi)
    if c.frame[c.l3] >> 4 == 4:
        assert hi <= c.l3 + 10 or lo >= c.l3 + 12, "the masked field may not overlap the IPv4 header checksum"
    return ref_out[:lo] + c.frame[lo:hi] + ref_out[hi:], kind


class Tally:
    """Counts the comparisons and the masked (case, protocol) pairs."""

    def __init__(self):
        self.compared = 0
        self.masked = Counter()

    def check(self):
        """At most 10 % masked, each of the three deviations at least 8 times."""
        total = sum(self.masked.values())
        assert total * 10 <= self.compared, (total, self.compared)
        for kind in ("odd", "below", "field"):
            assert self.masked[kind] >= 8, (kind, dict(self.masked))


def assert_same_tx(got: bytes, c, opt, who, ref_out: bytes, tally=None):
    """`got` (the frame as `who` left it) against the reference's answer for
    case c under option word opt, by the rules of expected()."""
    exp, kind = expected(c, ref_out)
    if tally is not None:
        tally.compared += 1
        if kind is not None and l4_wanted(c, opt):
            tally.masked[kind] += 1
    if got != exp:
        bad = [i for i in range(len(exp)) if got[i] != exp[i]]
        raise AssertionError(f"{who}: opt {opt:#x} group {c.group} len {len(c.frame)} l3 {c.l3} l4 {c.l4} "
                             f"flags {c.flags:#x} deviation {kind}: bytes {bad[:8]} differ, "
                             f"got {bytes(got[i] for i in bad[:8]).hex()} "
                             f"reference {bytes(exp[i] for i in bad[:8]).hex()}; frame {c.frame[:96].hex()}")


def ref_fix(cs, opt):
    """The reference's output frame of every case under option word opt, in
    this project's layout (ref_output), from the live library in one call."""
    from oracle import reflib
    b = pg.batch_from_frames([ref_input(c) for c in cs])
    desc = TX.make_desc([c.l3 for c in cs], [c.l4 for c in cs], np.array([c.flags for c in cs], np.uint8))
    out = reflib.tx_fix_checksums(b.buf, b.off, b.len, desc, TX.all_bits(opt))
    return [ref_output(c, o) for c, o in zip(cs, frames_of(b, out))]


def ref_queues(cs, hash_proto, frames=None, index=0):
    """get_dest_queue's queue index of every case for num_qs = each of
    MODULI, (n, 6); frames: other bytes for the same descriptors (the frames
    as a checksum insertion left them)."""
    from oracle import reflib
    assert tuple(reflib.TX_MODULI) == MODULI
    b = pg.batch_from_frames([c.frame for c in cs] if frames is None else list(frames))
    desc = TX.make_desc([c.l3 for c in cs], [c.l4 for c in cs], np.array([c.flags for c in cs], np.uint8))
    return reflib.tx_dest_queues(b.buf, b.off, b.len, desc, hash_proto, index)


def residues(h):
    """h % each of MODULI, shaped like reflib.tx_dest_queues' result."""
    h = np.asarray(h, np.uint64)
    return (h[:, None] % np.array(MODULI, np.uint64)[None, :]).astype(np.uint8)


# ------------------------------------------------------------------- batches
def batch_of(cs, unaligned_seed=None):
    """(pg.Batch, descriptors) of cases: packed at 64-B slots, or at arbitrary
    byte offsets."""
    frames = [c.frame for c in cs]
    desc = TX.make_desc([c.l3 for c in cs], [c.l4 for c in cs], np.array([c.flags for c in cs], np.uint8))
    if unaligned_seed is None:
        return pg.batch_from_frames(frames), desc
    rng = np.random.default_rng(unaligned_seed)
    off, pos = [], 1
    for f in frames:
        off.append(pos)
        pos += len(f) + int(rng.integers(0, 40))
    buf = np.zeros(pos + 64, np.uint8)
    for o, f in zip(off, frames):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return pg.Batch(buf, np.array(off, np.uint32), np.array([len(f) for f in frames], np.uint16)), desc


def frames_of(b, buf=None):
    buf = b.buf if buf is None else buf
    return [bytes(buf[int(o):int(o) + int(n)]) for o, n in zip(b.off, b.len)]
