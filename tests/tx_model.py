"""Pure-Python statement of the pktout checksum insertion rules.

Test infrastructure: what a loop pktio does to a packet on transmit
(reference pktio/loop.c:386-472 loopback_fix_checksums and odp_packet.c:
1888-2063 _odp_packet_{ipv4,udp,tcp,sctp}_chksum_insert), with the one
deliberate deviation of this project: the TCP checksum is stored at l4 + 16
(the reference stores it at l4 + 6, odp_packet.c:1988).  The GPU kernel
(mi_cls_tx_kernel) is compared with this model byte for byte.
"""
import struct

import numpy as np

from tests import chksum_frames as CK

# The option word of mi_cls_chksum_insert: odp_pktout_config_opt_t.all_bits
# (include/odp_rt.h) without its bit 0, ts_ena
ENA_IPV4, ENA_UDP, ENA_TCP, ENA_SCTP = 1 << 0, 1 << 1, 1 << 2, 1 << 3
CK_IPV4, CK_UDP, CK_TCP, CK_SCTP = 1 << 4, 1 << 5, 1 << 6, 1 << 7
ALL_TX = CK_IPV4 | CK_UDP | CK_TCP | CK_SCTP
ALL_ENA = ENA_IPV4 | ENA_UDP | ENA_TCP | ENA_SCTP
TS_ENA = 1      # all_bits bit 0: not a checksum option, not offered


def all_bits(opt: int) -> int:
    """odp_pktout_config_opt_t.all_bits of an option word: what a pktio is
    configured with and what the reference's loopback_fix_checksums reads
    (ipv4_chksum is bit 5 there)."""
    return opt << 1

# mi_cls_tx_desc_t.flags
L3_SET, L3_CK, L4_SET, L4_CK = 1, 2, 4, 8
# done bits (MI_CLS_TX_*)
DONE_IPV4, DONE_UDP, DONE_TCP, DONE_SCTP = 1, 2, 4, 8

INVALID = 0xFFFF

DESC_DTYPE = np.dtype([("l3", "<u2"), ("l4", "<u2"), ("flags", "u1"), ("rsv", "u1", (3,))])
assert DESC_DTYPE.itemsize == 8


def _want(ovr_set, ovr, cfg):
    return bool(ovr if ovr_set else cfg)


def insert(frame: bytes, l3: int, l4: int, flags: int, opt: int):
    """Returns (new frame bytes, done bits)."""
    b = bytearray(frame)
    n = len(b)
    if l3 == INVALID or l3 >= n:
        return bytes(b), 0
    ver = b[l3] >> 4
    if ver == 4 and n - l3 >= 20:
        v4 = True
        proto = b[l3 + 9]
        if struct.unpack_from("!H", b, l3 + 6)[0] & 0x3FFF:
            proto = 255
    elif ver == 6 and n - l3 >= 40:
        v4 = False
        proto = b[l3 + 6]
    else:
        return bytes(b), 0
    w_ip = v4 and _want(flags & L3_SET, flags & L3_CK, opt & CK_IPV4)
    w_tcp = proto == 6 and _want(flags & L4_SET, flags & L4_CK, opt & CK_TCP)
    w_udp = proto == 17 and _want(flags & L4_SET, flags & L4_CK, opt & CK_UDP)
    w_sctp = proto == 132 and _want(flags & L4_SET, flags & L4_CK, opt & CK_SCTP)
    done = 0
    if w_ip:
        ihl = b[l3] & 0xF
        if ihl >= 5 and l3 + 4 * ihl <= n:
            b[l3 + 10:l3 + 12] = b"\x00\x00"
            struct.pack_into("!H", b, l3 + 10, CK.inet_csum(bytes(b[l3:l3 + 4 * ihl])))
            done |= DONE_IPV4
    # contract: l4 valid, l4 - l3 even and at least the fixed IP header
    l4_ok = l4 != INVALID and l4 >= l3 + (20 if v4 else 40) and (l4 - l3) % 2 == 0
    if (w_tcp or w_udp) and l4_ok:
        fo = l4 + (16 if w_tcp else 6)
        if fo + 2 <= n:
            addrs = bytes(b[l3 + 12:l3 + 20]) if v4 else bytes(b[l3 + 8:l3 + 40])
            if w_tcp:
                plen = struct.pack("!H", (n - l4) & 0xFFFF)
            else:
                plen = bytes(b[l4 + 4:l4 + 6])      # the length field as stored
            b[fo:fo + 2] = b"\x00\x00"
            s = CK.ones_sum(addrs) + CK.ones_sum(bytes([0, 6 if w_tcp else 17]) + plen) + \
                CK.ones_sum(bytes(b[l4:n]))
            c = (~CK.ones_sum(struct.pack("!HH", s >> 16, s & 0xFFFF))) & 0xFFFF
            if w_udp and c == 0:
                c = 0xFFFF
            struct.pack_into("!H", b, fo, c)
            done |= DONE_TCP if w_tcp else DONE_UDP
    if w_sctp and l4_ok and l4 + 12 <= n:
        b[l4 + 8:l4 + 12] = b"\x00\x00\x00\x00"
        crc = (~CK.crc32c(bytes(b[l4:n]))) & 0xFFFFFFFF
        struct.pack_into("<I", b, l4 + 8, crc)
        done |= DONE_SCTP
    return bytes(b), done


def make_desc(l3s, l4s, flags):
    d = np.zeros(len(l3s), DESC_DTYPE)
    d["l3"] = l3s
    d["l4"] = l4s
    d["flags"] = flags
    return d


def apply(buf: np.ndarray, off, length, desc, opt):
    """The model over a packed batch: returns (new buffer, done array)."""
    out = buf.copy()
    done = np.zeros(len(off), np.uint8)
    for i in range(len(off)):
        o, n = int(off[i]), int(length[i])
        fr, done[i] = insert(bytes(buf[o:o + n]), int(desc["l3"][i]), int(desc["l4"][i]),
                             int(desc["flags"][i]), opt)
        out[o:o + n] = np.frombuffer(fr, np.uint8)
    return out, done


def offsets_of(frame: bytes):
    """(l3, l4) of a well-formed Ethernet frame the way the receive parse finds
    them: VLAN / QinQ tags skipped, IPv4 IHL, IPv6 fixed header."""
    o = 12
    et = struct.unpack_from("!H", frame, o)[0]
    while et in (0x8100, 0x88A8):
        o += 4
        et = struct.unpack_from("!H", frame, o)[0]
    l3 = o + 2
    if et == 0x0800:
        return l3, l3 + 4 * (frame[l3] & 0xF)
    if et == 0x86DD:
        return l3, l3 + 40
    return l3, INVALID


def valid_frames(seed=7, n=400):
    """[(frame, udp_zero)]: the frames of CK.frame_set valid by construction,
    and its two UDP zero-checksum frames."""
    fs = CK.frame_set(seed=seed, n=n)
    out = [(fr, False) for fr, l3_bad, l4_bad in fs[:-2] if l3_bad is not True and l4_bad is False]
    return out + [(fr, True) for fr, _, _ in fs[-2:]]


def scramble(frame: bytes, l3: int, l4: int, seed: int = 0x5A) -> bytes:
    """Overwrite the IPv4 header checksum and the L4 checksum field (by the IP
    header's protocol) with garbage."""
    b = bytearray(frame)
    g = bytes(((seed + 37 * i) & 0xFF) | 1 for i in range(4))
    ver = b[l3] >> 4
    if ver == 4:
        b[l3 + 10:l3 + 12] = g[:2]
        proto = b[l3 + 9]
    else:
        proto = b[l3 + 6]
    if proto == 17 and l4 + 8 <= len(b):
        b[l4 + 6:l4 + 8] = g[2:]
    elif proto == 6 and l4 + 18 <= len(b):
        b[l4 + 16:l4 + 18] = g[2:]
    elif proto == 132 and l4 + 12 <= len(b):
        b[l4 + 8:l4 + 12] = g
    return bytes(b)
