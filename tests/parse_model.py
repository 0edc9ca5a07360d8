"""CPU model of odp_packet_parse() (include/odp_rt.h, mi_cls_parse).

*** TEST INFRASTRUCTURE ***  Built on the oracle's full parse of an Ethernet
frame (oracle.oracle.parse) and the parser-layer cut of tests.rx_model
(apply_layer); nothing is taken from the kernels.

  ETH at offset o    parse frame[o:] with pktin_opt = chksums << 2, apply the
                     layer cut, add o to every valid offset.
  IPV4 / IPV6 at o   parse `a unicast 14-byte Ethernet header with ethertype
                     0x0800 / 0x86DD` + frame[o:]; clear the L2, ETH and JUMBO
                     bits, l2 invalid, offsets shifted by o - 14.
  return value       after the cut: layers L2 / L3: -1 iff an error bit is
                     left; layers L4 / ALL: -1 iff the oracle returned non-zero.
"""
from __future__ import annotations

import numpy as np

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests.rx_model import apply_layer

PROTO_ETH, PROTO_IPV4, PROTO_IPV6 = 1, 2, 3
L2, L3, L4, ALL = 1, 2, 3, 4
INVALID = 0xFFFF
# the reference's l2_offset[] (test/validation/api/packet/packet.c:3722)
REF_OFFSETS = (0, 2, 8, 12, 19, 36, 64, 120, 207, 0)

_F_L2, _F_ETH, _F_JUMBO = 1 << 3, 1 << 6, 1 << 9
_ETH_HDR = {PROTO_IPV4: bytes.fromhex("020000000001020000000002" "0800"),
            PROTO_IPV6: bytes.fromhex("020000000001020000000002" "86dd")}


def parse(frame: bytes, offset: int, proto: int, layer: int, chksums: int):
    """(ret, input_flags (low 32 bits), err, l2, l3, l4), offsets from the
    start of `frame`; ret 0 / -1 as odp_packet_parse."""
    from oracle.oracle import parse as oparse
    assert proto in (PROTO_ETH, PROTO_IPV4, PROTO_IPV6) and layer in (L2, L3, L4, ALL)
    assert 0 <= offset < len(frame)
    if proto == PROTO_ETH:
        r, fl, err, _, l3, l4 = oparse(frame[offset:], (chksums & 0xF) << 2)
        l2, shift = offset, offset
    else:
        r, fl, err, _, l3, l4 = oparse(_ETH_HDR[proto] + frame[offset:], (chksums & 0xF) << 2)
        fl &= ~(_F_L2 | _F_ETH | _F_JUMBO)
        l2, shift = INVALID, offset - 14
    fl, err, l4 = apply_layer(fl & 0xFFFFFFFF, err, l4, layer)
    ret = -1 if (err != 0 if layer < L4 else r != 0) else 0
    l3 = l3 + shift if l3 != INVALID else INVALID
    l4 = l4 + shift if l4 != INVALID else INVALID
    return ret, fl, err, l2, l3, l4


def record(frame: bytes, offset: int, proto: int, layer: int, chksums: int):
    """The mi_cls_result_t of mi_cls_parse for this packet: offsets relative
    to the parse start, outcome ENQ / PARSE_DROP, the rest zero."""
    ret, fl, err, _, l3, l4 = parse(frame, offset, proto, layer, chksums)
    rec = np.zeros((), R.RESULT_DTYPE)
    rec["in_flags"], rec["err"] = fl, err
    rec["outcome"] = R.OUT_PARSE_DROP if ret else R.OUT_ENQ
    rec["l3_offset"] = l3 - offset if l3 != INVALID else INVALID
    rec["l4_offset"] = l4 - offset if l4 != INVALID else INVALID
    return rec


def records(frames, offsets, proto, layer, chksums):
    out = np.zeros(len(frames), R.RESULT_DTYPE)
    for i, (f, o) in enumerate(zip(frames, offsets)):
        out[i] = record(f, o, proto, layer, chksums)
    return out


def batch_at(frames, offsets):
    """A pktgen.Batch whose descriptors have the parse offsets folded in:
    off[i] the byte where packet i's parse starts, len[i] = len - offset."""
    b = pg.batch_from_frames(frames)
    o = np.asarray(offsets, dtype=np.uint32)
    return pg.Batch(b.buf, (b.off + o).astype(np.uint32), (b.len - o).astype(np.uint16))


def shifted(frame: bytes, offset: int) -> bytes:
    """`frame` behind `offset` filler bytes (parse_test_alloc, packet.c:3718-3742)."""
    return bytes(i & 0xFF for i in range(offset)) + frame


# ------------------------------------------------ odp_packet_parse_result
# input_flags bits (packet_inline_types.h:60-107)
FLAG_BITS = {"l2": 3, "l3": 4, "l4": 5, "eth": 6, "eth_bcast": 7, "eth_mcast": 8, "jumbo": 9, "vlan": 10,
             "vlan_qinq": 11, "arp": 12, "ipv4": 13, "ipv6": 14, "ip_bcast": 15, "ip_mcast": 16,
             "ipfrag": 17, "ipopt": 18, "ipsec": 19, "udp": 22, "tcp": 23, "sctp": 24, "icmp": 25}
# odp_packet_parse_result_flag_t, bit order
RESULT_BITS = ("has_error", "has_l2_error", "has_l3_error", "has_l4_error", "l2", "l3", "l4", "eth",
               "eth_bcast", "eth_mcast", "jumbo", "vlan", "vlan_qinq", "arp", "ipv4", "ipv6", "ip_bcast",
               "ip_mcast", "ipfrag", "ipopt", "ipsec", "udp", "tcp", "sctp", "icmp")


def result_word(flags, err):
    w = 0
    for i, name in enumerate(RESULT_BITS):
        if name == "has_error":
            bit = err != 0
        elif name == "has_l2_error":
            bit = err & 0x01
        elif name == "has_l3_error":      # ip_err alone (packet_flag_inlines.h:277-284)
            bit = err & 0x02
        elif name == "has_l4_error":      # tcp_err | udp_err (packet_flag_inlines.h:286-293)
            bit = err & 0x18
        else:
            bit = (flags >> FLAG_BITS[name]) & 1
        w |= (1 if bit else 0) << i
    return w


def types_of(flags):
    l2 = 1 if flags >> 6 & 1 else 0
    l3 = 0x0800 if flags >> 13 & 1 else 0x86DD if flags >> 14 & 1 else 0x0806 if flags >> 12 & 1 else 0xFFFF
    icmp = flags >> 25 & 1
    l4 = (6 if flags >> 23 & 1 else 17 if flags >> 22 & 1 else 132 if flags >> 24 & 1 else
          51 if flags >> 20 & 1 else 50 if flags >> 21 & 1 else 1 if icmp and flags >> 13 & 1 else
          58 if icmp and flags >> 14 & 1 else 59 if flags >> 26 & 1 else 255)
    return l2, l3, l4
