"""NumPy / pure-Python statement of the loop pktio's pktin flow hash.

Test infrastructure: what get_dest_queue (reference pktio/loop.c:479-530)
computes for a packet before its `% num_qs` -- the byte string it builds from
the packet's metadata (has_udp / has_tcp / has_ipv4 / has_ipv6, l3, l4; the
frame is not parsed) and odp_hash_crc32c(string, n, 0), the raw reflected
CRC-32C (polynomial 0x82F63B78, no final inversion; arch/default/
odp_hash_crc32.c:437-462).  The GPU kernel (mi_cls_tx_kernel with the hash
step) is compared with this model on all 32 bits.
"""
import numpy as np

# odp_pktin_hash_proto_t.all_bits
HP_IPV4_UDP, HP_IPV4_TCP, HP_IPV4, HP_IPV6_UDP, HP_IPV6_TCP, HP_IPV6 = 1, 2, 4, 8, 16, 32
HP_ALL = 63
# mi_cls_tx_desc_t.flags, the metadata bits (MI_CLS_TXF_*)
F_UDP, F_TCP, F_IPV4, F_IPV6 = 0x10, 0x20, 0x40, 0x80
INVALID = 0xFFFF

_TAB = np.zeros(256, np.uint32)
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    _TAB[_i] = _c
_TABL = [int(x) for x in _TAB]


def crc32c_raw(data: bytes, init: int = 0) -> int:
    """odp_hash_crc32c(data, len, init)."""
    crc = init & 0xFFFFFFFF
    for b in data:
        crc = _TABL[(crc ^ b) & 0xFF] ^ (crc >> 8)
    return crc


def hash_string(frame: bytes, l3: int, l4: int, flags: int, hash_proto: int) -> bytes:
    """The bytes get_dest_queue appends for this packet (hash_proto != 0)."""
    n = len(frame)
    s = b""
    if l4 != INVALID:
        if hash_proto & (HP_IPV4_UDP | HP_IPV6_UDP) and flags & F_UDP:
            if l4 + 8 <= n:
                s += frame[l4:l4 + 4]
        elif hash_proto & (HP_IPV4_TCP | HP_IPV6_TCP) and flags & F_TCP:
            if l4 + 20 <= n:
                s += frame[l4:l4 + 4]
    if l3 != INVALID:
        if hash_proto & HP_IPV4 and flags & F_IPV4:
            if l3 + 20 <= n:
                s += frame[l3 + 12:l3 + 20]
        elif hash_proto & HP_IPV6 and flags & F_IPV6:
            if l3 + 40 <= n:
                s += frame[l3 + 8:l3 + 40]
    return s


def flow_hash(frame: bytes, l3: int, l4: int, flags: int, hash_proto: int):
    """(hash, string length) of one packet."""
    s = hash_string(frame, l3, l4, flags, hash_proto)
    return crc32c_raw(s), len(s)


def apply(buf: np.ndarray, off, length, desc, hash_proto):
    """The model over a packed batch: (hash words, string lengths)."""
    n = len(off)
    h = np.zeros(n, np.uint32)
    ln = np.zeros(n, np.uint8)
    for i in range(n):
        o, k = int(off[i]), int(length[i])
        h[i], ln[i] = flow_hash(bytes(buf[o:o + k]), int(desc["l3"][i]), int(desc["l4"][i]),
                                int(desc["flags"][i]), hash_proto)
    return h, ln


def meta_flags(in_flags: int) -> int:
    """The descriptor's metadata bits from a packet's input flags (parse
    record / tests.parse_model: ipv4 bit 13, ipv6 14, udp 22, tcp 23)."""
    return ((F_IPV4 if in_flags >> 13 & 1 else 0) | (F_IPV6 if in_flags >> 14 & 1 else 0) |
            (F_UDP if in_flags >> 22 & 1 else 0) | (F_TCP if in_flags >> 23 & 1 else 0))


def dest_queue(h: int, num_qs: int, hash_proto: int, index: int) -> int:
    """The loop queue: hash off (hash_proto 0): the pktout index % num_qs."""
    return (h if hash_proto else index) % num_qs
