"""ctypes binding of oracle/_ref/libodp_ref.so: the reference's OWN parser,
checksum and classifier sources, compiled unchanged, behind ref_shim.c, and
the loop pktio's transmit code (checksum insertion, pktin flow hash) behind
ref_loop_shim.c.

*** TEST INFRASTRUCTURE ***  Only tests/ may import this module.  The library
is built by odp_amd._build.build() (oracle/Makefile ref-lib) where the
reference tree is present, and travels with the working tree elsewhere; it is
never committed.  A missing library is an error, not a skip.

``Reference`` is shaped like oracle.oracle.Oracle; its table sizes are the
reference's compile-time constants (64 CoS, 256 PMRs, 8 PMRs per CoS), so the
oracle and the kernels are compared with it at limits=(64, 256, 8).
"""
from __future__ import annotations

import ctypes as C
import os
import struct

import numpy as np

from oracle.oracle import RESULT_DTYPE, Term

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_ref", "libodp_ref.so")
LIMITS = (64, 256, 8)


class ParseOut(C.Structure):
    _fields_ = [("ret", C.c_int32), ("in_flags", C.c_uint32), ("err", C.c_uint32),
                ("l2", C.c_uint32), ("l3", C.c_uint32), ("l4", C.c_uint32),
                ("result_flags", C.c_uint64), ("res_len", C.c_uint32), ("res_l2", C.c_uint32),
                ("res_l3", C.c_uint32), ("res_l4", C.c_uint32), ("l2_type", C.c_uint32),
                ("l3_type", C.c_uint32), ("l4_type", C.c_uint32),
                ("l3_chksum_status", C.c_uint32), ("l4_chksum_status", C.c_uint32)]


PARSE_OUT_DTYPE = np.dtype([(n, "<i4" if n == "ret" else "<u8" if n == "result_flags" else "<u4")
                            for n, _ in ParseOut._fields_], align=True)
assert PARSE_OUT_DTYPE.itemsize == C.sizeof(ParseOut)

_lib = None


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(LIB), (f"{LIB} is missing: odp_amd._build.build() makes it where the "
                                     "reference tree is present (oracle/Makefile ref-lib)")
        L = C.CDLL(LIB)
        vp, i32, u32 = C.c_void_p, C.c_int, C.c_uint32
        L.ref_reset.restype = i32
        L.ref_limits.argtypes = [C.POINTER(u32)] * 3
        L.ref_cos_create.argtypes = [i32, u32, i32, u32, i32]
        L.ref_cos_destroy.argtypes = [i32]
        L.ref_pmr_create.argtypes = [C.POINTER(Term), i32, u32, i32, i32]
        L.ref_pmr_destroy.argtypes = [i32]
        L.ref_default_cos_set.argtypes = [i32]
        L.ref_error_cos_set.argtypes = [i32]
        L.ref_pktin_opt_set.argtypes = [C.c_uint64]
        L.ref_pktin_opt_set.restype = None
        L.ref_cos_stats_packets.argtypes = [i32]
        L.ref_cos_stats_packets.restype = C.c_uint64
        L.ref_classify_batch.argtypes = [vp, vp, vp, u32, vp]
        L.ref_packet_parse.argtypes = [vp, u32, u32, i32, i32, u32, C.POINTER(ParseOut)]
        lim = [u32(), u32(), u32()]
        L.ref_limits(*[C.byref(x) for x in lim])
        assert tuple(x.value for x in lim) == LIMITS
        _lib = L
    return _lib


def _terms(terms):
    arr = (Term * max(1, len(terms)))()
    for i, (term, value, mask, offset) in enumerate(terms):
        arr[i].term = term
        for j, b in enumerate(bytes(value)[:16]):
            arr[i].value[j] = b
        for j, b in enumerate(bytes(mask)[:16]):
            arr[i].mask[j] = b
        arr[i].val_sz = len(value)
        arr[i].offset = offset
    return arr


class Reference:
    """The reference's classifier tables and receive path (one instance at a
    time: the tables are the library's globals, reset here)."""

    def __init__(self, pktin_opt=0):
        self.L = lib()
        assert self.L.ref_reset() == 0
        self.cos = []
        self.pmr = []
        self.pktin_opt = pktin_opt

    def apply(self, prog):
        """Run a rule program (odp_amd.rules ops); returns the CoS and PMR
        handles in creation order, 0 where the reference refused the create."""
        L = self.L
        for op in prog:
            k = op[0]
            if k == "cos":
                a = op[2]
                self.cos.append(L.ref_cos_create(a["action"], a["num_queue"], 1 if a["queue"] else 0,
                                                 a["hash_proto"], a["stats"]))
            elif k == "pmr":
                self.pmr.append(L.ref_pmr_create(_terms(op[1]), len(op[1]), op[4],
                                                 self.cos[op[2]], self.cos[op[3]]))
            elif k == "pmr_destroy":
                L.ref_pmr_destroy(self.pmr[op[1]])
            elif k == "cos_destroy":
                L.ref_cos_destroy(self.cos[op[1]])
            elif k == "default":
                L.ref_default_cos_set(0 if op[1] is None else self.cos[op[1]])
            elif k == "error":
                L.ref_error_cos_set(0 if op[1] is None else self.cos[op[1]])
            else:
                raise ValueError(op)
        return self.cos, self.pmr

    def classify(self, batch):
        n = batch.n
        out = np.zeros(max(1, n), dtype=RESULT_DTYPE)
        buf = np.ascontiguousarray(batch.buf)
        off = np.ascontiguousarray(batch.off, dtype=np.uint32)
        ln = np.ascontiguousarray(batch.len, dtype=np.uint16)
        self.L.ref_pktin_opt_set(self.pktin_opt)
        rc = self.L.ref_classify_batch(buf.ctypes.data, off.ctypes.data, ln.ctypes.data, n,
                                       out.ctypes.data)
        if rc == -2:
            raise ValueError("the rule graph has a CoS cycle: the reference would never return")
        assert rc == 0, rc
        return out[:n]

    def stats_packets(self, cos_handle):
        return self.L.ref_cos_stats_packets(cos_handle)


def packet_parse(frame: bytes, offset: int, proto: int, layer: int, chksums: int) -> ParseOut:
    """odp_packet_parse(frame, offset, {proto, layer, chksums}) followed by
    odp_packet_parse_result, on a one-segment packet."""
    out = ParseOut()
    b = np.frombuffer(frame, dtype=np.uint8) if frame else np.zeros(1, np.uint8)
    assert lib().ref_packet_parse(b.ctypes.data, len(frame), offset, proto, layer, chksums,
                                  C.byref(out)) == 0
    return out


# ------------------------------------------------------------ transmit side
# ref_loop_shim.c: the reference's loopback_fix_checksums and get_dest_queue
# (pktio/loop.c) on the same fake packet.

# The reference exposes only hash % num_qs.  These six moduli are pairwise
# coprime, none exceeds the loop pktio's 64 queues, and their product
# 42 300 054 720 exceeds 2^32: by the Chinese remainder theorem, agreement on
# all six residues is agreement on all 32 bits of the hash.
TX_MODULI = (64, 63, 61, 59, 55, 53)

# The transmit entries are bound from a second link of the same objects:
# _ref/libodp_ref.so is also what an oracle/ from before ref_loop_shim.c
# builds, without them, when such an older checker runs beside this build.
TX_LIB = os.path.join(HERE, "_ref", "libodp_ref_tx.so")
_tx_lib = None


def tx_lib():
    global _tx_lib
    if _tx_lib is None:
        assert os.path.exists(TX_LIB), (f"{TX_LIB} is missing: odp_amd._build.build() makes it where the "
                                        "reference tree is present (oracle/Makefile ref-lib)")
        L = C.CDLL(TX_LIB)
        vp, i32, u32 = C.c_void_p, C.c_int, C.c_uint32
        L.ref_tx_fix_checksums.argtypes = [vp, u32, u32, u32, u32, u32, vp]
        L.ref_tx_dest_queue.argtypes = [vp, u32, u32, u32, u32, u32, u32, i32]
        L.ref_tx_fix_checksums_batch.argtypes = [vp, vp, vp, vp, u32, u32, vp]
        L.ref_tx_dest_queue_batch.argtypes = [vp, vp, vp, vp, u32, u32, i32, vp]
        _tx_lib = L
    return _tx_lib


def tx_fix_checksums_one(frame: bytes, l3: int, l4: int, flags: int, opt: int) -> bytes:
    """loopback_fix_checksums on one frame: l3 / l4 (0xFFFF: invalid), the
    descriptor's four override bits, pktout_cfg.all_bits = opt (ipv4_chksum
    is bit 5 there: tests.tx_model.all_bits of a kernel option word)."""
    src = np.frombuffer(frame, dtype=np.uint8) if frame else np.zeros(1, np.uint8)
    out = np.zeros(max(1, len(frame)), np.uint8)
    assert tx_lib().ref_tx_fix_checksums(src.ctypes.data, len(frame), l3, l4, flags, opt, out.ctypes.data) == 0
    return bytes(out[:len(frame)])


def tx_dest_queue_one(frame: bytes, l3: int, l4: int, meta_flags: int, hash_proto: int, num_qs: int,
                      index: int = 0) -> int:
    """get_dest_queue on one frame: the index of the loop queue it picks."""
    src = np.frombuffer(frame, dtype=np.uint8) if frame else np.zeros(1, np.uint8)
    q = tx_lib().ref_tx_dest_queue(src.ctypes.data, len(frame), l3, l4, meta_flags, hash_proto, num_qs, index)
    assert q >= 0, q
    return q


def _tx_args(buf, off, length, desc):
    assert desc.dtype.itemsize == 8 and len(desc) == len(off) == len(length)
    return (np.ascontiguousarray(buf), np.ascontiguousarray(off, dtype=np.uint32),
            np.ascontiguousarray(length, dtype=np.uint16), np.ascontiguousarray(desc))


def tx_fix_checksums(buf, off, length, desc, opt):
    """What tests.tx_model.apply takes, with opt as pktout_cfg.all_bits: the
    new buffer (no done bytes: the reference has none)."""
    buf, off, length, desc = _tx_args(buf, off, length, desc)
    out = buf.copy()
    assert tx_lib().ref_tx_fix_checksums_batch(buf.ctypes.data, off.ctypes.data, length.ctypes.data,
                                            desc.ctypes.data, len(off), opt, out.ctypes.data) == 0
    return out


def tx_dest_queues(buf, off, length, desc, hash_proto, index=0):
    """What tests.txq_model.apply takes: an (n, 6) array, get_dest_queue's
    queue index for num_qs = each of TX_MODULI."""
    buf, off, length, desc = _tx_args(buf, off, length, desc)
    res = np.zeros((len(off), len(TX_MODULI)), np.uint8)
    assert tx_lib().ref_tx_dest_queue_batch(buf.ctypes.data, off.ctypes.data, length.ctypes.data,
                                         desc.ctypes.data, len(off), hash_proto, index,
                                         res.ctypes.data) == 0
    return res


def write_tx_corpus(path, cases, opts, hash_protos):
    """[(frame, l3, l4, flags)] and the option / hash_proto rows in the
    format ref_shim.c's main reads ("RST1")."""
    with open(path, "wb") as f:
        f.write(b"RST1" + struct.pack("<I", len(opts)) + struct.pack(f"<{len(opts)}I", *opts))
        f.write(struct.pack("<I", len(hash_protos)) + struct.pack(f"<{len(hash_protos)}I", *hash_protos))
        f.write(struct.pack("<I", len(cases)))
        for fr, l3, l4, flags in cases:
            f.write(struct.pack("<HHHB", len(fr), l3, l4, flags) + fr)


# ------------------------------------------------- corpus of ref_shim_main
def write_corpus(path, prog, frames, pktin_opt=0):
    """One rule program and its frames in the format ref_shim.c's main reads."""
    ops = []
    for op in prog:
        k = op[0]
        if k == "cos":
            a = op[2]
            ops.append(struct.pack("<BBBBII", 1, a["action"], 1 if a["queue"] else 0, a["stats"],
                                   a["num_queue"], a["hash_proto"]))
        elif k == "pmr":
            ops.append(struct.pack("<BBIii", 2, len(op[1]), op[4], op[2], op[3]) +
                       bytes(_terms(op[1]))[:len(op[1]) * C.sizeof(Term)])
        elif k in ("pmr_destroy", "cos_destroy"):
            ops.append(struct.pack("<BI", 3 if k == "pmr_destroy" else 4, op[1]))
        elif k in ("default", "error"):
            ops.append(struct.pack("<Bi", 5 if k == "default" else 6, -1 if op[1] is None else op[1]))
        else:
            raise ValueError(op)
    with open(path, "wb") as f:
        f.write(b"RSC1" + struct.pack("<QI", pktin_opt, len(ops)) + b"".join(ops))
        f.write(struct.pack("<I", len(frames)))
        for fr in frames:
            f.write(struct.pack("<H", len(fr)) + fr)
