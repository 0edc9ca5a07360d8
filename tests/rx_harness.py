"""ctypes access to the receive delivery / receive chain entry points of
libmi_cls.so for the kernel tests (test-only; the runtime reaches them
through odp_pktin.c).

An Arena is one page-locked allocation that holds everything the device
reads or writes in a run: frames, descriptors, records, table, packet lists,
output arrays and a pool of fake packets.  Before a run it is filled with a
seeded non-zero pattern, the inputs are written over it, and after the wait
the whole arena is compared with an expected image (the image before the
submit with the model's outputs written in), so a stray or a missing store
anywhere in it shows.
"""
from __future__ import annotations

import ctypes as C
import errno

import numpy as np

from odp_amd import cls

from tests import rx_model as M
from tests.rx_model import DLV_DTYPE, META_DTYPE, RXOUT_DTYPE, RXTAB_DTYPE  # noqa: F401 (re-exported)

EINVAL, E2BIG = errno.EINVAL, errno.E2BIG
vp, u8, u16, u32, u64 = C.c_void_p, C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64


class Dlv(C.Structure):
    """mi_cls_dlv_t"""
    _fields_ = [("meta", u64), ("dst_queue", u64), ("user_ptr", u64), ("src", u32), ("rec", u32),
                ("len", u16), ("flags", u8), ("qid", u8), ("data_off", u32), ("rsv", u64)]


class DlvArgs(C.Structure):
    """mi_cls_dlv_args_t"""
    _fields_ = [("base", vp), ("res", vp), ("dlv", vp), ("n", u32), ("layer", u32),
                ("input", u64), ("headroom", u32), ("data_from_meta", u32), ("perm", vp),
                ("gcnt", vp)]


class RxTab(C.Structure):
    """mi_cls_rxtab_t"""
    _fields_ = [("flags", u32), ("npool", u32), ("pool_cap", u32 * 16), ("rt_slot", u8 * 64),
                ("cos_pool", u8 * 256), ("cos_nq", u8 * 256), ("cos_q0", u16 * 256),
                ("rt_pinned", u8 * 64), ("qh", u64 * 1024), ("qg", u8 * 1024), ("stamp", u64)]


class RxOut(C.Structure):
    """mi_cls_rx_out_t"""
    _fields_ = [("in_errors", u64), ("in_discards", u64), ("packets", u64), ("octets", u64),
                ("used", u32 * 16), ("need", u32 * 16), ("short_pool", u32),
                ("not_in_place", u32), ("rsv", u32 * 2)]


class RxcArgs(C.Structure):
    """mi_cls_rxc_args_t"""
    _fields_ = [("base", vp), ("soff", vp), ("slen", vp), ("res", vp), ("n", u32), ("layer", u32),
                ("input", u64), ("headroom", u32), ("data_from_meta", u32), ("tab", vp),
                ("got", vp), ("got_base", u32 * 16), ("have", u32 * 16), ("pk", vp),
                ("ppool", vp), ("pdoff", vp), ("meta_off", u32), ("stage", u32),
                ("head_off", u16), ("pool_off", u16), ("dec", vp), ("ent", vp), ("perm", vp),
                ("gcnt", vp), ("out", vp)]


STRUCTS = {"mi_cls_dlv_t": Dlv, "mi_cls_dlv_args_t": DlvArgs, "mi_cls_rxtab_t": RxTab,
           "mi_cls_rx_out_t": RxOut, "mi_cls_rxc_args_t": RxcArgs}
DTYPES = {"mi_cls_pkt_meta_t": META_DTYPE, "mi_cls_dlv_t": DLV_DTYPE, "mi_cls_rxtab_t": RXTAB_DTYPE,
          "mi_cls_rx_out_t": RXOUT_DTYPE, "mi_cls_result_t": M.RESULT_DTYPE}


def layout_of(name):
    """{field: offset, "": size} of a bound struct, from ctypes and from numpy."""
    out = []
    if name in STRUCTS:
        s = STRUCTS[name]
        d = {f[0]: getattr(s, f[0]).offset for f in s._fields_}
        d[""] = C.sizeof(s)
        out.append(d)
    if name in DTYPES:
        t = DTYPES[name]
        d = {f: t.fields[f][1] for f in t.names}
        d[""] = t.itemsize
        out.append(d)
    return out


_bound = None


def lib():
    """cls.lib() with the receive entry points' signatures set."""
    global _bound
    if _bound is None:
        L = cls.lib()
        for name, res, args in (
                ("mi_cls_deliver_submit", C.c_int, [vp, C.POINTER(DlvArgs), C.POINTER(u64)]),
                ("mi_cls_rx_chain_submit", C.c_int, [vp, vp, C.c_size_t, C.POINTER(RxcArgs),
                                                     C.POINTER(u64)]),
                ("mi_cls_classify_host_wait", C.c_int, [vp, u64]),
                ("mi_cls_host_mapped", C.c_int, [vp])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _bound = L
    return _bound


class Context:
    """A device context (mi_cls_ctx_create), with a compiled rule table
    loaded when one is given."""

    def __init__(self, blob=None, gpu=0):
        self.L = lib()
        ctx = vp()
        rc = self.L.mi_cls_ctx_create(gpu, C.byref(ctx))
        if rc:
            raise RuntimeError(f"mi_cls_ctx_create: {rc}")
        self.ctx = ctx
        if blob is not None:
            rc = self.L.mi_cls_rules_load(ctx, blob, len(blob), None)
            if rc:
                raise RuntimeError(f"mi_cls_rules_load: {rc}")

    @staticmethod
    def _hip_ok(rc):
        """-EIO is a failed HIP call: the device may have faulted, so the
        session ends here and starts nothing more on it."""
        if rc == -errno.EIO:
            import pytest
            pytest.exit("a HIP call failed (-EIO): no further GPU work is started", returncode=3)
        return rc

    def deliver_submit(self, args):
        t = u64(0xDEAD)
        rc = self._hip_ok(self.L.mi_cls_deliver_submit(self.ctx, C.byref(args), C.byref(t)))
        return rc, t.value

    def chain_submit(self, pkts, nbytes, args):
        t = u64(0xDEAD)
        rc = self._hip_ok(self.L.mi_cls_rx_chain_submit(self.ctx, pkts, nbytes, C.byref(args),
                                                        C.byref(t)))
        return rc, t.value

    def wait(self, ticket):
        return self._hip_ok(self.L.mi_cls_classify_host_wait(self.ctx, ticket))

    def close(self):
        if self.ctx:
            self.L.mi_cls_ctx_destroy(self.ctx)
            self.ctx = None


# fake packet: a 64-byte header line (the buffer pointer and the pool index the
# stage kernel reads), the 64-byte metadata line, headroom, data
HEAD_OFF, POOL_OFF, META_OFF = 8, 16, 64
HEADROOM = 128
DATA_FROM_META = 64 + HEADROOM      # from the metadata line to the data at HEADROOM
TAIL = 64


class Arena:
    """Bump allocator over one cls.PinnedArray, with named regions."""

    def __init__(self, nbytes):
        self.mem = cls.PinnedArray(nbytes)
        assert lib().mi_cls_host_mapped(self.mem.ptr) == 1
        self.ptr, self.nbytes, self.u8 = self.mem.ptr, nbytes, self.mem.u8
        self.reset()

    def close(self):
        self.mem.close()

    def reset(self):
        self.top, self.regions = 0, []

    def alloc(self, name, nbytes, align=64, item=1):
        off = (self.top + align - 1) & ~(align - 1)
        assert off + nbytes <= self.nbytes, "arena too small"
        self.top = off + nbytes
        self.regions.append((off, nbytes, name, item))
        return off

    def array(self, name, dtype, count, align=64):
        dtype = np.dtype(dtype)
        off = self.alloc(name, dtype.itemsize * count, align, dtype.itemsize)
        return off, self.u8[off: off + dtype.itemsize * count].view(dtype)

    def packets(self, name, count, cap):
        """count fake packets of `cap` data bytes; returns their handles'
        offsets.  Their headers are written by init_packets (after fill)."""
        size = META_OFF + DATA_FROM_META + ((cap + 63) & ~63) + TAIL
        off = self.alloc(name, size * count, 64, size)
        return off + size * np.arange(count, dtype=np.int64), size

    def fill(self, seed):
        """Every byte allocated so far (the gaps too) gets a non-zero pattern."""
        rng = np.random.default_rng(seed)
        self.u8[: self.top] = rng.integers(1, 256, self.top, dtype=np.uint8)

    def init_packets(self, offs, pool):
        for o in offs:
            o = int(o)
            self.u8[o + HEAD_OFF: o + HEAD_OFF + 8].view("<u8")[0] = self.ptr + o + META_OFF + 64
            self.u8[o + POOL_OFF: o + POOL_OFF + 2].view("<u2")[0] = pool
            m = self.meta(o)
            m["data_off"] = HEADROOM

    def meta(self, pkt_off, image=None):
        img = self.u8 if image is None else image
        o = int(pkt_off) + META_OFF
        return img[o: o + 64].view(META_DTYPE)[0]

    def snapshot(self):
        return self.u8[: self.top].copy()

    def where(self, off):
        for o, nb, name, item in self.regions:
            if o <= off < o + nb:
                return name, (off - o) // item, (off - o) % item
        return "gap", off, 0


def put_packet(arena, exp, care, pkt_off, line, frame=None):
    """Write a delivered packet into the expected image: its metadata line and,
    for a copied frame, the data (the bytes up to the copy extent do not
    matter: care = 0)."""
    o = int(pkt_off) + META_OFF
    exp[o: o + 64] = np.frombuffer(line, np.uint8)
    if frame is not None:
        d = o + DATA_FROM_META
        exp[d: d + len(frame)] = frame
        care[d + len(frame): d + M.copy_extent(len(frame))] = 0


def compare(arena, got, exp, care, describe=None):
    """Exact equality of the arena with the expected image where care != 0."""
    bad = np.nonzero((got != exp) & (care != 0))[0]
    if not len(bad):
        return
    off = int(bad[0])
    name, idx, byte = arena.where(off)
    msg = (f"{len(bad)} bytes differ; first at arena offset {off}: region {name} item {idx} "
           f"byte {byte}: got {got[off: off + 16].tobytes().hex()} "
           f"expected {exp[off: off + 16].tobytes().hex()}")
    if describe:
        msg += "\n" + describe(name, idx)
    raise AssertionError(msg)
