"""ctypes binding of libodp_cls.so (include/odp_cls_api.h) and libmi_cls.so.

This is the host-side mirror of the reference's classifier interface
(include/odp/api/spec/classification.h) used by the tests and bench: the
same function names, argument meaning and error behaviour (INVALID handle
= 0 on failure, -1 from destroy, ...).  The compute path is the HIP kernel in
libmi_cls.so; there is no CPU fallback -- loading fails loudly if the
native libraries are missing.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import rules as R

_HERE = os.path.dirname(os.path.abspath(__file__))
# ODP_AMD_LIB_DIR selects an alternative build (kernel variants for A/B runs)
_LIBDIR = os.environ.get("ODP_AMD_LIB_DIR", _HERE)
LIB_MI = os.path.join(_LIBDIR, "libmi_cls.so")
LIB_ODP = os.path.join(_LIBDIR, "libodp_cls.so")


class PmrParam(C.Structure):
    """odp_pmr_param_t (classification.h:278-321)."""
    _fields_ = [("term", C.c_int), ("range_term", C.c_bool), ("value", C.c_void_p),
                ("mask", C.c_void_p), ("val_sz", C.c_uint32), ("offset", C.c_uint32)]


class PmrCreateOpt(C.Structure):
    """odp_pmr_create_opt_t."""
    _fields_ = [("terms", C.POINTER(PmrParam)), ("num_terms", C.c_int), ("mark", C.c_uint64),
                ("priority", C.c_uint32)]


class SchedParam(C.Structure):
    _fields_ = [("prio", C.c_int), ("sync", C.c_int), ("group", C.c_int),
                ("lock_count", C.c_uint32)]


class QueueParam(C.Structure):
    """odp_queue_param_t (queue_types.h:249-349)."""
    _fields_ = [("type", C.c_int), ("enq_mode", C.c_int), ("deq_mode", C.c_int),
                ("sched", SchedParam), ("order", C.c_int), ("nonblocking", C.c_int),
                ("context", C.c_void_p), ("context_len", C.c_uint32), ("size", C.c_uint32),
                ("num_aggr", C.c_uint32), ("aggr", C.c_void_p)]


class _QP(C.Structure):
    _fields_ = [("queue_param", QueueParam), ("hash_proto", C.c_uint32)]


class _QU(C.Union):
    _fields_ = [("queue", C.c_void_p), ("qp", _QP)]


class RedParam(C.Structure):
    _fields_ = [("enable", C.c_bool), ("threshold", C.c_uint64)]


class BpParam(C.Structure):
    _fields_ = [("enable", C.c_bool), ("threshold", C.c_uint64), ("pfc_level", C.c_uint8)]


class VectorCfg(C.Structure):
    _fields_ = [("enable", C.c_bool), ("pool", C.c_void_p), ("max_tmo_ns", C.c_uint64),
                ("max_size", C.c_uint32)]


class AggrProfile(C.Structure):
    _fields_ = [("type", C.c_int), ("param", C.c_void_p)]


class CosParam(C.Structure):
    """odp_cls_cos_param_t (classification.h:647-770)."""
    _anonymous_ = ("u",)
    _fields_ = [("action", C.c_int), ("stats_enable", C.c_bool), ("num_queue", C.c_uint32),
                ("u", _QU), ("pool", C.c_void_p), ("red", RedParam), ("bp", BpParam),
                ("vector", VectorCfg), ("aggr_enq_profile", AggrProfile)]


class CosStats(C.Structure):
    _fields_ = [("octets", C.c_uint64), ("packets", C.c_uint64), ("discards", C.c_uint64),
                ("errors", C.c_uint64)]


class Capability(C.Structure):
    _fields_ = [("supported_terms", C.c_uint64), ("max_pmr", C.c_uint32),
                ("max_pmr_per_cos", C.c_uint32), ("max_terms_per_pmr", C.c_uint32),
                ("max_pmr_priority", C.c_uint32), ("max_cos", C.c_uint32),
                ("max_cos_stats", C.c_uint32), ("max_hash_queues", C.c_uint32),
                ("hash_protocols", C.c_uint32), ("pmr_range_supported", C.c_bool),
                ("random_early_detection", C.c_int), ("threshold_red", C.c_uint8),
                ("back_pressure", C.c_int), ("threshold_bp", C.c_uint8),
                ("max_mark", C.c_uint64), ("stats_cos", C.c_uint64), ("stats_queue", C.c_uint64)]


class ParseParam(C.Structure):
    """mi_cls_parse_param_t."""
    _fields_ = [("proto", C.c_uint32), ("last_layer", C.c_uint32), ("chksums", C.c_uint32)]


# the enqueue plan (include/mi_cls.h): the table's bounds, the kernels' shape
ENQ_ENT, ENQ_DST_MAX = 8192, 8192
ENQ_TILE, ENQ_GRID, ENQ_DIGIT = 1024, 256, 8


class EnqTab(C.Structure):
    """mi_cls_enq_tab_t."""
    _fields_ = [("ndst", C.c_uint32), ("rsv", C.c_uint32), ("cos_nq", C.c_uint8 * 256),
                ("cos_q0", C.c_uint16 * 256), ("ent_dst", C.c_uint16 * ENQ_ENT), ("stamp", C.c_uint64)]


class EnqOut(C.Structure):
    """mi_cls_enq_out_t."""
    _fields_ = [("in_errors", C.c_uint64), ("in_discards", C.c_uint64), ("packets", C.c_uint64),
                ("octets", C.c_uint64), ("delivered", C.c_uint64), ("stale", C.c_uint64)]


ENQ_OUT_FIELDS = tuple(f[0] for f in EnqOut._fields_)
_enq_stamps = 0


def enq_tab(cos_nq, cos_q0, ent_dst, ndst) -> EnqTab:
    """A mi_cls_enq_tab_t from its arrays (cos_nq / cos_q0: up to 256 values
    by CoS index, ent_dst: up to ENQ_ENT destination ids), with a stamp no
    earlier table of this process had."""
    global _enq_stamps
    t = EnqTab()
    t.ndst = int(ndst)
    for name, src in (("cos_nq", cos_nq), ("cos_q0", cos_q0), ("ent_dst", ent_dst)):
        a = np.ctypeslib.as_array(getattr(t, name))
        s = np.asarray(src)
        a[:s.shape[0]] = s
    _enq_stamps += 1
    t.stamp = (1 << 32) + _enq_stamps
    return t


# the run plan (include/mi_cls.h): the mode bits, the vector-pool slots, the
# kernels' shape
RUN_AGGR, RUN_VEC, RUN_VSLOTS = 1, 2, 16
RUN_TILE, RUN_GRID = 1024, 256
RUN_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("dst", "<u2"), ("cos", "u1"), ("flags", "u1"),
                      ("nvec", "<u4")])


class RunTab(C.Structure):
    """mi_cls_run_tab_t."""
    _fields_ = [("mode", C.c_uint8 * 256), ("vmax", C.c_uint16 * 256), ("vslot", C.c_uint8 * 256),
                ("stamp", C.c_uint64)]


class RunOut(C.Structure):
    """mi_cls_run_out_t."""
    _fields_ = EnqOut._fields_ + [("nruns", C.c_uint64), ("vectors", C.c_uint64),
                                  ("vec_need", C.c_uint64 * RUN_VSLOTS)]


RUN_OUT_WORDS = C.sizeof(RunOut) // 8


def run_tab(mode, vmax, vslot) -> RunTab:
    """A mi_cls_run_tab_t from its arrays (up to 256 values by CoS index), with
    a stamp no earlier table of this process had."""
    global _enq_stamps
    t = RunTab()
    for name, src in (("mode", mode), ("vmax", vmax), ("vslot", vslot)):
        a = np.ctypeslib.as_array(getattr(t, name))
        s = np.asarray(src)
        a[:s.shape[0]] = s
    _enq_stamps += 1
    t.stamp = (1 << 32) + _enq_stamps
    return t


# the pool plan (include/mi_cls.h): the slots, the fates of dec, the kernels'
# shape
POOL_SLOTS = 16
POOL_TILE, POOL_GRID = 1024, 256
POOL_NONE, POOL_INPLACE, POOL_FRESH, POOL_TOO_LONG, POOL_SHORT = 0, 1, 2, 3, 4
POOL_NO_IDX = 0xFFFFFFFF        # idx of every record that is not FRESH
POOL_UNLIMITED = 0xFFFFFFFF     # have[k]: the need alone, nothing is SHORT


class PoolTab(C.Structure):
    """mi_cls_pool_tab_t."""
    _fields_ = [("nslot", C.c_uint32), ("rsv", C.c_uint32), ("slot_cap", C.c_uint32 * POOL_SLOTS),
                ("cos_slot", C.c_uint8 * 256), ("stamp", C.c_uint64)]


class PoolOut(C.Structure):
    """mi_cls_pool_out_t."""
    _fields_ = [("inplace", C.c_uint64), ("fresh", C.c_uint64), ("too_long", C.c_uint64),
                ("shorted", C.c_uint64), ("need", C.c_uint32 * POOL_SLOTS), ("used", C.c_uint32 * POOL_SLOTS)]


POOL_OUT_FIELDS = ("inplace", "fresh", "too_long", "shorted")
POOL_OUT_WORDS = C.sizeof(PoolOut) // 4      # 32-bit words
POOL_OUT_DTYPE = np.dtype([("inplace", "<u8"), ("fresh", "<u8"), ("too_long", "<u8"), ("shorted", "<u8"),
                           ("need", "<u4", (POOL_SLOTS,)), ("used", "<u4", (POOL_SLOTS,))])


def pool_tab(cos_slot, slot_cap, nslot=None) -> PoolTab:
    """A mi_cls_pool_tab_t from its arrays (cos_slot: up to 256 values by CoS
    index, the rest 0xFF; slot_cap: up to POOL_SLOTS values; nslot: their number
    by default), with a stamp no earlier table of this process had."""
    global _enq_stamps
    t = PoolTab()
    cs = np.ctypeslib.as_array(t.cos_slot)
    cs[:] = 0xFF
    s = np.asarray(cos_slot)
    cs[:s.shape[0]] = s
    caps = np.asarray(slot_cap, dtype=np.uint32)
    np.ctypeslib.as_array(t.slot_cap)[:caps.shape[0]] = caps
    t.nslot = int(caps.shape[0] if nslot is None else nslot)
    _enq_stamps += 1
    t.stamp = (1 << 32) + _enq_stamps
    return t


def pool_out_dict(words32):
    """The 40 32-bit words of a mi_cls_pool_out_t as a dict (need, used: lists)."""
    o = np.ascontiguousarray(words32, dtype=np.uint32).view(POOL_OUT_DTYPE)[0]
    d = {k: int(o[k]) for k in POOL_OUT_FIELDS}
    d["need"] = [int(v) for v in o["need"]]
    d["used"] = [int(v) for v in o["used"]]
    return d


def _pool_u32x16(v):
    a = (C.c_uint32 * POOL_SLOTS)()
    for k, x in enumerate(v):
        a[k] = int(x)
    return a


# the pool move (include/mi_cls.h): the kernel's shape (a wave's tile of
# records, the blocks' bound, the bytes of a copy round)
MOVE_TILE, MOVE_GRID, MOVE_ROUND = 64, 512, 8192


class MoveOut(C.Structure):
    """mi_cls_move_out_t."""
    _fields_ = [("moved", C.c_uint64), ("inplace", C.c_uint64), ("bytes", C.c_uint64), ("refused", C.c_uint64)]


MOVE_OUT_FIELDS = tuple(f[0] for f in MoveOut._fields_)


class MoveArgs(C.Structure):
    """mi_cls_move_args_t."""
    _fields_ = [("pkts", C.c_void_p), ("pkts_bytes", C.c_uint64), ("off", C.c_void_p), ("len", C.c_void_p),
                ("res", C.c_void_p), ("dec", C.c_void_p), ("idx", C.c_void_p), ("got", C.c_void_p),
                ("pk", C.c_void_p), ("n", C.c_uint32), ("ngot", C.c_uint32), ("tab", C.POINTER(EnqTab)),
                ("dst_queue", C.c_void_p), ("input", C.c_uint64), ("headroom", C.c_uint32),
                ("data_from_meta", C.c_uint32), ("arena_lo", C.c_uint64), ("arena_bytes", C.c_uint64),
                ("ent", C.c_void_p), ("out", C.c_void_p)]


def move_args(tab, dst_queue, **kw) -> MoveArgs:
    """A mi_cls_move_args_t: tab an EnqTab (None: NULL), dst_queue the
    odp_queue_t of each destination id (a sequence; None: NULL), every other
    field by keyword -- pointers as ints (0 / None: NULL).  The table and the
    queue array stay alive with the returned struct."""
    a = MoveArgs()
    if tab is not None:
        a.tab = C.pointer(tab)
    if dst_queue is not None:
        q = np.ascontiguousarray(dst_queue, dtype=np.uint64)
        q = q if q.shape[0] else np.zeros(1, np.uint64)
        a.dst_queue = q.ctypes.data
        a._dst_queue = q
    a._tab = tab
    for k, v in kw.items():
        if k not in dict(MoveArgs._fields_) or k in ("tab", "dst_queue"):
            raise TypeError(f"move_args: no field {k}")
        setattr(a, k, v or None if dict(MoveArgs._fields_)[k] is C.c_void_p else int(v))
    return a


def move_out_dict(words):
    """The four uint64 of a mi_cls_move_out_t as a dict."""
    return {k: int(v) for k, v in zip(MOVE_OUT_FIELDS, words)}


def _move_host(L, prefix, handle, args, submit):
    """The host forms of `prefix` (mi_cls_pool_move_host /
    odp_amd_cls_pool_move_host).  submit: the _submit / _wait pair; "ticket":
    the _submit alone, returning the ticket.  Returns the C status otherwise."""
    if submit:
        t = C.c_uint64()
        rc = getattr(L, prefix + "_submit")(handle, C.byref(args), C.byref(t))
        if rc == 0 and submit == "ticket":
            return t.value
        if rc == 0:
            rc = getattr(L, prefix + "_wait")(handle, t.value)
    else:
        rc = getattr(L, prefix)(handle, C.byref(args))
    return rc


# the vector fill (include/mi_cls.h): the kernels' shape (a tile of runs or of
# delivered places, the blocks' bound)
VEC_TILE, VEC_GRID = 1024, 256
VEC_NO_VECTOR = 0xFFFFFFFF      # vfirst of a run that got no vector
EVRUN_DTYPE = np.dtype([("ev_first", "<u4"), ("ev_count", "<u4"), ("pk_enq", "<u4"), ("vfirst", "<u4")])


class VecOut(C.Structure):
    """mi_cls_vec_out_t."""
    _fields_ = [("events", C.c_uint64), ("ev_span", C.c_uint64), ("vectors", C.c_uint64),
                ("in_vectors", C.c_uint64), ("lost", C.c_uint64), ("holes", C.c_uint64),
                ("refused", C.c_uint64), ("truncated", C.c_uint64), ("vec_used", C.c_uint64 * 16)]


VEC_OUT_FIELDS = tuple(f[0] for f in VecOut._fields_[:8])
VEC_OUT_WORDS = C.sizeof(VecOut) // 8


class VecArgs(C.Structure):
    """mi_cls_vec_args_t."""
    _fields_ = [("seq", C.c_void_p), ("runs", C.c_void_p), ("run_out", C.c_void_p), ("ent", C.c_void_p),
                ("vgot", C.c_void_p), ("n", C.c_uint32), ("run_cap", C.c_uint32), ("nvgot", C.c_uint32),
                ("size_off", C.c_uint32), ("tbl_off", C.c_uint32), ("rsv", C.c_uint32),
                ("ent_to_handle", C.c_uint64), ("rtab", C.c_void_p),
                ("vbase", C.c_uint32 * 16), ("vhave", C.c_uint32 * 16), ("vcap", C.c_uint32 * 16),
                ("varena_lo", C.c_uint64), ("varena_bytes", C.c_uint64),
                ("ev", C.c_void_p), ("evr", C.c_void_p), ("lost", C.c_void_p), ("out", C.c_void_p)]


def vec_args(rtab, vbase=(), vhave=(), vcap=(), **kw) -> VecArgs:
    """A mi_cls_vec_args_t: rtab a RunTab (None: NULL), vbase / vhave / vcap
    per slot (shorter sequences are padded with 0), every other field by
    keyword -- pointers as ints (0 / None: NULL).  The table stays alive with
    the returned struct."""
    a = VecArgs()
    if rtab is not None:
        a.rtab = C.addressof(rtab)
    a._rtab = rtab
    for name, v in (("vbase", vbase), ("vhave", vhave), ("vcap", vcap)):
        for k, x in enumerate(v):
            getattr(a, name)[k] = int(x)
    fields = dict(VecArgs._fields_)
    for k, v in kw.items():
        if k not in fields or k in ("rtab", "vbase", "vhave", "vcap"):
            raise TypeError(f"vec_args: no field {k}")
        setattr(a, k, v or None if fields[k] is C.c_void_p else int(v))
    return a


def vec_out_dict(words):
    """The 24 uint64 of a mi_cls_vec_out_t as a dict (vec_used: a list)."""
    w = [int(v) for v in words]
    d = dict(zip(VEC_OUT_FIELDS, w))
    d["vec_used"] = w[8:8 + RUN_VSLOTS]
    return d


def run_out_dict(words):
    """The 24 uint64 of a mi_cls_run_out_t as a dict (vec_need: a list)."""
    w = [int(v) for v in words]
    d = dict(zip(ENQ_OUT_FIELDS + ("nruns", "vectors"), w))
    d["vec_need"] = w[8:8 + RUN_VSLOTS]
    return d


# odp_proto_t, odp_proto_layer_t, odp_proto_chksums_t.all_chksum
PROTO_ETH, PROTO_IPV4, PROTO_IPV6 = 1, 2, 3
LAYER_L2, LAYER_L3, LAYER_L4, LAYER_ALL = 1, 2, 3, 4
CHKSUM_IPV4, CHKSUM_UDP, CHKSUM_TCP, CHKSUM_SCTP = 1, 2, 4, 8


def _load():
    for p in (LIB_MI, LIB_ODP):
        if not os.path.exists(p):
            raise RuntimeError(f"{p} is missing: run __graft_entry__.build() (no CPU fallback)")
    C.CDLL(LIB_MI, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(LIB_ODP)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    sig = {
        "odp_cls_cos_param_init": (None, [C.POINTER(CosParam)]),
        "odp_cls_capability": (i32, [C.POINTER(Capability)]),
        "odp_cls_cos_create": (vp, [C.c_char_p, C.POINTER(CosParam)]),
        "odp_cos_destroy": (i32, [vp]),
        "odp_cos_queue_set": (i32, [vp, vp]),
        "odp_cos_queue": (vp, [vp]),
        "odp_cls_cos_num_queue": (u32, [vp]),
        "odp_cls_cos_queues": (u32, [vp, C.POINTER(vp), u32]),
        "odp_cls_cos_stats": (i32, [vp, C.POINTER(CosStats)]),
        "odp_cls_pmr_param_init": (None, [C.POINTER(PmrParam)]),
        "odp_cls_pmr_create": (vp, [C.POINTER(PmrParam), i32, vp, vp]),
        "odp_cls_pmr_create_opt": (vp, [C.POINTER(PmrCreateOpt), vp, vp]),
        "odp_cls_pmr_destroy": (i32, [vp]),
        "odp_cls_cos_pool_set": (i32, [vp, vp]),
        "odp_cls_cos_pool": (vp, [vp]),
        "odp_cos_to_u64": (C.c_uint64, [vp]),
        "odp_pmr_to_u64": (C.c_uint64, [vp]),
        "odp_cls_print_all": (None, []),
        "odp_pktio_default_cos_set": (i32, [vp, vp]),
        "odp_pktio_error_cos_set": (i32, [vp, vp]),
        "odp_pktio_skip_set": (i32, [vp, u32]),
        "odp_pktio_headroom_set": (i32, [vp, u32]),
        "odp_amd_cls_limits_set": (i32, [u32, u32, u32]),
        "odp_amd_cls_reset": (None, []),
        "odp_amd_cls_pktio_create": (vp, [i32]),
        "odp_amd_cls_pktio_create_multi": (vp, [C.POINTER(i32), i32]),
        "odp_amd_cls_classify_host": (i32, [vp, vp, C.c_size_t, vp, vp, u32, vp, i32]),
        "mi_cls_shard": (i32, [vp, u32, u32, vp]),
        "mi_cls_host_alloc": (vp, [C.c_size_t]),
        "mi_cls_host_free": (None, [vp]),
        "odp_amd_cls_pktio_destroy": (i32, [vp]),
        "odp_amd_cls_compile": (C.c_long, [vp, vp, C.c_size_t]),
        "odp_amd_cls_classify": (i32, [vp, vp, vp, vp, u32, vp, vp]),
        "odp_amd_cls_queue_of": (vp, [u32, u32]),
        "odp_amd_cls_generation": (C.c_uint64, []),
        "odp_amd_cls_pktin_opt_set": (i32, [vp, C.c_uint64]),
        "odp_amd_cls_spec_wait": (i32, [vp]),
        "mi_cls_spec_wait": (i32, [vp]),
        "odp_amd_cls_last_launch": (i32, [vp, C.POINTER(u32), u32]),
        "mi_cls_last_launch": (i32, [vp, C.POINTER(u32), u32]),
        "mi_cls_spec_pending": (i32, [C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        "mi_cls_device_count": (i32, []),
        "mi_cls_ctx_create": (i32, [i32, C.POINTER(vp)]),
        "mi_cls_ctx_destroy": (i32, [vp]),
        "mi_cls_rules_load": (i32, [vp, vp, C.c_size_t, vp]),
        "mi_cls_classify": (i32, [vp, vp, vp, vp, u32, vp, vp]),
        "mi_cls_strerror": (C.c_char_p, [i32]),
        "mi_cls_program_info": (i32, [vp, C.c_size_t, C.POINTER(u32), u32]),
        "mi_cls_chksum_insert": (i32, [vp, vp, vp, vp, vp, u32, C.c_uint64, vp, vp]),
        "mi_cls_chksum_insert_host": (i32, [vp, vp, C.c_size_t, vp, vp, vp, u32, C.c_uint64, vp]),
        "mi_cls_chksum_insert_host_submit": (i32, [vp, vp, C.c_size_t, vp, vp, vp, u32, C.c_uint64, vp,
                                                   C.POINTER(C.c_uint64)]),
        "mi_cls_chksum_insert_host_wait": (i32, [vp, C.c_uint64]),
        "mi_cls_tx_hash": (i32, [vp, vp, vp, vp, vp, u32, C.c_uint64, vp, u32, vp, i32, vp]),
        "mi_cls_tx_hash_host": (i32, [vp, vp, C.c_size_t, vp, vp, vp, u32, C.c_uint64, vp, u32, vp, i32]),
        "mi_cls_tx_hash_host_submit": (i32, [vp, vp, C.c_size_t, vp, vp, vp, u32, C.c_uint64, vp, u32, vp, i32,
                                             C.POINTER(C.c_uint64)]),
        "mi_cls_tx_hash_host_wait": (i32, [vp, C.c_uint64]),
        "mi_cls_parse": (i32, [vp, vp, vp, vp, u32, C.POINTER(ParseParam), vp, vp]),
        "mi_cls_parse_host": (i32, [vp, vp, C.c_size_t, vp, vp, u32, C.POINTER(ParseParam), vp]),
        "mi_cls_parse_host_submit": (i32, [vp, vp, C.c_size_t, vp, vp, u32, C.POINTER(ParseParam), vp,
                                           C.POINTER(C.c_uint64)]),
        "mi_cls_parse_host_wait": (i32, [vp, C.c_uint64]),
        "mi_cls_lso_plan": (i32, [u32, u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]),
        "mi_cls_lso_segment": (i32, [vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, vp]),
        "mi_cls_lso_segment_host": (i32, [vp, vp, C.c_size_t, vp, vp, vp, u32, vp, C.c_size_t, vp, u32, vp,
                                          u32, vp]),
        "mi_cls_lso_segment_host_submit": (i32, [vp, vp, C.c_size_t, vp, vp, vp, u32, vp, C.c_size_t, vp,
                                                 u32, vp, u32, vp, C.POINTER(C.c_uint64)]),
        "mi_cls_lso_segment_host_wait": (i32, [vp, C.c_uint64]),
        "mi_cls_enq_plan": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), vp, vp, vp, vp]),
        "mi_cls_enq_plan_host": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), vp, vp, vp]),
        "mi_cls_enq_plan_host_submit": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), vp, vp, vp,
                                              C.POINTER(C.c_uint64)]),
        "mi_cls_enq_plan_host_wait": (i32, [vp, C.c_uint64]),
        "odp_amd_cls_enqtab_fill": (i32, [C.POINTER(EnqTab), C.POINTER(vp), C.POINTER(u32),
                                          C.POINTER(C.c_uint64)]),
        "odp_amd_cls_enq_plan": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), vp, vp, vp, vp]),
        "odp_amd_cls_enq_plan_host": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), vp, vp, vp]),
        "odp_amd_cls_enq_plan_host_submit": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), vp, vp, vp,
                                                   C.POINTER(C.c_uint64)]),
        "odp_amd_cls_enq_plan_host_wait": (i32, [vp, C.c_uint64]),
        "mi_cls_enq_runs": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), C.POINTER(RunTab), u32, vp, vp, u32, vp,
                                  vp]),
        "mi_cls_enq_runs_host": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), C.POINTER(RunTab), u32, vp, vp, u32,
                                       vp]),
        "mi_cls_enq_runs_host_submit": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), C.POINTER(RunTab), u32, vp, vp,
                                              u32, vp, C.POINTER(C.c_uint64)]),
        "mi_cls_enq_runs_host_wait": (i32, [vp, C.c_uint64]),
        "odp_amd_cls_runtab_fill": (i32, [C.POINTER(RunTab), C.POINTER(vp), C.POINTER(u32),
                                          C.POINTER(C.c_uint64)]),
        "odp_amd_cls_enq_runs": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), C.POINTER(RunTab), u32, vp, vp, u32,
                                       vp, vp]),
        "odp_amd_cls_enq_runs_host": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), C.POINTER(RunTab), u32, vp, vp,
                                            u32, vp]),
        "odp_amd_cls_enq_runs_host_submit": (i32, [vp, vp, vp, u32, C.POINTER(EnqTab), C.POINTER(RunTab), u32, vp,
                                                   vp, u32, vp, C.POINTER(C.c_uint64)]),
        "odp_amd_cls_enq_runs_host_wait": (i32, [vp, C.c_uint64]),
        "mi_cls_pool_plan": (i32, [vp, vp, vp, vp, u32, C.POINTER(PoolTab), vp, vp, vp, vp, vp, vp, vp]),
        "mi_cls_pool_plan_host": (i32, [vp, vp, vp, vp, u32, C.POINTER(PoolTab), vp, vp, vp, vp, vp, vp]),
        "mi_cls_pool_plan_host_submit": (i32, [vp, vp, vp, vp, u32, C.POINTER(PoolTab), vp, vp, vp, vp, vp, vp,
                                               C.POINTER(C.c_uint64)]),
        "mi_cls_pool_plan_host_wait": (i32, [vp, C.c_uint64]),
        "odp_amd_cls_pooltab_cos": (i32, [vp, C.POINTER(PoolTab), C.POINTER(vp), C.POINTER(u32),
                                          C.POINTER(C.c_uint64)]),
        "odp_amd_cls_pool_plan": (i32, [vp, vp, vp, vp, u32, C.POINTER(PoolTab), vp, vp, vp, vp, vp, vp, vp]),
        "odp_amd_cls_pool_plan_host": (i32, [vp, vp, vp, vp, u32, C.POINTER(PoolTab), vp, vp, vp, vp, vp, vp]),
        "odp_amd_cls_pool_plan_host_submit": (i32, [vp, vp, vp, vp, u32, C.POINTER(PoolTab), vp, vp, vp, vp, vp,
                                                    vp, C.POINTER(C.c_uint64)]),
        "odp_amd_cls_pool_plan_host_wait": (i32, [vp, C.c_uint64]),
        "mi_cls_pool_move": (i32, [vp, C.POINTER(MoveArgs), vp]),
        "mi_cls_pool_move_host": (i32, [vp, C.POINTER(MoveArgs)]),
        "mi_cls_pool_move_host_submit": (i32, [vp, C.POINTER(MoveArgs), C.POINTER(C.c_uint64)]),
        "mi_cls_pool_move_host_wait": (i32, [vp, C.c_uint64]),
        "odp_amd_cls_pool_move": (i32, [vp, C.POINTER(MoveArgs), vp]),
        "odp_amd_cls_pool_move_host": (i32, [vp, C.POINTER(MoveArgs)]),
        "odp_amd_cls_pool_move_host_submit": (i32, [vp, C.POINTER(MoveArgs), C.POINTER(C.c_uint64)]),
        "odp_amd_cls_pool_move_host_wait": (i32, [vp, C.c_uint64]),
        "odp_amd_cls_pool_move_geom": (i32, [C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint64)]),
        "mi_cls_vec_fill": (i32, [vp, C.POINTER(VecArgs), vp]),
        "mi_cls_vec_fill_host": (i32, [vp, C.POINTER(VecArgs)]),
        "mi_cls_vec_fill_host_submit": (i32, [vp, C.POINTER(VecArgs), C.POINTER(C.c_uint64)]),
        "mi_cls_vec_fill_host_wait": (i32, [vp, C.c_uint64]),
        "odp_amd_cls_vec_fill": (i32, [vp, C.POINTER(VecArgs), vp]),
        "odp_amd_cls_vec_fill_host": (i32, [vp, C.POINTER(VecArgs)]),
        "odp_amd_cls_vec_fill_host_submit": (i32, [vp, C.POINTER(VecArgs), C.POINTER(C.c_uint64)]),
        "odp_amd_cls_vec_fill_host_wait": (i32, [vp, C.c_uint64]),
        "odp_amd_cls_vec_geom": (i32, [C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]),
        "odp_amd_cls_parse_host": (i32, [vp, C.c_size_t, vp, vp, u32, u32, u32, u32, vp]),
        "odp_amd_cls_parse_term": (None, []),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return lib


_lib = None


def shard(lens: np.ndarray, nshards: int) -> np.ndarray:
    """mi_cls_shard: begin[0..nshards] of contiguous slices balanced by
    header-window bytes (the product's multi-GPU cut; host only)."""
    ln = np.ascontiguousarray(lens, dtype=np.uint16)
    begin = np.zeros(nshards + 1, dtype=np.uint32)
    rc = lib().mi_cls_shard(ln.ctypes.data, int(ln.shape[0]), nshards, begin.ctypes.data)
    if rc:
        raise RuntimeError(f"mi_cls_shard: {rc}")
    return begin


class PinnedArray:
    """numpy view of page-locked host memory from mi_cls_host_alloc
    (hipHostMalloc): the GPU reads and writes it in place (zero copy)."""

    def __init__(self, nbytes: int):
        self.ptr = lib().mi_cls_host_alloc(max(1, nbytes))
        if not self.ptr:
            raise MemoryError("mi_cls_host_alloc failed")
        self.nbytes = nbytes
        self.u8 = np.ctypeslib.as_array((C.c_uint8 * max(1, nbytes)).from_address(self.ptr))

    def view(self, dtype, count=None):
        a = self.u8.view(dtype)
        return a if count is None else a[:count]

    def close(self):
        if self.ptr:
            lib().mi_cls_host_free(self.ptr)
            self.ptr = None


def spec_pending() -> dict:
    """Specialised-kernel compiler state (mi_cls_spec_pending)."""
    r, q, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    active = lib().mi_cls_spec_pending(C.byref(r), C.byref(q), C.byref(c))
    return {"active": bool(active), "running": r.value, "queued": q.value, "cached": c.value}


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def _h(x):
    return x or 0


# mi_cls_tx_desc_t (include/mi_cls.h): l3, l4, flags (bit 0 l3_chksum_set,
# 1 l3_chksum, 2 l4_chksum_set, 3 l4_chksum; for mi_cls_tx_hash bits 4-7: the
# packet has UDP / TCP / IPv4 / IPv6)
TX_DESC_DTYPE = np.dtype([("l3", "<u2"), ("l4", "<u2"), ("flags", "u1"), ("rsv", "u1", (3,))])


class _FeatureContext:
    """A device context of one offload (checksum insertion, parse, LSO): its
    own stream, staging buffers and ticket ring; needs no rules."""

    def __init__(self, gpu: int = 0):
        self.L = lib()
        self.gpu = gpu
        ctx = C.c_void_p()
        rc = self.L.mi_cls_ctx_create(gpu, C.byref(ctx))
        if rc:
            raise RuntimeError(f"mi_cls_ctx_create: {rc} ({self.L.mi_cls_strerror(rc).decode()})")
        self.ctx = ctx

    def close(self):
        if self.ctx:
            self.L.mi_cls_ctx_destroy(self.ctx)
            self.ctx = None

    def last_launch(self):
        info = (C.c_uint32 * 7)()
        self.L.mi_cls_last_launch(self.ctx, info, 7)
        return list(info)


class TxContext(_FeatureContext):
    """A device context for pktout checksum insertion (mi_cls_chksum_insert
    and its host entries); needs no rules."""

    def insert_device(self, d_buf, d_off, d_len, d_desc, n, opt, d_done=0, stream=0):
        """On device pointers (ints), stream-ordered.  Returns the C status."""
        return self.L.mi_cls_chksum_insert(self.ctx, d_buf, d_off, d_len, d_desc, n, int(opt),
                                           d_done or None, stream or None)

    def insert(self, batch, desc, opt, device="cuda:0"):
        """Upload a pktgen.Batch and its descriptors (TX_DESC_DTYPE), insert
        the checksums, return (buffer bytes, done bytes) as numpy arrays."""
        import torch
        dev = torch.device(device)
        n = batch.n
        desc = np.ascontiguousarray(desc, dtype=TX_DESC_DTYPE)
        assert desc.shape[0] == n
        t_buf = torch.from_numpy(np.ascontiguousarray(batch.buf)).to(dev)
        t_off = torch.from_numpy(batch.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(batch.len.astype(np.uint16).view(np.int16)).to(dev)
        t_desc = torch.from_numpy(desc.view(np.int64).copy() if n else np.zeros(1, np.int64)).to(dev)
        t_done = torch.zeros(max(1, n), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.insert_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(),
                                t_desc.data_ptr(), n, opt, t_done.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"mi_cls_chksum_insert: {rc} ({self.L.mi_cls_strerror(rc).decode()})")
        torch.cuda.synchronize(dev)
        return t_buf.cpu().numpy(), t_done.cpu().numpy()[:n]

    def insert_host(self, buf, off, ln, desc, opt, done=None, submit=False):
        """mi_cls_chksum_insert_host on numpy arrays (views of a PinnedArray
        are worked on in place, other arrays go through the staging
        buffers); buf is modified.  submit: the _submit / _wait pair."""
        n = int(off.shape[0])
        args = (self.ctx, buf.ctypes.data, buf.nbytes, off.ctypes.data, ln.ctypes.data,
                desc.ctypes.data, n, int(opt), done.ctypes.data if done is not None else None)
        if submit:
            t = C.c_uint64()
            rc = self.L.mi_cls_chksum_insert_host_submit(*args, C.byref(t))
            if rc == 0:
                rc = self.L.mi_cls_chksum_insert_host_wait(self.ctx, t.value)
        else:
            rc = self.L.mi_cls_chksum_insert_host(*args)
        if rc != 0:
            raise RuntimeError(f"mi_cls_chksum_insert_host: {rc}")


    def hash_device(self, d_buf, d_off, d_len, d_desc, n, opt, d_done, hash_proto, d_hash, chksum, stream=0):
        """mi_cls_tx_hash on device pointers (ints), stream-ordered.  Returns
        the C status."""
        return self.L.mi_cls_tx_hash(self.ctx, d_buf, d_off, d_len, d_desc, n, int(opt), d_done or None,
                                     int(hash_proto), d_hash, int(bool(chksum)), stream or None)

    def hash(self, batch, desc, hash_proto, opt=0, chksum=False, device="cuda:0", poison=0xA5A5A5A5):
        """mi_cls_tx_hash: the pktin flow hash of every packet (pktio/loop.c
        get_dest_queue before its modulo) under hash_proto
        (odp_pktin_hash_proto_t.all_bits), from the descriptors' flag bits
        4-7 and offsets; chksum: the same launch also inserts the checksums
        as insert() does.  The hash words hold `poison` before the launch.
        Returns (buffer bytes, done bytes, hash words)."""
        import torch
        dev = torch.device(device)
        n = batch.n
        desc = np.ascontiguousarray(desc, dtype=TX_DESC_DTYPE)
        assert desc.shape[0] == n
        t_buf = torch.from_numpy(np.ascontiguousarray(batch.buf)).to(dev)
        t_off = torch.from_numpy(batch.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(batch.len.astype(np.uint16).view(np.int16)).to(dev)
        t_desc = torch.from_numpy(desc.view(np.int64).copy() if n else np.zeros(1, np.int64)).to(dev)
        t_done = torch.full((max(1, n),), 0xEE, dtype=torch.uint8, device=dev)
        t_hash = torch.from_numpy(np.full(max(1, n) + 1, poison, np.uint32).view(np.int32)).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.hash_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), t_desc.data_ptr(), n,
                              opt, t_done.data_ptr(), hash_proto, t_hash.data_ptr(), chksum, stream)
        if rc != 0:
            raise RuntimeError(f"mi_cls_tx_hash: {rc} ({self.L.mi_cls_strerror(rc).decode()})")
        torch.cuda.synchronize(dev)
        h = t_hash.cpu().numpy().view(np.uint32)
        if h[n] != poison:
            raise RuntimeError("mi_cls_tx_hash wrote past its n hash words")
        return t_buf.cpu().numpy(), t_done.cpu().numpy()[:n], h[:n].copy()

    def hash_host(self, buf, off, ln, desc, hash_proto, hash_out, opt=0, chksum=False, done=None,
                  submit=False):
        """mi_cls_tx_hash_host on numpy arrays, as insert_host; hash_out
        (uint32, n words) receives the hashes."""
        n = int(off.shape[0])
        args = (self.ctx, buf.ctypes.data, buf.nbytes, off.ctypes.data, ln.ctypes.data,
                desc.ctypes.data, n, int(opt), done.ctypes.data if done is not None else None,
                int(hash_proto), hash_out.ctypes.data, int(bool(chksum)))
        if submit:
            t = C.c_uint64()
            rc = self.L.mi_cls_tx_hash_host_submit(*args, C.byref(t))
            if rc == 0:
                rc = self.L.mi_cls_tx_hash_host_wait(self.ctx, t.value)
        else:
            rc = self.L.mi_cls_tx_hash_host(*args)
        if rc != 0:
            raise RuntimeError(f"mi_cls_tx_hash_host: {rc}")


def chksum_insert(batch, desc, opt, gpu: int = 0):
    """pktout checksum insertion of a pktgen.Batch on the GPU
    (mi_cls_chksum_insert): desc is an array of TX_DESC_DTYPE (the packets'
    l3 / l4 offsets and override flags), opt the
    odp_pktout_config_opt_t.all_bits.  Returns (buffer bytes, done bytes)."""
    c = TxContext(gpu)
    try:
        return c.insert(batch, desc, opt, device=f"cuda:{gpu}")
    finally:
        c.close()


class ParseContext(_FeatureContext):
    """A device context for the parse on its own (mi_cls_parse and its host
    entries: odp_packet_parse for a batch); needs no rules."""

    def parse_device(self, d_buf, d_off, d_len, n, proto, last_layer, chksums, d_out, stream=0):
        """On device pointers (ints), stream-ordered.  Returns the C status."""
        pp = ParseParam(proto, last_layer, chksums)
        return self.L.mi_cls_parse(self.ctx, d_buf, d_off, d_len, n, C.byref(pp), d_out, stream or None)

    def parse(self, batch, proto=PROTO_ETH, last_layer=LAYER_ALL, chksums=0):
        """Upload a pktgen.Batch (off[i]: where packet i's parse starts,
        len[i]: its frame length less the parse offset), parse it, return the
        records (rules.RESULT_DTYPE)."""
        import torch
        dev = torch.device(f"cuda:{self.gpu}")
        n = batch.n
        t_buf = torch.from_numpy(np.ascontiguousarray(batch.buf)).to(dev)
        t_off = torch.from_numpy(batch.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(batch.len.astype(np.uint16).view(np.int16)).to(dev)
        t_out = torch.zeros((max(1, n), 16), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.parse_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, proto,
                               last_layer, chksums, t_out.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"mi_cls_parse: {rc} ({self.L.mi_cls_strerror(rc).decode()})")
        torch.cuda.synchronize(dev)
        return t_out.cpu().numpy().reshape(-1).view(R.RESULT_DTYPE)[:n].copy()

    def parse_host(self, buf, off, ln, out, proto=PROTO_ETH, last_layer=LAYER_ALL, chksums=0):
        """mi_cls_parse_host on numpy arrays (views of a PinnedArray are read
        and written in place, other arrays go through the staging buffers)."""
        pp = ParseParam(proto, last_layer, chksums)
        rc = self.L.mi_cls_parse_host(self.ctx, buf.ctypes.data, buf.nbytes, off.ctypes.data,
                                      ln.ctypes.data, int(off.shape[0]), C.byref(pp), out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"mi_cls_parse_host: {rc}")

    def submit_host(self, buf, off, ln, out, proto=PROTO_ETH, last_layer=LAYER_ALL, chksums=0):
        """mi_cls_parse_host_submit: returns the ticket for wait()."""
        pp = ParseParam(proto, last_layer, chksums)
        t = C.c_uint64()
        rc = self.L.mi_cls_parse_host_submit(self.ctx, buf.ctypes.data, buf.nbytes, off.ctypes.data,
                                             ln.ctypes.data, int(off.shape[0]), C.byref(pp),
                                             out.ctypes.data, C.byref(t))
        if rc != 0:
            raise RuntimeError(f"mi_cls_parse_host_submit: {rc}")
        return t.value

    def wait(self, ticket):
        rc = self.L.mi_cls_parse_host_wait(self.ctx, ticket)
        if rc != 0:
            raise RuntimeError(f"mi_cls_parse_host_wait: {rc}")


def _enq_plan_device(call, handle, records, lens, tab, device, poison=0xA5A5A5A5):
    """Upload records (rules.RESULT_DTYPE) and lens, run the device form
    `call` (mi_cls_enq_plan / odp_amd_cls_enq_plan) on torch's current stream
    and return (perm, gbeg, counters dict).  Every output word, and one guard
    word past each array, holds `poison` before the launch."""
    import torch
    dev = torch.device(device)
    rec = np.ascontiguousarray(records, dtype=R.RESULT_DTYPE)
    n = int(rec.shape[0])
    ln = np.ascontiguousarray(lens, dtype=np.uint16)
    assert ln.shape[0] == n
    ng = int(tab.ndst) + 2
    t_res = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy() if n else np.zeros(16, np.uint8)).to(dev)
    t_len = torch.from_numpy(ln.view(np.int16).copy() if n else np.zeros(1, np.int16)).to(dev)
    t_perm = torch.from_numpy(np.full(n + 1, poison, np.uint32).view(np.int32)).to(dev)
    t_gbeg = torch.from_numpy(np.full(ng + 1, poison, np.uint32).view(np.int32)).to(dev)
    t_out = torch.from_numpy(np.full(2 * (len(ENQ_OUT_FIELDS) + 1), poison, np.uint32).view(np.int32)).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = call(handle, t_res.data_ptr(), t_len.data_ptr(), n, C.byref(tab), t_perm.data_ptr(),
              t_gbeg.data_ptr(), t_out.data_ptr(), stream or None)
    if rc != 0:
        raise RuntimeError(f"enq_plan: {rc} ({lib().mi_cls_strerror(rc).decode()})")
    torch.cuda.synchronize(dev)
    perm = t_perm.cpu().numpy().view(np.uint32)
    gbeg = t_gbeg.cpu().numpy().view(np.uint32)
    out = t_out.cpu().numpy().view(np.uint32)
    if perm[n] != poison or gbeg[ng] != poison or out[-1] != poison or out[-2] != poison:
        raise RuntimeError("enq_plan wrote past an output array")
    ctr = out[:-2].view(np.uint64)
    return perm[:n].copy(), gbeg[:ng].copy(), {k: int(v) for k, v in zip(ENQ_OUT_FIELDS, ctr)}


def _enq_plan_host(L, prefix, handle, res, ln, tab, perm, gbeg, out, submit):
    """The host forms of `prefix` (mi_cls_enq_plan_host / odp_amd_cls_enq_plan_host)
    on numpy arrays: views of a PinnedArray are read and written in place,
    other arrays go through the staging buffers.  out: 6 uint64
    (ENQ_OUT_FIELDS).  submit: the _submit / _wait pair."""
    n = int(res.shape[0])
    args = (handle, res.ctypes.data if n else None, ln.ctypes.data if n else None, n, C.byref(tab),
            perm.ctypes.data if n else None, gbeg.ctypes.data, out.ctypes.data)
    if submit:
        t = C.c_uint64()
        rc = getattr(L, prefix + "_submit")(*args, C.byref(t))
        if rc == 0:
            rc = getattr(L, prefix + "_wait")(handle, t.value)
    else:
        rc = getattr(L, prefix)(*args)
    if rc != 0:
        raise RuntimeError(f"{prefix}: {rc}")


def _enq_runs_device(call, handle, records, lens, tab, rtab, burst, run_cap, device, poison=0xA5A5A5A5):
    """Upload records and lens, run the device form `call` (mi_cls_enq_runs /
    odp_amd_cls_enq_runs) on torch's current stream and return (seq, runs,
    out): runs all run_cap entries (RUN_DTYPE; those the call left alone still
    hold `poison`), out the dict of run_out_dict.  Every output word, and a
    guard past each array, holds `poison` before the launch."""
    import torch
    dev = torch.device(device)
    rec = np.ascontiguousarray(records, dtype=R.RESULT_DTYPE)
    n = int(rec.shape[0])
    ln = np.ascontiguousarray(lens, dtype=np.uint16)
    assert ln.shape[0] == n
    t_res = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy() if n else np.zeros(16, np.uint8)).to(dev)
    t_len = torch.from_numpy(ln.view(np.int16).copy() if n else np.zeros(1, np.int16)).to(dev)
    t_seq = torch.from_numpy(np.full(n + 1, poison, np.uint32).view(np.int32)).to(dev)
    t_runs = torch.from_numpy(np.full(4 * (run_cap + 1), poison, np.uint32).view(np.int32)).to(dev)
    t_out = torch.from_numpy(np.full(2 * (RUN_OUT_WORDS + 1), poison, np.uint32).view(np.int32)).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = call(handle, t_res.data_ptr(), t_len.data_ptr(), n, C.byref(tab), C.byref(rtab), burst,
              t_seq.data_ptr(), t_runs.data_ptr(), run_cap, t_out.data_ptr(), stream or None)
    if rc != 0:
        raise RuntimeError(f"enq_runs: {rc} ({lib().mi_cls_strerror(rc).decode()})")
    torch.cuda.synchronize(dev)
    seq = t_seq.cpu().numpy().view(np.uint32)
    runs = t_runs.cpu().numpy().view(np.uint32)
    out = t_out.cpu().numpy().view(np.uint32)
    if seq[n] != poison or np.any(runs[4 * run_cap:] != poison) or out[-1] != poison or out[-2] != poison:
        raise RuntimeError("enq_runs wrote past an output array")
    return seq[:n].copy(), runs[:4 * run_cap].copy().view(RUN_DTYPE), run_out_dict(out[:-2].view(np.uint64))


def _enq_runs_host(L, prefix, handle, res, ln, tab, rtab, burst, seq, runs, out, submit):
    """The host forms of `prefix` (mi_cls_enq_runs_host /
    odp_amd_cls_enq_runs_host) on numpy arrays, as _enq_plan_host.  runs:
    RUN_DTYPE, its length the run_cap; out: 24 uint64."""
    n = int(res.shape[0])
    cap = int(runs.shape[0])
    args = (handle, res.ctypes.data if n else None, ln.ctypes.data if n else None, n, C.byref(tab),
            C.byref(rtab), burst, seq.ctypes.data if n else None, runs.ctypes.data if cap else None, cap,
            out.ctypes.data)
    if submit:
        t = C.c_uint64()
        rc = getattr(L, prefix + "_submit")(*args, C.byref(t))
        if rc == 0:
            rc = getattr(L, prefix + "_wait")(handle, t.value)
    else:
        rc = getattr(L, prefix)(*args)
    if rc != 0:
        raise RuntimeError(f"{prefix}: {rc}")


def _pool_plan_device(call, handle, records, lens, own, tab, have, base, device, poison=0xA5A5A5A5,
                      in_place=False):
    """Upload records, lens and own (None: NULL), run the device form `call`
    (mi_cls_pool_plan / odp_amd_cls_pool_plan) on torch's current stream and
    return (res_out, dec, idx, out): res_out as rules.RESULT_DTYPE, out the dict
    of pool_out_dict.  Every output word, and a guard past each array, holds
    `poison` before the launch.  in_place: res_out is the uploaded records' own
    array (a guard record follows it)."""
    import torch
    dev = torch.device(device)
    rec = np.ascontiguousarray(records, dtype=R.RESULT_DTYPE)
    n = int(rec.shape[0])
    ln = np.ascontiguousarray(lens, dtype=np.uint16)
    assert ln.shape[0] == n
    up = np.full(4 * (n + 1), poison, np.uint32)
    up[:4 * n] = rec.view(np.uint32).reshape(-1)
    t_res = torch.from_numpy(up.view(np.int32)).to(dev)
    t_len = torch.from_numpy(ln.view(np.int16).copy() if n else np.zeros(1, np.int16)).to(dev)
    t_own = None
    if own is not None:
        ow = np.ascontiguousarray(own, dtype=np.uint8)
        assert ow.shape[0] == n
        t_own = torch.from_numpy(ow.copy() if n else np.zeros(1, np.uint8)).to(dev)
    t_ro = t_res if in_place else torch.from_numpy(np.full(4 * (n + 1), poison, np.uint32).view(np.int32)).to(dev)
    t_dec = torch.from_numpy(np.full(n + 1, poison, np.uint32).view(np.int32)).to(dev)
    t_idx = torch.from_numpy(np.full(n + 1, poison, np.uint32).view(np.int32)).to(dev)
    t_out = torch.from_numpy(np.full(POOL_OUT_WORDS + 2, poison, np.uint32).view(np.int32)).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    h, b = _pool_u32x16(have), _pool_u32x16(base)
    rc = call(handle, t_res.data_ptr(), t_len.data_ptr(), t_own.data_ptr() if t_own is not None else None, n,
              C.byref(tab), h, b, t_ro.data_ptr(), t_dec.data_ptr(), t_idx.data_ptr(), t_out.data_ptr(),
              stream or None)
    if rc != 0:
        raise RuntimeError(f"pool_plan: {rc} ({lib().mi_cls_strerror(rc).decode()})")
    torch.cuda.synchronize(dev)
    ro = t_ro.cpu().numpy().view(np.uint32)
    dec = t_dec.cpu().numpy().view(np.uint32)
    idx = t_idx.cpu().numpy().view(np.uint32)
    out = t_out.cpu().numpy().view(np.uint32)
    if np.any(ro[4 * n:] != poison) or dec[n] != poison or idx[n] != poison or np.any(out[-2:] != poison):
        raise RuntimeError("pool_plan wrote past an output array")
    if not in_place and not np.array_equal(t_res.cpu().numpy().view(np.uint32), up):
        raise RuntimeError("pool_plan wrote its input records")
    return ro[:4 * n].copy().view(R.RESULT_DTYPE), dec[:n].copy(), idx[:n].copy(), pool_out_dict(out[:-2])


def _pool_plan_host(L, prefix, handle, res, ln, own, tab, have, base, res_out, dec, idx, out, submit):
    """The host forms of `prefix` (mi_cls_pool_plan_host /
    odp_amd_cls_pool_plan_host) on numpy arrays, as _enq_plan_host.  own: None
    for NULL; out: POOL_OUT_DTYPE (one element) or its 40 uint32.  submit: the
    _submit / _wait pair; "ticket": the _submit alone, returning the ticket."""
    n = int(res.shape[0])
    args = (handle, res.ctypes.data if n else None, ln.ctypes.data if n else None,
            own.ctypes.data if n and own is not None else None, n, C.byref(tab), _pool_u32x16(have),
            _pool_u32x16(base), res_out.ctypes.data if n else None, dec.ctypes.data if n else None,
            idx.ctypes.data if n else None, out.ctypes.data)
    if submit:
        t = C.c_uint64()
        rc = getattr(L, prefix + "_submit")(*args, C.byref(t))
        if rc == 0 and submit == "ticket":
            return t.value
        if rc == 0:
            rc = getattr(L, prefix + "_wait")(handle, t.value)
    else:
        rc = getattr(L, prefix)(*args)
    if rc != 0:
        raise RuntimeError(f"{prefix}: {rc}")
    return None


class EnqContext(_FeatureContext):
    """A device context for the enqueue plan (mi_cls_enq_plan and its host
    entries: a classified batch's records grouped by destination queue, the
    records that are not delivered, the pktio counters) and the run plan
    (mi_cls_enq_runs: the same batch cut into the reference's runs, with the
    packet-vector counts); needs no rules."""

    def runs_device(self, d_res, d_len, n, tab, rtab, burst, d_seq, d_runs, run_cap, d_out, stream=0):
        """mi_cls_enq_runs on device pointers (ints), stream-ordered.  Returns
        the C status."""
        return self.L.mi_cls_enq_runs(self.ctx, d_res or None, d_len or None, n, C.byref(tab), C.byref(rtab),
                                      burst, d_seq or None, d_runs or None, run_cap, d_out or None,
                                      stream or None)

    def runs(self, records, lens, tab, rtab, burst=0, run_cap=None, poison=0xA5A5A5A5):
        """Upload records and lens, plan the runs; returns (seq, runs, out)
        (run_cap: room for every run by default)."""
        cap = len(records) if run_cap is None else run_cap
        return _enq_runs_device(self.L.mi_cls_enq_runs, self.ctx, records, lens, tab, rtab, burst, cap,
                                f"cuda:{self.gpu}", poison)

    def runs_host(self, res, ln, tab, rtab, burst, seq, runs, out, submit=False):
        """mi_cls_enq_runs_host (submit: _host_submit / _host_wait)."""
        _enq_runs_host(self.L, "mi_cls_enq_runs_host", self.ctx, res, ln, tab, rtab, burst, seq, runs, out,
                       submit)

    def pools_device(self, d_res, d_len, d_own, n, tab, have, base, d_res_out, d_dec, d_idx, d_out, stream=0):
        """mi_cls_pool_plan on device pointers (ints), stream-ordered.  Returns
        the C status."""
        return self.L.mi_cls_pool_plan(self.ctx, d_res or None, d_len or None, d_own or None, n, C.byref(tab),
                                       _pool_u32x16(have), _pool_u32x16(base), d_res_out or None,
                                       d_dec or None, d_idx or None, d_out or None, stream or None)

    def pools(self, records, lens, own, tab, have, base, poison=0xA5A5A5A5, in_place=False):
        """Upload records, lens and own (None: no frame has a packet), plan the
        pools (mi_cls_pool_plan); returns (res_out, dec, idx, out)."""
        return _pool_plan_device(self.L.mi_cls_pool_plan, self.ctx, records, lens, own, tab, have, base,
                                 f"cuda:{self.gpu}", poison, in_place)

    def pools_host(self, res, ln, own, tab, have, base, res_out, dec, idx, out, submit=False):
        """mi_cls_pool_plan_host (submit: _host_submit / _host_wait; "ticket":
        _host_submit alone, returns the ticket for pools_wait)."""
        return _pool_plan_host(self.L, "mi_cls_pool_plan_host", self.ctx, res, ln, own, tab, have, base, res_out,
                               dec, idx, out, submit)

    def pools_wait(self, ticket):
        rc = self.L.mi_cls_pool_plan_host_wait(self.ctx, ticket)
        if rc != 0:
            raise RuntimeError(f"mi_cls_pool_plan_host_wait: {rc}")

    def move_device(self, args, stream=0):
        """mi_cls_pool_move on a MoveArgs of device pointers, stream-ordered.
        Returns the C status."""
        return self.L.mi_cls_pool_move(self.ctx, C.byref(args), stream or None)

    def move(self, args):
        """mi_cls_pool_move on torch's current stream, waited for."""
        import torch
        dev = torch.device(f"cuda:{self.gpu}")
        rc = self.move_device(args, torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"mi_cls_pool_move: {rc} ({lib().mi_cls_strerror(rc).decode()})")
        torch.cuda.synchronize(dev)

    def move_host(self, args, submit=False):
        """mi_cls_pool_move_host on a MoveArgs of host pointers (submit: the
        _host_submit / _host_wait pair; "ticket": _host_submit alone, returns
        the ticket for move_wait).  Returns the C status."""
        return _move_host(self.L, "mi_cls_pool_move_host", self.ctx, args, submit)

    def move_wait(self, ticket):
        rc = self.L.mi_cls_pool_move_host_wait(self.ctx, ticket)
        if rc != 0:
            raise RuntimeError(f"mi_cls_pool_move_host_wait: {rc}")

    def fill_device(self, args, stream=0):
        """mi_cls_vec_fill on a VecArgs of device pointers, stream-ordered.
        Returns the C status."""
        return self.L.mi_cls_vec_fill(self.ctx, C.byref(args), stream or None)

    def fill(self, args):
        """mi_cls_vec_fill on torch's current stream, waited for."""
        import torch
        dev = torch.device(f"cuda:{self.gpu}")
        rc = self.fill_device(args, torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"mi_cls_vec_fill: {rc} ({lib().mi_cls_strerror(rc).decode()})")
        torch.cuda.synchronize(dev)

    def fill_host(self, args, submit=False):
        """mi_cls_vec_fill_host on a VecArgs of host pointers (submit: the
        _submit / _wait pair; "ticket": the _submit alone, returning the
        ticket for fill_wait).  Returns the C status."""
        return _move_host(self.L, "mi_cls_vec_fill_host", self.ctx, args, submit)

    def fill_wait(self, ticket):
        rc = self.L.mi_cls_vec_fill_host_wait(self.ctx, ticket)
        if rc != 0:
            raise RuntimeError(f"mi_cls_vec_fill_host_wait: {rc}")

    def plan_device(self, d_res, d_len, n, tab, d_perm, d_gbeg, d_out, stream=0):
        """On device pointers (ints), stream-ordered.  Returns the C status."""
        return self.L.mi_cls_enq_plan(self.ctx, d_res or None, d_len or None, n, C.byref(tab),
                                      d_perm or None, d_gbeg or None, d_out or None, stream or None)

    def plan(self, records, lens, tab, poison=0xA5A5A5A5):
        """Upload records and lens, plan; returns (perm, gbeg, counters)."""
        return _enq_plan_device(self.L.mi_cls_enq_plan, self.ctx, records, lens, tab, f"cuda:{self.gpu}",
                                poison)

    def plan_host(self, res, ln, tab, perm, gbeg, out, submit=False):
        """mi_cls_enq_plan_host (submit: _host_submit / _host_wait)."""
        _enq_plan_host(self.L, "mi_cls_enq_plan_host", self.ctx, res, ln, tab, perm, gbeg, out, submit)


# LSO (include/mi_cls.h): odp_lso_protocol_t / odp_lso_modify_t values, the
# per-source descriptor, the segment table entry, st[] values
LSO_PROTO_CUSTOM, LSO_PROTO_IPV4 = 1, 2
LSO_ADD_SEGMENT_NUM, LSO_WRITE_BITS = 1, 5
LSO_L3_INVALID = 0xFFFF
LSO_ST_OK, LSO_ST_IHL, LSO_ST_FIELD, LSO_ST_DESC = 0, 1, 2, 3
LSO_DESC_DTYPE = np.dtype([("hdr_len", "<u2"), ("seg_payload", "<u2"), ("l3", "<u2"), ("profile", "u1"),
                           ("nseg", "u1"), ("first_seg", "<u4"), ("rsv", "<u4")])
LSO_SEG_DTYPE = np.dtype([("off", "<u4"), ("src", "<u4")])


class LsoField(C.Structure):
    """mi_cls_lso_field_t."""
    _fields_ = [("mod_op", C.c_uint8), ("offset", C.c_uint8), ("size", C.c_uint8), ("rsv", C.c_uint8),
                ("mask", C.c_uint8 * 3), ("value", C.c_uint8 * 3), ("rsv2", C.c_uint8 * 2)]


class LsoProfile(C.Structure):
    """mi_cls_lso_profile_t."""
    _fields_ = [("proto", C.c_uint8), ("num_custom", C.c_uint8), ("rsv", C.c_uint8 * 2),
                ("field", LsoField * 8)]


def lso_profiles(profiles):
    """A profile table for LsoContext from [(proto, [field, ...])]; a field is
    (LSO_ADD_SEGMENT_NUM, offset, size) or (LSO_WRITE_BITS, offset, 1,
    (first, middle, last) masks, (first, middle, last) values)."""
    arr = (LsoProfile * max(1, len(profiles)))()
    for p, (proto, fields) in zip(arr, profiles):
        p.proto = proto
        p.num_custom = len(fields)
        for f, spec in zip(p.field, fields):   # more than 8: num_custom tells, the C side rejects
            f.mod_op, f.offset, f.size = spec[0], spec[1], spec[2]
            if len(spec) > 3:
                f.mask[:] = spec[3]
                f.value[:] = spec[4]
    return arr


def lso_plan(length, hdr_len, max_payload, proto, l3=LSO_L3_INVALID):
    """mi_cls_lso_plan (host only): (segments, payload per segment, left-over)
    or (negative errno, 0, 0)."""
    pay, left = C.c_uint32(), C.c_uint32()
    rc = lib().mi_cls_lso_plan(length, hdr_len, max_payload, proto, l3, C.byref(pay), C.byref(left))
    return (rc, pay.value, left.value) if rc > 0 else (rc, 0, 0)


class LsoContext(_FeatureContext):
    """A device context for the LSO segmentation (mi_cls_lso_segment and its
    host entries); needs no rules."""

    plan = staticmethod(lso_plan)

    def segment_device(self, d_src, d_off, d_len, d_desc, n, d_dst, d_seg, nsegs, prof, d_st, stream=0):
        """On device pointers (ints), stream-ordered; prof: lso_profiles().
        Returns the C status."""
        return self.L.mi_cls_lso_segment(self.ctx, d_src, d_off, d_len, d_desc, n, d_dst, d_seg, nsegs,
                                         C.cast(prof, C.c_void_p), len(prof), d_st, stream or None)

    def segment(self, buf, off, ln, desc, seg, prof):
        """Upload one buffer holding the sources and room for the segments,
        its descriptors (LSO_DESC_DTYPE) and segment table (LSO_SEG_DTYPE),
        segment in place, return (buffer bytes, st bytes) as numpy arrays."""
        import torch
        dev = torch.device(f"cuda:{self.gpu}")
        n, nsegs = int(len(desc)), int(len(seg))
        desc = np.ascontiguousarray(desc, dtype=LSO_DESC_DTYPE)
        seg = np.ascontiguousarray(seg, dtype=LSO_SEG_DTYPE)
        t_buf = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
        t_off = torch.from_numpy(np.asarray(off, np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(np.asarray(ln, np.uint16).view(np.int16)).to(dev)
        t_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1, 16).copy() if n
                                  else np.zeros((1, 16), np.uint8)).to(dev)
        t_seg = torch.from_numpy(seg.view(np.int64).copy() if nsegs else np.zeros(1, np.int64)).to(dev)
        t_st = torch.full((max(1, n),), 0xEE, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.segment_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), t_desc.data_ptr(), n,
                                 t_buf.data_ptr(), t_seg.data_ptr(), nsegs, prof, t_st.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"mi_cls_lso_segment: {rc} ({self.L.mi_cls_strerror(rc).decode()})")
        torch.cuda.synchronize(dev)
        return t_buf.cpu().numpy(), t_st.cpu().numpy()[:n]

    def segment_host(self, src, off, ln, desc, dst, seg, prof, st, submit=False):
        """mi_cls_lso_segment_host on numpy arrays (views of PinnedArrays are
        worked on in place, other arrays go through the staging buffers); dst
        (which may be src) and st are written.  Returns the C status."""
        args = (self.ctx, src.ctypes.data, src.nbytes, off.ctypes.data, ln.ctypes.data, desc.ctypes.data,
                int(len(desc)), dst.ctypes.data, dst.nbytes, seg.ctypes.data, int(len(seg)),
                C.cast(prof, C.c_void_p), len(prof), st.ctypes.data)
        if submit:
            t = C.c_uint64()
            rc = self.L.mi_cls_lso_segment_host_submit(*args, C.byref(t))
            if rc == 0:
                rc = self.L.mi_cls_lso_segment_host_wait(self.ctx, t.value)
            return rc
        return self.L.mi_cls_lso_segment_host(*args)


class Classifier:
    """One classifier-enabled receive endpoint (pktio) on one GPU, driven
    through the ODP classification API.  ``apply(program)`` replays a rule
    program (odp_amd.rules) with odp_cls_* calls."""

    def __init__(self, gpu: int = 0, limits=(255, 8192, 4096), gpus=None):
        """gpus: a list of device ids -- host batches (classify_host) are then
        sharded over them (mi_cls_group_classify_host)."""
        L = lib()
        L.odp_amd_cls_reset()
        if limits is not None:
            assert L.odp_amd_cls_limits_set(*limits) == 0
        self.L = L
        if gpus:
            arr = (C.c_int * len(gpus))(*gpus)
            self.pktio = L.odp_amd_cls_pktio_create_multi(arr, len(gpus))
        else:
            self.pktio = L.odp_amd_cls_pktio_create(gpu)
        if not self.pktio:
            raise RuntimeError("odp_amd_cls_pktio_create failed")
        self.cos = []
        self.pmr = []
        self._keep = []

    def close(self):
        if self.pktio:
            self.L.odp_amd_cls_pktio_destroy(self.pktio)
            self.pktio = None

    # -- API passthroughs ------------------------------------------------
    def cos_create(self, name, action=0, queue=1, num_queue=1, hash_proto=0, stats=0, pool=0):
        p = CosParam()
        self.L.odp_cls_cos_param_init(C.byref(p))
        p.action = action
        p.num_queue = num_queue
        p.stats_enable = bool(stats)
        if num_queue > 1:
            p.qp.hash_proto = hash_proto
        else:
            p.queue = queue
        p.pool = pool
        return _h(self.L.odp_cls_cos_create(name.encode() if name else None, C.byref(p)))

    def _terms(self, terms):
        arr = (PmrParam * max(1, len(terms)))()
        keep = []
        for i, (term, value, mask, offset) in enumerate(terms):
            vb = C.create_string_buffer(bytes(value), max(1, len(value)))
            mb = C.create_string_buffer(bytes(mask), max(1, len(mask)))
            keep += [vb, mb]
            arr[i].term = term
            arr[i].range_term = False
            arr[i].value = C.cast(vb, C.c_void_p)
            arr[i].mask = C.cast(mb, C.c_void_p)
            arr[i].val_sz = len(value)
            arr[i].offset = offset
        return arr, keep

    def pmr_create(self, terms, src, dst, mark=0):
        arr, keep = self._terms(terms)
        if mark:
            o = PmrCreateOpt()
            o.terms = C.cast(arr, C.POINTER(PmrParam))
            o.num_terms = len(terms)
            o.mark = mark
            o.priority = 0
            return _h(self.L.odp_cls_pmr_create_opt(C.byref(o), src, dst))
        return _h(self.L.odp_cls_pmr_create(C.cast(arr, C.POINTER(PmrParam)), len(terms), src, dst))

    def apply(self, prog):
        """Replay a rule program; returns (cos handles, pmr handles)."""
        for op in prog:
            k = op[0]
            if k == "cos":
                a = op[2]
                self.cos.append(self.cos_create(op[1], action=a["action"], queue=a["queue"],
                                                num_queue=a["num_queue"],
                                                hash_proto=a["hash_proto"], stats=a["stats"]))
            elif k == "pmr":
                self.pmr.append(self.pmr_create(op[1], self.cos[op[2]], self.cos[op[3]], op[4]))
            elif k == "pmr_destroy":
                self.L.odp_cls_pmr_destroy(self.pmr[op[1]])
            elif k == "cos_destroy":
                self.L.odp_cos_destroy(self.cos[op[1]])
            elif k == "default":
                self.L.odp_pktio_default_cos_set(self.pktio, 0 if op[1] is None else self.cos[op[1]])
            elif k == "error":
                self.L.odp_pktio_error_cos_set(self.pktio, 0 if op[1] is None else self.cos[op[1]])
            else:
                raise ValueError(op)
        return self.cos, self.pmr

    def set_pktin_opt(self, opt: int):
        """pktin parse options of this receive endpoint
        (odp_pktin_config_opt_t.all_bits: bits 2-5 IPv4/UDP/TCP/SCTP
        checksum validation, bits 6-10 drop on IPv4/IPv6/UDP/TCP/SCTP
        errors)."""
        assert self.L.odp_amd_cls_pktin_opt_set(self.pktio, int(opt)) == 0

    def compile(self) -> bytes:
        n = self.L.odp_amd_cls_compile(self.pktio, None, 0)
        buf = C.create_string_buffer(n)
        assert self.L.odp_amd_cls_compile(self.pktio, buf, n) == n
        return buf.raw

    def program_info(self) -> dict:
        """Device encoding of the current rule snapshot (host only)."""
        blob = self.compile()
        info = (C.c_uint32 * 13)()
        rc = self.L.mi_cls_program_info(blob, len(blob), info, 13)
        if rc:
            raise RuntimeError(f"mi_cls_program_info: {rc}")
        return {"words": info[0], "hot_words": info[1], "blocks": info[2],
                "direct": info[3], "candidate": info[4], "bitmap": info[5], "wide": info[6],
                "tree": bool(info[7]), "cand1": info[8], "flat_engine": int(info[9]) - 1,
                "chained": info[10], "joint_direct": info[11], "joint_bitmap": info[12]}

    def spec_wait(self) -> int:
        """Snapshot the rules and wait for their program-specialised kernel
        (odp_amd_cls_spec_wait): 0 in use, 1 none (not a flat program,
        MI_CLS_JIT=0, or the compile failed)."""
        rc = self.L.odp_amd_cls_spec_wait(self.pktio)
        if rc < 0:
            raise RuntimeError(f"odp_amd_cls_spec_wait: {rc}")
        return rc

    def last_launch(self) -> dict:
        """The kernel instantiation of the last device launch
        (odp_amd_cls_last_launch)."""
        info = (C.c_uint32 * 7)()
        rc = self.L.odp_amd_cls_last_launch(self.pktio, info, 7)
        if rc < 0:
            raise RuntimeError(f"odp_amd_cls_last_launch: {rc}")
        k = {"nw": info[0], "lds_hot": bool(info[1]), "div": bool(info[2]),
             "flat_engine": int(info[3]) - 1, "specialised": bool(info[4]), "ck": bool(info[5]),
             "grid": info[6]}
        k["name"] = (f"mi_cls_kernel<LT={int(k['lds_hot'])}, DIV={int(k['div'])}, NW={k['nw']}, "
                     f"FM={k['flat_engine']}, CK={int(k['ck'])}"
                     f"{', MiSpec' if k['specialised'] else ''}>")
        return k

    # -- data path -------------------------------------------------------
    def classify_device(self, d_buf, d_off, d_len, n, d_out, stream=0):
        """Batch classify on device pointers (ints).  Returns the C status."""
        return self.L.odp_amd_cls_classify(self.pktio, d_buf, d_off, d_len, n, d_out, stream)

    def classify(self, batch, device="cuda:0"):
        """Convenience: upload a pktgen.Batch, classify, return a numpy
        structured array of result records (RESULT_DTYPE)."""
        import torch
        dev = torch.device(device)
        t_buf = torch.from_numpy(np.ascontiguousarray(batch.buf)).to(dev)
        t_off = torch.from_numpy(batch.off.astype(np.int32, copy=False).view(np.int32)).to(dev)
        t_len = torch.from_numpy(batch.len.astype(np.int16, copy=False).view(np.int16)).to(dev)
        t_out = torch.empty((max(1, batch.n), 4), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), batch.n,
                                  t_out.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"odp_amd_cls_classify: {rc} "
                               f"({self.L.mi_cls_strerror(rc).decode()})")
        torch.cuda.synchronize(dev)
        out = t_out.cpu().numpy().view(np.uint8).reshape(-1)[: 16 * batch.n]
        return out.view(R.RESULT_DTYPE).copy()

    def classify_host(self, batch):
        """The pktio receive-path entry (odp_amd_cls_classify_host): the
        batch from host memory, staged, classified (sharded over the
        pktio's GPUs when it has several) and the records copied back."""
        out = np.zeros(max(1, batch.n), dtype=R.RESULT_DTYPE)
        buf = np.ascontiguousarray(batch.buf)
        off = np.ascontiguousarray(batch.off, dtype=np.uint32)
        ln = np.ascontiguousarray(batch.len, dtype=np.uint16)
        rc = self.L.odp_amd_cls_classify_host(self.pktio, buf.ctypes.data, buf.nbytes,
                                              off.ctypes.data, ln.ctypes.data, batch.n,
                                              out.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"odp_amd_cls_classify_host: {rc}")
        return out[: batch.n]

    def enq_table(self):
        """The enqueue plan's table of the current control plane
        (odp_amd_cls_enqtab_fill; host only).  Returns (EnqTab, queues, gen):
        queues[id] the odp_queue_t of destination id, gen the generation the
        table was built under."""
        tab = EnqTab()
        q = (C.c_void_p * ENQ_DST_MAX)()
        nd, gen = C.c_uint32(), C.c_uint64()
        rc = self.L.odp_amd_cls_enqtab_fill(C.byref(tab), q, C.byref(nd), C.byref(gen))
        if rc != 0:
            raise RuntimeError(f"odp_amd_cls_enqtab_fill: {rc}")
        return tab, [_h(q[i]) for i in range(nd.value)], gen.value

    def enq_plan(self, records, lens, tab=None, device="cuda:0", poison=0xA5A5A5A5):
        """The enqueue plan of classified records (odp_amd_cls_enq_plan, on
        the pktio's context and torch's current stream -- the stream of
        classify()): returns (perm, gbeg, counters).  tab: enq_table()'s
        (default: built now)."""
        if tab is None:
            tab = self.enq_table()[0]
        return _enq_plan_device(self.L.odp_amd_cls_enq_plan, self.pktio, records, lens, tab, device, poison)

    def enq_plan_host(self, res, ln, perm, gbeg, out, tab=None, submit=False):
        """odp_amd_cls_enq_plan_host on numpy arrays (submit: the _submit /
        _wait pair), as EnqContext.plan_host."""
        if tab is None:
            tab = self.enq_table()[0]
        _enq_plan_host(self.L, "odp_amd_cls_enq_plan_host", self.pktio, res, ln, tab, perm, gbeg, out, submit)

    def run_table(self):
        """The run plan's table of the current control plane
        (odp_amd_cls_runtab_fill; host only).  Returns (RunTab, vpools, gen):
        vpools[slot] the vector pool of each slot."""
        tab = RunTab()
        p = (C.c_void_p * RUN_VSLOTS)()
        ns, gen = C.c_uint32(), C.c_uint64()
        rc = self.L.odp_amd_cls_runtab_fill(C.byref(tab), p, C.byref(ns), C.byref(gen))
        if rc != 0:
            raise RuntimeError(f"odp_amd_cls_runtab_fill: {rc}")
        return tab, [_h(p[i]) for i in range(ns.value)], gen.value

    def enq_runs(self, records, lens, tab=None, rtab=None, burst=0, run_cap=None, device="cuda:0",
                 poison=0xA5A5A5A5):
        """The run plan of classified records (odp_amd_cls_enq_runs, on the
        pktio's context and torch's current stream): returns (seq, runs, out).
        tab / rtab: enq_table()'s and run_table()'s (default: built now)."""
        if tab is None:
            tab = self.enq_table()[0]
        if rtab is None:
            rtab = self.run_table()[0]
        cap = len(records) if run_cap is None else run_cap
        return _enq_runs_device(self.L.odp_amd_cls_enq_runs, self.pktio, records, lens, tab, rtab, burst, cap,
                                device, poison)

    def enq_runs_host(self, res, ln, seq, runs, out, tab=None, rtab=None, burst=0, submit=False):
        """odp_amd_cls_enq_runs_host on numpy arrays (submit: the _submit /
        _wait pair), as EnqContext.runs_host."""
        if tab is None:
            tab = self.enq_table()[0]
        if rtab is None:
            rtab = self.run_table()[0]
        _enq_runs_host(self.L, "odp_amd_cls_enq_runs_host", self.pktio, res, ln, tab, rtab, burst, seq, runs, out,
                       submit)

    def pool_table(self, slot_cap, pktio_pool=None):
        """The pool plan's table of the current control plane
        (odp_amd_cls_pooltab_cos; host only) for a pktio whose own pool is
        pktio_pool.  slot_cap: {pool handle: capacity}, or one capacity for
        every slot.  Returns (PoolTab, pools, gen): pools[slot] each slot's
        pool handle."""
        tab = PoolTab()
        p = (C.c_void_p * POOL_SLOTS)()
        ns, gen = C.c_uint32(), C.c_uint64()
        rc = self.L.odp_amd_cls_pooltab_cos(pktio_pool, C.byref(tab), p, C.byref(ns), C.byref(gen))
        if rc != 0:
            raise RuntimeError(f"odp_amd_cls_pooltab_cos: {rc}")
        pools = [_h(p[i]) for i in range(ns.value)]
        for k, h in enumerate(pools):
            tab.slot_cap[k] = int(slot_cap[h] if isinstance(slot_cap, dict) else slot_cap)
        return tab, pools, gen.value

    def pool_plan(self, records, lens, own, have, base, tab, device="cuda:0", poison=0xA5A5A5A5,
                  in_place=False):
        """The pool plan of classified records (odp_amd_cls_pool_plan, on the
        pktio's context and torch's current stream): returns (res_out, dec,
        idx, out).  tab: pool_table()'s."""
        return _pool_plan_device(self.L.odp_amd_cls_pool_plan, self.pktio, records, lens, own, tab, have, base,
                                 device, poison, in_place)

    def pool_plan_host(self, res, ln, own, have, base, res_out, dec, idx, out, tab, submit=False):
        """odp_amd_cls_pool_plan_host on numpy arrays (submit: the _submit /
        _wait pair), as EnqContext.pools_host."""
        return _pool_plan_host(self.L, "odp_amd_cls_pool_plan_host", self.pktio, res, ln, own, tab, have, base,
                               res_out, dec, idx, out, submit)

    def pool_move_geom(self):
        """odp_amd_cls_pool_move_geom: (rc, meta_off, data_from_meta, arena_lo,
        arena_bytes); rc -ENOENT when no pool is page-locked."""
        mo, dfm = C.c_uint32(), C.c_uint32()
        lo, nb = C.c_uint64(), C.c_uint64()
        rc = self.L.odp_amd_cls_pool_move_geom(C.byref(mo), C.byref(dfm), C.byref(lo), C.byref(nb))
        return rc, mo.value, dfm.value, lo.value, nb.value

    def pool_move(self, args, stream=0):
        """The pool move of a planned batch (odp_amd_cls_pool_move, on the
        pktio's context) on a MoveArgs of device pointers, stream-ordered.
        Returns the C status."""
        return self.L.odp_amd_cls_pool_move(self.pktio, C.byref(args), stream or None)

    def pool_move_host(self, args, submit=False):
        """odp_amd_cls_pool_move_host (submit: the _submit / _wait pair), as
        EnqContext.move_host."""
        return _move_host(self.L, "odp_amd_cls_pool_move_host", self.pktio, args, submit)

    def vec_geom(self):
        """odp_amd_cls_vec_geom: (rc, size_off, tbl_off, varena_lo,
        varena_bytes)."""
        so, to = C.c_uint32(), C.c_uint32()
        lo, nb = C.c_uint64(), C.c_uint64()
        rc = self.L.odp_amd_cls_vec_geom(C.byref(so), C.byref(to), C.byref(lo), C.byref(nb))
        return rc, so.value, to.value, lo.value, nb.value

    def vec_fill(self, args, stream=0):
        """The vector fill of a planned batch (odp_amd_cls_vec_fill, on the
        pktio's context) on a VecArgs of device pointers, stream-ordered.
        Returns the C status."""
        return self.L.odp_amd_cls_vec_fill(self.pktio, C.byref(args), stream or None)

    def vec_fill_host(self, args, submit=False):
        """odp_amd_cls_vec_fill_host (submit: the _submit / _wait pair), as
        EnqContext.fill_host."""
        return _move_host(self.L, "odp_amd_cls_vec_fill_host", self.pktio, args, submit)

    def cos_stats_packets(self, cos_handle):
        s = CosStats()
        assert self.L.odp_cls_cos_stats(cos_handle, C.byref(s)) == 0
        return s.packets
