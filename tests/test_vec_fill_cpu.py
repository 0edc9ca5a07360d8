"""The vector fill without a GPU: the model (tests/vec_model.py), loop against
numpy and by hand; its deliveries against the runtime's statement of the
reference's packet vectors (rt_helpers.expected_vectors); the struct mirrors
against the C compiler; what the library and pktio entries answer without a
device; and the host side -- geometry, odp_amd_cls_vec_take, odp_amd_cls_vec_enq
-- through a stand-alone C program (tests/rt/vecenq_unit.c).
"""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import enq_model as M
from tests import rt_helpers as H
from tests import run_model as RM
from tests import vec_model as VM
from tests import zoo

UNIT = os.path.join(H.ROOT, "tests", "_bin", "vecenq_unit")


def random_plan(rng, n, ndst, burst, nslots, vmaxes=(1, 2, 3, 4096)):
    """A run plan over random records of every outcome, in stretches of 1 .. 12
    records to one destination, under every mode."""
    table, entry_of = M.make_table(rng, ndst)
    rtable = RM.make_rtable(rng, nslots=nslots, vmaxes=vmaxes)
    lens_ = rng.integers(1, 13, n + 1)
    dst = np.repeat(rng.integers(0, ndst, n + 1), lens_)[:n]
    dst = np.where(rng.integers(0, 5, n) == 0, M.drops(n), dst)
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    seq, runs, out = RM.plan_runs_np(rec, lens, table, rtable, burst)
    return seq, runs, out, rtable


@pytest.mark.parametrize("burst", [0, 7, 1000])
@pytest.mark.parametrize("seed,n,ndst,nslots", [(1, 0, 3, 1), (2, 1, 1, 1), (3, 500, 1, 2), (4, 3000, 7, 3),
                                                (5, 3000, 300, 16), (6, 2500, 40, 5)])
@pytest.mark.parametrize("stock", ["none", "short", "exact", "ample"])
def test_model_pair(seed, n, ndst, nslots, burst, stock):
    """fill() -- the per-run loop that allocates until the slot's stock is gone
    -- equals fill_np() on random plans: every mode, vector sizes 1, 2, 3 and
    4096, 1 to 16 slots, a stock of nothing, one short, exact and ample, holes
    in ent."""
    rng = np.random.default_rng(seed)
    seq, runs, out, rtable = random_plan(rng, n, ndst, burst, nslots)
    need = np.array(out["vec_need"], np.int64)
    vhave = {"none": need * 0, "short": np.maximum(need - 1, 0), "exact": need, "ample": need + 5}[stock]
    if stock == "short" and seed % 2:
        vhave = need // 2
    vbase = np.cumsum(vhave) - vhave + 3
    vgot = (0x7000000 + 0x400 * rng.permutation(int(vhave.sum()) + 3)).astype(np.uint64)
    ent = VM.make_ent(rng, n, holes=0.05)
    ok = VM.arena_ok(0x7000000, 0x400 * (vgot.shape[0] // 2 + 1), 16) if seed == 6 else None
    a = VM.fill(seq, runs, ent, rtable, vgot, vbase, vhave, 64, ok)
    b = VM.fill_np(seq, runs, ent, rtable, vgot, vbase, vhave, 64, ok)
    VM.same(a, b)
    o, evr = a["out"], a["evr"]
    assert o["ev_span"] == a["ev"].shape[0] <= n and o["lost"] == a["lost"].shape[0]
    assert o["events"] == int(evr["ev_count"].astype(np.int64).sum())
    assert o["vec_used"] == np.minimum(need, vhave).tolist()
    assert o["vectors"] + o["refused"] == sum(o["vec_used"])
    plain = (runs["flags"] & RM.VEC) == 0
    packets = int(runs["count"][plain].sum()) + o["in_vectors"] + o["lost"]
    assert packets == out["delivered"] if ok is None else packets <= out["delivered"]
    assert int(evr["pk_enq"].astype(np.int64).sum()) + o["lost"] == out["delivered"]
    if stock in ("exact", "ample"):
        assert o["lost"] == 0
    if stock == "none":
        assert o["vectors"] == 0 and o["lost"] == int(runs["count"][~plain].sum())
    if seed == 6 and stock != "none":
        assert o["refused"] > 0


def test_model_by_hand():
    """Three slots' worth of rules on runs written out one by one: CoS 0 and 2
    share slot 5 (vectors of 2 and of 3), CoS 1 is plain with an aggregator."""
    mode, vmax, vslot = np.zeros(256, np.uint8), np.zeros(256, np.uint16), np.zeros(256, np.uint8)
    mode[0], mode[1], mode[2] = RM.VEC, RM.AGGR, RM.VEC
    vmax[0], vmax[2] = 2, 3
    vslot[0] = vslot[2] = 5
    runs = np.array([(0, 3, 0, 0, RM.VEC, 2),     # vectors of 2 and 1: stock 0, 1
                     (3, 2, 0, 1, RM.AGGR, 0),    # plain, two events
                     (5, 1, 1, 0, 0, 0),          # a single packet of a vector CoS: plain
                     (6, 7, 0, 2, RM.VEC, 3),     # wants 3, gets stock 2 alone: 3 in, 4 lost
                     (13, 2, 0, 0, RM.VEC, 1)],   # the stock is gone: 2 lost
                    RM.RUN_DTYPE)
    seq = np.array([14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 15], np.uint32)   # 15: not delivered
    ent = (1000 + 100 * np.arange(16)).astype(np.uint64)
    ent[9] = 0                                    # seq[5]: the move refused it
    vgot = np.array([0, 0, 0, 0, 8000, 8100, 8200], np.uint64)
    vbase, vhave = [0] * 5 + [4], [0] * 5 + [3]
    h = lambda p: int(ent[seq[p]]) - 40 if ent[seq[p]] else 0   # noqa: E731
    for f in (VM.fill, VM.fill_np):
        r = f(seq, runs, ent, (mode, vmax, vslot), vgot, vbase, vhave, 40)
        assert r["ev"].tolist() == [8000, 8100, h(3), h(4), 0, 8200, 0, 0, 0]
        assert r["evr"].tolist() == [(0, 2, 3, 4), (2, 2, 2, VM.NONE), (4, 1, 1, VM.NONE), (5, 1, 3, 6),
                                     (8, 0, 0, VM.NONE)]
        assert r["lost"].tolist() == sorted(h(p) for p in (9, 10, 11, 12, 13, 14))
        assert r["vec_idx"].tolist() == [4, 5, 6] and r["vec_size"].tolist() == [2, 1, 3]
        assert r["vec_tbl"].tolist() == [h(0), h(1), h(2), h(6), h(7), h(8)]
        assert r["out"] == {"events": 6, "ev_span": 9, "vectors": 3, "in_vectors": 6, "lost": 6, "holes": 1,
                            "refused": 0, "truncated": 0, "vec_used": [0] * 5 + [3] + [0] * 10}
        assert VM.events(runs, r, ["q0", "q1"]) == {"q0": [("V", 2), ("V", 1), ("P",), ("P",), ("V", 3)],
                                                    "q1": [("P",)]}
    # the second vector does not lie in the arena: refused, its packet in no count
    r = VM.fill(seq, runs, ent, (mode, vmax, vslot), vgot, vbase, vhave, 40,
                lambda v, size: np.asarray(v) != 8100)
    assert r["ev"].tolist()[:2] == [8000, 0] and r["vec_idx"].tolist() == [4, 6]
    assert (r["out"]["vectors"], r["out"]["in_vectors"], r["out"]["refused"], r["out"]["events"]) == (2, 5, 1, 6)


def _oracle_plan(burst, max_size, vmode=RM.VEC):
    from oracle.oracle import Oracle
    frames = H.pcap_frames([f for _, f in zoo.all_frames()] * 3)
    prog = zoo.prog_everything()
    o = Oracle()
    o.apply(prog)
    b = pg.batch_from_frames(frames)
    recs = o.classify(b)
    cos_nq, cos_q0 = np.zeros(256, np.uint8), np.zeros(256, np.uint16)
    ent, names = [], []
    mode = np.zeros(256, np.uint8)
    for s, (name, attrs) in sorted(H.cos_names(prog).items()):
        if attrs["action"]:
            continue
        nq = attrs["num_queue"]
        cos_nq[s], cos_q0[s], mode[s] = nq, len(ent), vmode
        for j in range(nq):
            ent.append(len(names))
            names.append(name if nq == 1 else f"_odp_cos_hq_{s}_{j}")
    ent_dst = np.full(M.ENT, 0xFFFF, np.uint16)
    ent_dst[:len(ent)] = ent
    table = (cos_nq, cos_q0, ent_dst, len(names))
    rtable = (mode, np.full(256, max_size, np.uint16), np.zeros(256, np.uint8))
    seq, runs, out = RM.plan_runs(recs, b.len, table, rtable, burst)
    return prog, frames, seq, runs, out, rtable, names


@pytest.mark.parametrize("max_size", [4, 4096])
@pytest.mark.parametrize("burst", [32, 4096])
def test_model_events_are_the_runtimes(built, burst, max_size):
    """The fill's deliveries per queue over the oracle's records equal
    rt_helpers.expected_vectors -- the statement the runtime's packet-vector
    delivery through odp_pktin_recv is tested against
    (test_rx_packet_vector_cos) -- for that test's program and frames.  With a
    vector pool too small for the batch, the runs are served in arrival order
    until the pool is empty: each queue's deliveries are the full ones with
    vectors left out, the vectors delivered are the pool's, and every packet is
    delivered or lost."""
    prog, frames, seq, runs, out, rtable, names = _oracle_plan(burst, max_size)
    exp = H.expected_vectors(prog, frames, burst, max_size)
    n = seq.shape[0]
    ent = (0x100000 + 0x800 * np.arange(n)).astype(np.uint64)
    need = out["vec_need"][0]
    assert out["delivered"] > 100 and need > 3
    vgot = (0x9000000 + 64 * np.arange(need)).astype(np.uint64)
    full = VM.fill(seq, runs, ent, rtable, vgot, [0], [need], 64)
    VM.same(full, VM.fill_np(seq, runs, ent, rtable, vgot, [0], [need], 64))
    assert VM.events(runs, full, names) == exp
    assert full["out"]["lost"] == 0 and full["out"]["vectors"] == need
    have = need // 2
    short = VM.fill(seq, runs, ent, rtable, vgot, [0], [have], 64)
    VM.same(short, VM.fill_np(seq, runs, ent, rtable, vgot, [0], [have], 64))
    got = VM.events(runs, short, names)
    assert sum(e[0] == "V" for q in got.values() for e in q) == have == short["out"]["vectors"]
    for q, evs in exp.items():
        it = iter(evs)
        assert all(e in it for e in got.get(q, [])), q      # a subsequence, order kept
        assert [e for e in got.get(q, []) if e[0] == "P"] == [e for e in evs if e[0] == "P"]
    inq = sum(1 if e[0] == "P" else e[1] for q in got.values() for e in q)
    assert inq + short["out"]["lost"] == out["delivered"] and short["out"]["lost"] > 0
    # the vectors go to the runs in arrival order: those served are a prefix
    vec = (runs["flags"] & RM.VEC) != 0
    served = short["evr"]["ev_count"][vec] > 0
    assert not served.all() and not served[np.argmin(served):].any()


# ---- the library's entry points --------------------------------------------
MIRROR_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mi_cls.h"
#define F(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
	printf("mi_cls_vec_args_t %zu\nmi_cls_vec_out_t %zu\nmi_cls_evrun_t %zu\n", sizeof(mi_cls_vec_args_t),
	       sizeof(mi_cls_vec_out_t), sizeof(mi_cls_evrun_t));
	F(mi_cls_vec_args_t, seq); F(mi_cls_vec_args_t, runs); F(mi_cls_vec_args_t, run_out);
	F(mi_cls_vec_args_t, ent); F(mi_cls_vec_args_t, vgot); F(mi_cls_vec_args_t, n);
	F(mi_cls_vec_args_t, run_cap); F(mi_cls_vec_args_t, nvgot); F(mi_cls_vec_args_t, size_off);
	F(mi_cls_vec_args_t, tbl_off); F(mi_cls_vec_args_t, rsv); F(mi_cls_vec_args_t, ent_to_handle);
	F(mi_cls_vec_args_t, rtab); F(mi_cls_vec_args_t, vbase); F(mi_cls_vec_args_t, vhave);
	F(mi_cls_vec_args_t, vcap); F(mi_cls_vec_args_t, varena_lo); F(mi_cls_vec_args_t, varena_bytes);
	F(mi_cls_vec_args_t, ev); F(mi_cls_vec_args_t, evr); F(mi_cls_vec_args_t, lost); F(mi_cls_vec_args_t, out);
	F(mi_cls_vec_out_t, events); F(mi_cls_vec_out_t, ev_span); F(mi_cls_vec_out_t, vectors);
	F(mi_cls_vec_out_t, in_vectors); F(mi_cls_vec_out_t, lost); F(mi_cls_vec_out_t, holes);
	F(mi_cls_vec_out_t, refused); F(mi_cls_vec_out_t, truncated); F(mi_cls_vec_out_t, vec_used);
	F(mi_cls_evrun_t, ev_first); F(mi_cls_evrun_t, ev_count); F(mi_cls_evrun_t, pk_enq); F(mi_cls_evrun_t, vfirst);
	printf("tile %d grid %d\n", MI_CLS_VEC_TILE, MI_CLS_VEC_GRID);
	return 0;
}
"""


def test_struct_mirrors(built, tmp_path):
    """cls.VecArgs, VecOut and EVRUN_DTYPE against the compiler's sizeof and
    offsetof of include/mi_cls.h."""
    from odp_amd import cls
    src = tmp_path / "mirror.c"
    src.write_text(MIRROR_C)
    exe = str(tmp_path / "mirror")
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(H.ROOT, "include"), "-o", exe, str(src)], check=True)
    c = dict(ln.rsplit(" ", 1) for ln in subprocess.run([exe], stdout=subprocess.PIPE, text=True,
                                                         check=True).stdout.splitlines() if "tile" not in ln)
    c = {k: int(v) for k, v in c.items()}
    assert C.sizeof(cls.VecArgs) == c["mi_cls_vec_args_t"] and C.sizeof(cls.VecOut) == c["mi_cls_vec_out_t"] == 192
    assert cls.EVRUN_DTYPE.itemsize == c["mi_cls_evrun_t"] == 16 and cls.EVRUN_DTYPE == VM.EVRUN_DTYPE
    for name, _ in cls.VecArgs._fields_:
        assert getattr(cls.VecArgs, name).offset == c[f"mi_cls_vec_args_t.{name}"], name
    for name, _ in cls.VecOut._fields_:
        assert getattr(cls.VecOut, name).offset == c[f"mi_cls_vec_out_t.{name}"], name
    for name in cls.EVRUN_DTYPE.names:
        assert cls.EVRUN_DTYPE.fields[name][1] == c[f"mi_cls_evrun_t.{name}"], name
    assert len(c) == 3 + len(cls.VecArgs._fields_) + len(cls.VecOut._fields_) + 4
    assert (cls.VEC_TILE, cls.VEC_GRID) == (1024, 256) and cls.VEC_OUT_WORDS == 24
    assert tuple(cls.vec_out_dict(range(24))) == VM.FIELDS and cls.VEC_NO_VECTOR == VM.NONE
    assert cls.vec_out_dict(range(24))["vec_used"] == list(range(8, 24))


def test_library_entries_without_a_context(built):
    """The table and the scalars are checked first, with or without a device:
    every documented bad argument that needs no array is -EINVAL.  No context:
    -ENODEV where there is no device (-EINVAL where there is one).  Nothing is
    written."""
    from odp_amd import cls
    L = cls.lib()
    out = np.zeros(24, np.uint64)
    vg = np.zeros(4, np.uint64)
    good = cls.run_tab([cls.RUN_VEC, cls.RUN_AGGR], [8, 0], [2, 0])
    novmax = cls.run_tab([cls.RUN_VEC], [0], [0])
    badslot = cls.run_tab([cls.RUN_VEC], [5], [cls.RUN_VSLOTS])
    unused = cls.run_tab([cls.RUN_AGGR, 0], [9, 9], [200, 99])   # no VEC bit: vmax and vslot mean nothing
    no_ctx = -errno.ENODEV if L.mi_cls_device_count() <= 0 else -errno.EINVAL
    ok = dict(out=out.ctypes.data, size_off=16, tbl_off=24, varena_lo=4096, varena_bytes=4096)
    cap = [0, 0, 8]
    cases = [((None, cap, ok), -errno.EINVAL),
             ((novmax, [8], ok), -errno.EINVAL),
             ((badslot, [8] * 16, ok), -errno.EINVAL),
             ((good, [0, 0, 7], ok), -errno.EINVAL),                       # vmax 8 > the pool's max_size 7
             ((good, cap, dict(ok, size_off=18)), -errno.EINVAL),
             ((good, cap, dict(ok, size_off=24)), -errno.EINVAL),          # size not wholly before tbl
             ((good, cap, dict(ok, size_off=20, tbl_off=20)), -errno.EINVAL),
             ((good, cap, dict(ok, tbl_off=28)), -errno.EINVAL),
             ((good, cap, dict(ok, n=1 << 28)), -errno.EINVAL),
             ((good, cap, dict(ok, varena_lo=(1 << 64) - 64, varena_bytes=128)), -errno.EINVAL),
             ((good, cap, dict(ok, nvgot=3, vgot=0)), -errno.EINVAL),      # vectors and no array
             ((good, cap, dict(ok, nvgot=4, vgot=vg.ctypes.data, vb=(2, 3))), -errno.EINVAL),   # past nvgot
             ((good, cap, dict(ok, nvgot=4, vgot=vg.ctypes.data, vb=(2, 2))), no_ctx),
             ((good, cap, ok), no_ctx),
             ((unused, [], ok), no_ctx),
             ((good, cap, dict(ok, n=(1 << 28) - 1)), no_ctx)]
    t = C.c_uint64(99)
    for (rtab, vcap, kw), rc in cases:
        kw = dict(kw)
        vb = kw.pop("vb", None)
        a = cls.vec_args(rtab, vbase=[0, 0, vb[0]] if vb else (), vhave=[0, 0, vb[1]] if vb else (), vcap=vcap, **kw)
        assert L.mi_cls_vec_fill(None, C.byref(a), None) == rc, kw
        assert L.mi_cls_vec_fill_host(None, C.byref(a)) == rc
        t.value = 99
        assert L.mi_cls_vec_fill_host_submit(None, C.byref(a), C.byref(t)) == rc and t.value == 0
    assert L.mi_cls_vec_fill(None, None, None) == -errno.EINVAL
    assert L.mi_cls_vec_fill_host_submit(None, C.byref(cls.vec_args(good, vcap=cap, **ok)), None) == -errno.EINVAL
    assert L.mi_cls_vec_fill_host_wait(None, 1) == no_ctx
    assert not out.any()
    with pytest.raises(TypeError):
        cls.vec_args(good, nope=1)


def test_pktio_entries(built):
    """The pktio forms create the context on first use: -ENODEV without a GPU;
    with one, an empty batch's out is all zeros.  The geometry is the
    runtime's: -ENOENT while no vector pool is page-locked."""
    from odp_amd import cls
    have = cls.lib().mi_cls_device_count() > 0
    c = cls.Classifier(gpu=0)
    try:
        c.apply([R.cos("a", queue=11), ("default", 0)])
        rtab, _, _ = c.run_table()
        rc, size_off, tbl_off, lo, nb = c.vec_geom()
        assert rc in (0, -errno.ENOENT) and size_off % 4 == 0 and tbl_off % 8 == 0 and size_off + 4 <= tbl_off
        assert (rc == 0) == (nb != 0)
        for submit in (False, True):
            out = np.full(24, 7, np.uint64)
            a = cls.vec_args(rtab, out=out.ctypes.data, size_off=size_off, tbl_off=tbl_off, varena_lo=lo,
                             varena_bytes=nb)
            rc = c.vec_fill_host(a, submit=submit)
            assert rc == (0 if have else -errno.ENODEV)
            assert not out.any() if have else (out == 7).all()
        out = np.full(24, 7, np.uint64)
        a = cls.vec_args(rtab, out=out.ctypes.data, size_off=size_off, tbl_off=tbl_off)
        assert c.vec_fill(a) == (0 if have else -errno.ENODEV)
    finally:
        c.close()


def test_host_side_unit(built):
    """tests/rt/vecenq_unit.c: odp_amd_cls_vec_geom agrees with the runtime's
    vectors, odp_amd_cls_pool_move_geom answers as before with vector pools
    created, the context-free argument checks, odp_amd_cls_vec_take with a pool
    that runs short and odp_amd_cls_vec_enq: events, vector sizes and packets
    per queue, queue stats and pool free counts."""
    r = subprocess.run([UNIT], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
