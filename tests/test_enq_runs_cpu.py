"""The run plan without a GPU: the model (tests/run_model.py), loop against
numpy; its deliveries against the runtime's statement of the reference's runs
(rt_helpers.expected_vectors); the table builder odp_amd_cls_runtab_fill
through a C driver; and what the library entries answer without a device.
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
from tests import zoo

RUNTAB_DRIVER = os.path.join(H.ROOT, "tests", "_bin", "runtab_driver")


def same(a, b):
    assert np.array_equal(a[0], b[0])
    assert a[1].dtype == b[1].dtype == RM.RUN_DTYPE and np.array_equal(a[1], b[1])
    assert a[2] == b[2]


@pytest.mark.parametrize("burst", [0, 1, 7, 64, 1000])
@pytest.mark.parametrize("seed,n,ndst", [(1, 0, 3), (2, 1, 1), (3, 500, 1), (4, 3000, 7), (5, 3000, 300),
                                         (6, 5000, 8192), (7, 2000, 0)])
def test_model_pair(seed, n, ndst, burst):
    """plan_runs() -- the per-record loop -- equals plan_runs_np() on random
    records of every outcome, stale ones among them, in runs of random
    lengths (so that neighbours often share a key), under every mode."""
    rng = np.random.default_rng(seed)
    table, entry_of = M.make_table(rng, ndst)
    rtable = RM.make_rtable(rng)
    if ndst:
        # stretches of 1 .. 12 records to one destination, a fifth of them dropped
        lens_ = rng.integers(1, 13, n + 1)
        dst = np.repeat(rng.integers(0, ndst, n + 1), lens_)[:n]
        dst = np.where(rng.integers(0, 5, n) == 0, M.drops(n), dst)
    else:
        dst = M.drops(n)
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    wild = rng.integers(0, 9, n) == 0
    rec["outcome"][wild] = M.OUT_ENQ
    rec["cos"][wild] = rng.integers(0, 256, int(wild.sum()))
    rec["queue"][wild] = rng.integers(0, 70, int(wild.sum()))
    a = RM.plan_runs(rec, lens, table, rtable, burst)
    same(a, RM.plan_runs_np(rec, lens, table, rtable, burst))
    seq, runs, out = a
    # the plan's counters and its not-delivered group are the run plan's
    perm, gbeg, ctr = M.plan(rec, lens, table)
    assert {k: out[k] for k in M.FIELDS} == ctr
    assert np.array_equal(seq[out["delivered"]:], perm[gbeg[ndst]:])
    assert sorted(seq.tolist()) == list(range(n))
    assert int(runs["count"].sum()) == out["delivered"] and out["nruns"] == runs.shape[0]
    assert np.array_equal(runs["first"], np.cumsum(runs["count"]) - runs["count"])
    assert out["vectors"] == sum(out["vec_need"]) == int(runs["nvec"].sum())
    if burst == 1:
        assert out["nruns"] == out["delivered"] and out["vectors"] == 0


def test_model_by_hand():
    """The rules on records written out one by one: ids 0 and 1, CoS 0 (two
    entries that share id 0, and one of id 1), CoS 1 on id 0 as well."""
    table = (np.array([3, 1] + [0] * 254, np.uint8), np.array([0, 3] + [0] * 254, np.uint16),
             np.array([0, 0, 1, 0] + [0xFFFF] * (M.ENT - 4), np.uint16), 2)
    mode = np.zeros(256, np.uint8)
    mode[0], mode[1] = RM.VEC, RM.AGGR
    vmax = np.zeros(256, np.uint16)
    vmax[0] = 2
    vslot = np.zeros(256, np.uint8)
    vslot[0] = 5
    rows = [  # outcome, cos, queue
        (M.OUT_ENQ, 0, 0),        # 0: id 0 cos 0           run 0
        (M.OUT_ENQ, 0, 1),        # 1: another entry, id 0: the same run
        (M.OUT_DISCARD, 0, 0),    # 2: ends no run
        (M.OUT_ENQ, 0, 0),        # 3: still run 0 (3 packets: 2 vectors)
        (M.OUT_ENQ, 1, 0),        # 4: id 0 under CoS 1: run 1 (aggregator, plain)
        (M.OUT_ENQ, 1, 0),        # 5
        (M.OUT_ENQ, 0, 2),        # 6: CoS 0, id 1: run 2, one packet: plain
        (M.OUT_ENQ, 0, 0),        # 7: CoS 0, id 0: run 3 ...
        (M.OUT_ENQ, 0, 7),        # 8: stale: ends no run
        (M.OUT_ENQ, 0, 0),        # 9: ... two packets, one vector
    ]
    rec = np.zeros(len(rows), R.RESULT_DTYPE)
    for i, (outcome, cos, queue) in enumerate(rows):
        rec[i]["outcome"], rec[i]["cos"], rec[i]["queue"] = outcome, cos, queue
    lens = np.full(len(rows), 100, np.uint16)
    seq, runs, out = RM.plan_runs(rec, lens, table, (mode, vmax, vslot))
    assert seq.tolist() == [0, 1, 3, 4, 5, 6, 7, 9, 2, 8]
    assert runs.tolist() == [(0, 3, 0, 0, RM.VEC, 2), (3, 2, 0, 1, RM.AGGR, 0), (5, 1, 1, 0, 0, 0),
                             (6, 2, 0, 0, RM.VEC, 1)]
    assert out["nruns"] == 4 and out["vectors"] == 3 and out["vec_need"][5] == 3 and out["stale"] == 1
    # bursts of 3: records 0-2 | 3-5 | 6-8 | 9
    seq3, runs3, out3 = RM.plan_runs(rec, lens, table, (mode, vmax, vslot), burst=3)
    assert seq3.tolist() == seq.tolist()
    assert [(r["first"], r["count"], r["flags"], r["nvec"]) for r in runs3] == \
        [(0, 2, RM.VEC, 1), (2, 1, 0, 0), (3, 2, RM.AGGR, 0), (5, 1, 0, 0), (6, 1, 0, 0), (7, 1, 0, 0)]
    assert out3["vectors"] == 1


@pytest.mark.parametrize("max_size", [4, 4096])
@pytest.mark.parametrize("burst", [32, 4096])
def test_model_events_are_the_runtimes(built, burst, max_size):
    """The model's deliveries per queue over the oracle's records equal
    rt_helpers.expected_vectors -- the statement the runtime's packet-vector
    delivery is tested against -- for the program and frames of
    test_rx_packet_vector_cos: every enqueue CoS delivers vectors, every
    (CoS, queue slot) has a queue of its own."""
    from oracle.oracle import Oracle
    frames = H.pcap_frames([f for _, f in zoo.all_frames()] * 3)
    prog = zoo.prog_everything()
    exp = H.expected_vectors(prog, frames, burst, max_size)
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
        cos_nq[s], cos_q0[s], mode[s] = nq, len(ent), RM.VEC
        for j in range(nq):
            ent.append(len(names))
            names.append(name if nq == 1 else f"_odp_cos_hq_{s}_{j}")
    ent_dst = np.full(M.ENT, 0xFFFF, np.uint16)
    ent_dst[:len(ent)] = ent
    table = (cos_nq, cos_q0, ent_dst, len(names))
    rtable = (mode, np.full(256, max_size, np.uint16), np.zeros(256, np.uint8))
    seq, runs, out = RM.plan_runs(recs, b.len, table, rtable, burst)
    assert out["stale"] == 0 and out["delivered"] > 100
    assert RM.events(runs, rtable, names) == exp
    same((seq, runs, out), RM.plan_runs_np(recs, b.len, table, rtable, burst))


def test_runtab_fill(built):
    """odp_amd_cls_runtab_fill over a control plane made through the public
    API (tests/rt/runtab_driver.c): plain, vector and aggregator CoS, two CoS on
    one pool, a drop CoS; 16 pools fit, the 17th is -E2BIG."""
    r = subprocess.run([RUNTAB_DRIVER], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0] == "fill 0 nslots 2 gen_ok 1 stamp_new 1".split()
    cos = {ln[1]: tuple(int(x) for x in ln[4::2]) for ln in lines if ln[0] == "cos"}
    assert cos == {"plain": (0, 0, 0), "vecA": (RM.VEC, 8, 0), "aggr": (RM.AGGR, 0, 0), "vecA2": (RM.VEC, 3, 0),
                   "vecB": (RM.VEC, 64, 1), "drop": (0, 0, 0)}
    assert [ln[1:] for ln in lines if ln[0] == "slot"] == [["0", "vpoolA"], ["1", "vpoolB"]]
    rest = {ln[0]: ln[1:] for ln in lines if ln[0] not in ("cos", "slot", "fill")}
    assert rest == {"unused_modes": ["0"], "full": ["0", "nslots", "16"], "over": [str(-errno.E2BIG)],
                    "bad": [str(-errno.EINVAL)] * 2}


def test_runtab_fill_binding(built):
    """Classifier.run_table() on a control plane without vectors: no slot, no
    mode; the generation is the control plane's."""
    from odp_amd.cls import Classifier
    c = Classifier(gpu=0)
    try:
        c.apply([R.cos("a", queue=11), R.cos("h", num_queue=4, hash_proto=R.HP_IPV4_UDP), ("default", 0)])
        rtab, vpools, gen = c.run_table()
        assert vpools == [] and gen == c.L.odp_amd_cls_generation()
        assert not any(a.any() for a in RM.rtable_of(rtab))
        assert c.run_table()[0].stamp != rtab.stamp
    finally:
        c.close()


def test_struct_mirrors(built):
    from odp_amd import cls
    assert C.sizeof(cls.RunTab) == 256 + 512 + 256 + 8 and cls.RunTab.stamp.offset == 1024
    assert C.sizeof(cls.RunOut) == 8 * cls.RUN_OUT_WORDS == 192 and cls.RunOut.vec_need.offset == 64
    assert cls.RUN_DTYPE == RM.RUN_DTYPE and cls.RUN_DTYPE.itemsize == 16
    assert (cls.RUN_AGGR, cls.RUN_VEC, cls.RUN_VSLOTS) == (RM.AGGR, RM.VEC, RM.VSLOTS)
    assert cls.RUN_TILE % 64 == 0 and cls.RUN_GRID >= 1
    assert tuple(cls.run_out_dict(range(24))) == RM.FIELDS


def _args(cls, tab, rtab, out, n=0, cap=0):
    return (None, None, None, n, C.byref(tab) if tab else None, C.byref(rtab) if rtab else None, 0, None, None,
            cap, out.ctypes.data)


def test_library_entries_without_a_context(built):
    """The tables are checked first, with or without a device: more
    destinations than the bound is -E2BIG, a vector CoS without a size or with a
    slot past the bound -EINVAL.  No context: -ENODEV where there is no device
    (-EINVAL where there is one).  Nothing is written."""
    from odp_amd import cls
    L = cls.lib()
    out = np.zeros(24, np.uint64)
    t = C.c_uint64(99)
    good = cls.run_tab([], [], [])
    big = cls.enq_tab([], [], [], cls.ENQ_DST_MAX + 1)
    tab = cls.enq_tab([], [], [], 2)
    novmax = cls.run_tab([0, cls.RUN_VEC], [5, 0], [0, 0])
    badslot = cls.run_tab([cls.RUN_VEC], [5], [cls.RUN_VSLOTS])
    unused = cls.run_tab([cls.RUN_AGGR, 0], [0, 0], [200, 99])   # no VEC bit: vmax and vslot mean nothing
    no_ctx = -errno.ENODEV if L.mi_cls_device_count() <= 0 else -errno.EINVAL
    for etab, rtab, rc in ((big, good, -errno.E2BIG), (tab, novmax, -errno.EINVAL), (tab, badslot, -errno.EINVAL),
                           (None, good, -errno.EINVAL), (tab, None, -errno.EINVAL), (tab, good, no_ctx),
                           (tab, unused, no_ctx)):
        a = _args(cls, etab, rtab, out)
        assert L.mi_cls_enq_runs(*a, None) == rc
        assert L.mi_cls_enq_runs_host(*a) == rc
        t.value = 99
        assert L.mi_cls_enq_runs_host_submit(*a, C.byref(t)) == rc and t.value == 0
    assert L.mi_cls_enq_runs_host_submit(*_args(cls, tab, good, out), None) == -errno.EINVAL
    assert L.mi_cls_enq_runs_host_wait(None, 1) == no_ctx
    assert not out.any()


def test_pktio_entries_of_an_empty_batch(built):
    """The pktio forms create the context on first use: -ENODEV without a GPU;
    with one, an empty batch's out is all zeros."""
    from odp_amd import cls
    have = cls.lib().mi_cls_device_count() > 0
    c = cls.Classifier(gpu=0)
    try:
        c.apply([R.cos("a", queue=11), ("default", 0)])
        res, ln, seq = np.zeros(0, R.RESULT_DTYPE), np.zeros(0, np.uint16), np.zeros(0, np.uint32)
        runs = np.zeros(0, cls.RUN_DTYPE)
        for submit in (False, True):
            out = np.full(24, 7, np.uint64)
            if have:
                c.enq_runs_host(res, ln, seq, runs, out, submit=submit)
                assert not out.any()
            else:
                with pytest.raises(RuntimeError, match=f"{-errno.ENODEV}"):
                    c.enq_runs_host(res, ln, seq, runs, out, submit=submit)
    finally:
        c.close()
