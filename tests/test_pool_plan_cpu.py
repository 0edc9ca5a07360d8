"""The pool plan without a GPU: the model (tests/pool_model.py), loop against
numpy and against the receive chain's decide model; its composition with the
enqueue plan and the run plan against a per-packet statement of the reference's
loop; the table builder odp_amd_cls_pooltab_fill and odp_amd_cls_pool_own
through a C driver; and what the library entries answer without a device.
"""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

from odp_amd import rules as R
from tests import enq_model as M
from tests import pool_model as PM
from tests import rt_helpers as H
from tests import run_model as RM
from tests import rx_model as RX

POOLTAB_DRIVER = os.path.join(H.ROOT, "tests", "_bin", "pooltab_driver")
HAVES = ("zero", "small", "exact", "unlimited")


def wild_records(rng, n, ndst=40):
    """Random records of every outcome over a random enqueue table, a ninth of
    them enqueue records of any CoS and queue (stale ones among them)."""
    table, entry_of = M.make_table(rng, ndst)
    dst = np.where(rng.integers(0, 4, n) == 0, M.drops(n), rng.integers(0, ndst, n))
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    wild = rng.integers(0, 9, n) == 0
    rec["outcome"][wild] = M.OUT_ENQ
    rec["cos"][wild] = rng.integers(0, 256, int(wild.sum()))
    rec["queue"][wild] = rng.integers(0, 70, int(wild.sum()))
    return rec, lens, table


def have_of(kind, rng, rec, lens, own, ptable):
    """have[] of a kind, from the batch's need; base[] with it: the slots'
    packets one after another from a random start."""
    need = np.array(PM.plan_pools_np(rec, lens, own, ptable, [PM.UNLIMITED] * PM.SLOTS, [0] * PM.SLOTS)[3]["need"])
    if kind == "zero":
        have = np.zeros(PM.SLOTS, np.int64)
    elif kind == "small":
        have = need // 3
    elif kind == "exact":
        have = need.copy()
    else:
        have = np.full(PM.SLOTS, PM.UNLIMITED, np.int64)
    room = np.where(have == PM.UNLIMITED, need, have)
    base = int(rng.integers(0, 1000)) + np.cumsum(room) - room
    return have.tolist(), base.tolist()


@pytest.mark.parametrize("kind", HAVES)
@pytest.mark.parametrize("nslot", [1, 3, 16])
@pytest.mark.parametrize("seed,n", [(1, 0), (2, 1), (3, 500), (4, 3000), (5, 5000)])
def test_model_pair(seed, n, nslot, kind):
    """plan_pools() -- the per-record loop -- equals plan_pools_np() on random
    records of every outcome, CoS without a slot and with a slot past nslot,
    with and without own[]."""
    rng = np.random.default_rng(seed * 100 + nslot)
    rec, lens, _ = wild_records(rng, n)
    ptable = PM.make_ptable(rng, nslot)
    for own in (None, PM.make_own(rng, rec, ptable)):
        have, base = have_of(kind, rng, rec, lens, own, ptable)
        a = PM.plan_pools(rec, lens, own, ptable, have, base)
        PM.same(a, PM.plan_pools_np(rec, lens, own, ptable, have, base))
        res_out, dec, idx, out = a
        fate = dec & 15
        assert [int((fate == f).sum()) for f in (1, 2, 3, 4)] == [out[k] for k in ("inplace", "fresh", "too_long",
                                                                                 "shorted")]
        assert sum(out["used"]) == out["fresh"] and sum(out["need"]) == out["fresh"] + out["shorted"]
        assert np.array_equal(idx != PM.NO_IDX, fate == PM.PF_FRESH)
        if kind in ("exact", "unlimited"):
            assert out["shorted"] == 0 and out["used"] == out["need"]
        if kind == "zero":
            assert out["fresh"] == 0
        # a slot's packets are taken in arrival order, one after another
        for k in range(nslot):
            got = idx[(fate == PM.PF_FRESH) & (dec >> 4 == k)]
            assert np.array_equal(got, base[k] + np.arange(out["used"][k]))
        changed = rec.view(np.uint8) != res_out.view(np.uint8)
        assert np.array_equal(changed.reshape(n, 16).any(axis=1) if n else np.zeros(0, bool),
                              np.isin(fate, (PM.PF_TOO_LONG, PM.PF_SHORT)))


def test_model_by_hand():
    """The rule on records written out one by one: slot 0 holds 100-byte
    frames, slot 1 1500-byte ones; CoS 0 and 3 on slot 0, CoS 1 on slot 1, CoS 2
    without a slot, CoS 4 on a slot past nslot."""
    cos_slot = np.full(256, 0xFF, np.uint8)
    cos_slot[[0, 1, 3, 4]] = [0, 1, 0, 2]
    ptable = (cos_slot, np.array([100, 1500], np.uint32), 2)
    rows = [  # outcome, cos, len, own
        (M.OUT_ENQ, 0, 60, 0),          # 0: slot 0 rank 0: FRESH
        (M.OUT_ENQ, 0, 101, 0),         # 1: longer than slot 0's packets: TOO_LONG, no rank
        (M.OUT_ENQ, 3, 100, 0),         # 2: slot 0 rank 1: FRESH (exactly the capacity)
        (M.OUT_ENQ, 0, 5000, 1),        # 3: already in slot 0: INPLACE though longer than slot_cap
        (M.OUT_DISCARD, 0, 60, 0),      # 4: NONE
        (M.OUT_ENQ, 2, 60, 0),          # 5: a CoS without a slot: NONE
        (M.OUT_ENQ, 1, 1500, 1),        # 6: in slot 0's packet, CoS of slot 1: slot 1 rank 0: FRESH
        (M.OUT_ENQ, 0, 60, 2),          # 7: slot 0 rank 2: the pool had two: SHORT
        (M.OUT_ENQ, 1, 60, 0),          # 8: slot 1 rank 1: FRESH
        (M.OUT_ENQ, 4, 60, 3),          # 9: cos_slot >= nslot: NONE, whatever own says
        (M.OUT_ENQ, 1, 60, 7),          # 10: own past nslot selects nothing: slot 1 rank 2: SHORT
    ]
    rec = np.zeros(len(rows), R.RESULT_DTYPE)
    for i, (outcome, cos, _, _) in enumerate(rows):
        rec[i]["outcome"], rec[i]["cos"], rec[i]["err"] = outcome, cos, 1 if i == 7 else 0
    lens = np.array([r[2] for r in rows], np.uint16)
    own = np.array([r[3] for r in rows], np.uint8)
    res_out, dec, idx, out = PM.plan_pools(rec, lens, own, ptable, [2, 2], [10, 20])
    F, T, S, I = PM.PF_FRESH, PM.PF_TOO_LONG, PM.PF_SHORT, PM.PF_INPLACE   # noqa: E741
    assert dec.tolist() == [F, T, F, I, 0, 0, F | 16, S, F | 16, 0, S | 16]
    no = PM.NO_IDX
    assert idx.tolist() == [10, no, 11, no, no, no, 20, no, 21, no, no]
    assert out == {"inplace": 1, "fresh": 4, "too_long": 1, "shorted": 2, "need": [3, 3] + [0] * 14,
                   "used": [2, 2] + [0] * 14}
    assert res_out["outcome"].tolist() == [0, 2, 0, 0, 2, 0, 0, 2, 0, 0, 2]
    assert res_out["err"].tolist() == rec["err"].tolist() and res_out["cos"].tolist() == rec["cos"].tolist()
    PM.same((res_out, dec, idx, out), PM.plan_pools_np(rec, lens, own, ptable, [2, 2], [10, 20]))
    # own == NULL: record 3 is too long and takes no rank, every other fate as before
    _, dec0, _, out0 = PM.plan_pools(rec, lens, None, ptable, [2, 2], [10, 20])
    assert dec0.tolist() == [F, T, F, T, 0, 0, F | 16, S, F | 16, 0, S | 16] and out0["too_long"] == 2
    # the need alone
    _, decu, idxu, outu = PM.plan_pools(rec, lens, own, ptable, [PM.UNLIMITED] * 2, [10, 20])
    assert outu["shorted"] == 0 and outu["need"][:2] == [3, 3] == outu["used"][:2]
    assert idxu.tolist() == [10, no, 11, no, no, no, 20, 12, 21, no, 22]


@pytest.mark.parametrize("kind", HAVES)
@pytest.mark.parametrize("seed,n,nslot", [(1, 1, 1), (2, 700, 3), (3, 8192, 16), (4, 4000, 4)])
def test_model_is_the_receive_chains_decide(seed, n, nslot, kind):
    """Fates, slots, ranks, need, used and in_discards are rx_model.decide's on
    the same inputs (every CoS has a slot there); RXF_FRESH with rank >= have
    is SHORT here."""
    rng = np.random.default_rng(seed)
    table, entry_of = M.make_table(rng, 24)
    dst = np.where(rng.integers(0, 5, n) == 0, M.drops(n), rng.integers(0, 24, n))
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    cos_slot = rng.integers(0, nslot, 256).astype(np.uint8)
    ptable = (cos_slot, PM.make_ptable(rng, nslot)[1], nslot)
    own = PM.make_own(rng, rec, ptable)
    have, base = have_of(kind, rng, rec, lens, own, ptable)
    tab = np.zeros((), RX.RXTAB_DTYPE)
    tab["flags"], tab["npool"] = RX.RXT_CLS, nslot
    tab["pool_cap"], tab["cos_pool"] = ptable[1], cos_slot
    tab["rt_slot"][:RX.RX_POOLS] = np.arange(1, RX.RX_POOLS + 1)   # pool handle p is slot p - 1
    got = np.arange(5000, 5000 + max(base) + n + 1)
    d = RX.decide(rec, lens, tab, have, base, got, pk=np.arange(n) + 1, ppool=own)
    res_out, dec, idx, out = PM.plan_pools_np(rec, lens, own, ptable, have, base)
    rfate, rslot, rrank = d.dec & 3, (d.dec >> 2) & 63, (d.dec >> 16).astype(np.int64)
    enq = rec["outcome"] == M.OUT_ENQ
    hv = np.asarray(PM._pad(have))[rslot]
    exp = np.select([rfate == RX.RXF_INPLACE, (rfate == RX.RXF_DISCARD) & enq,
                     (rfate == RX.RXF_FRESH) & (rrank < hv), rfate == RX.RXF_FRESH],
                    [PM.PF_INPLACE, PM.PF_TOO_LONG, PM.PF_FRESH, PM.PF_SHORT], PM.PF_NONE)
    assert np.array_equal(dec & 15, exp)
    assert np.array_equal(dec >> 4, rslot)
    fresh = exp == PM.PF_FRESH
    assert np.array_equal(idx[fresh], np.asarray(PM._pad(base))[rslot[fresh]] + rrank[fresh])
    assert out["need"] == list(d.out.need) and out["used"] == list(d.out.used)
    assert M.plan(res_out, lens, table)[2]["in_discards"] == d.out.in_discards + out["shorted"]


def consistent_batch(rng, n, nslot, ndst=30):
    """Records, lens, own and the two tables of one control plane: the CoS with
    queues are those with a slot; stale records come from CoS without either."""
    table, entry_of = M.make_table(rng, ndst)
    dst = np.where(rng.integers(0, 5, n) == 0, M.drops(n), rng.integers(0, ndst, n))
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    ptable = PM.make_ptable(rng, nslot, cos_nq=table[0])
    wild = rng.integers(0, 15, n) == 0
    rec["outcome"][wild] = M.OUT_ENQ
    rec["cos"][wild] = rng.integers(0, 256, int(wild.sum()))   # mostly CoS without queues; else a wrong queue
    rec["queue"][wild] = rng.integers(0, 70, int(wild.sum()))
    return rec, lens, PM.make_own(rng, rec, ptable), ptable, table


@pytest.mark.parametrize("kind", HAVES)
@pytest.mark.parametrize("seed,n,nslot", [(1, 0, 1), (2, 1, 1), (3, 600, 1), (4, 3000, 3), (5, 3000, 16)])
def test_composition_is_the_reference_loop(seed, n, nslot, kind):
    """enq_model.plan over res_out is the reference's loop with the pool switch
    in it, avail = have: each destination's survivors in order, the freed set
    and the four pktio counters."""
    rng = np.random.default_rng(seed)
    rec, lens, own, ptable, table = consistent_batch(rng, n, nslot)
    for ow in (None, own):
        have, base = have_of(kind, rng, rec, lens, ow, ptable)
        res_out, dec, idx, out = PM.plan_pools(rec, lens, ow, ptable, have, base)
        queues, freed, ctr = PM.reference_loop(rec, lens, ow, ptable, have, table)
        perm, gbeg, c = M.plan(res_out, lens, table)
        ndst = table[3]
        for g in range(ndst):
            assert perm[gbeg[g]:gbeg[g + 1]].tolist() == queues[g]
        assert perm[gbeg[ndst]:].tolist() == freed
        assert {k: c[k] for k in ctr} == ctr
        # the plan alone, without the pool switch, counts the losers as delivered
        c0 = M.plan(rec, lens, table)[2]
        assert c["in_discards"] == c0["in_discards"] + out["too_long"] + out["shorted"]
        assert c["in_errors"] == c0["in_errors"]
        losers = np.isin(dec & 15, (PM.PF_TOO_LONG, PM.PF_SHORT))
        assert not np.isin(np.nonzero(losers)[0], perm[:gbeg[ndst]]).any()


@pytest.mark.parametrize("kind", ["small", "exact"])
@pytest.mark.parametrize("seed,n,nslot", [(6, 2500, 3), (7, 2500, 16)])
def test_composition_with_the_run_plan(seed, n, nslot, kind):
    """run_model.plan_runs over res_out: no loser is in a run, the runs are
    those of the survivors alone and the vector counts follow."""
    rng = np.random.default_rng(seed)
    rec, lens, own, ptable, table = consistent_batch(rng, n, nslot, ndst=6)
    rtable = RM.make_rtable(rng)
    have, base = have_of(kind, rng, rec, lens, own, ptable)
    res_out, dec, _, out = PM.plan_pools(rec, lens, own, ptable, have, base)
    queues, freed, ctr = PM.reference_loop(rec, lens, own, ptable, have, table)
    seq, runs, ro = RM.plan_runs(res_out, lens, table, rtable)
    surv = sorted(i for q in queues for i in q)
    assert seq[:ro["delivered"]].tolist() == surv and seq[ro["delivered"]:].tolist() == freed
    assert {k: ro[k] for k in ctr} == ctr
    # the survivors alone, as a batch of their own
    _, runs2, ro2 = RM.plan_runs(rec[surv], lens[surv], table, rtable)
    assert np.array_equal(runs, runs2)
    assert (ro["nruns"], ro["vectors"], ro["vec_need"]) == (ro2["nruns"], ro2["vectors"], ro2["vec_need"])
    for burst in (64,):
        seqb, _, rob = RM.plan_runs(res_out, lens, table, rtable, burst)
        assert seqb[:rob["delivered"]].tolist() == surv


def test_pooltab_fill(built):
    """odp_amd_cls_pooltab_fill and odp_amd_cls_pool_own over a control plane
    made through the public API (tests/rt/pooltab_driver.c)."""
    r = subprocess.run([POOLTAB_DRIVER], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0] == "fill 0 nslot 3 gen_ok 1 stamp_new 1".split()
    cos = {ln[1]: int(ln[4]) for ln in lines if ln[0] == "cos"}
    assert cos == {"plain": 0, "a1": 1, "b1": 2, "a2": 1, "named": 0, "drop": 0xFF}
    # a pool's data capacity: the packet length rounded up to 64
    assert [ln[1:] for ln in lines if ln[0] == "slot"] == [["0", "pio", "cap", "1536"], ["1", "poolA", "cap", "256"],
                                                           ["2", "poolB", "cap", "9024"]]
    rest = {ln[0]: ln[1:] for ln in lines if ln[0] not in ("cos", "slot", "fill")}
    assert rest == {"unused": ["0"], "own": ["0", "1", "2", "3", "0", "0"],
                    "regen": ["1", "nslot", "4", "late", "3", "cap", "320"],
                    "full": ["0", "nslot", "16"], "over": [str(-errno.E2BIG)], "bad": [str(-errno.EINVAL)] * 3}


def test_pool_table_binding(built):
    """Classifier.pool_table() on a control plane whose CoS have no pool of
    their own: one slot, the enqueueing CoS on it."""
    from odp_amd import cls
    c = cls.Classifier(gpu=0)
    try:
        c.apply([R.cos("a", queue=11), R.cos("d", action=1), ("default", 0)])
        tab, pools, gen = c.pool_table(1536)
        cos_slot, slot_cap, nslot = PM.ptable_of(tab)
        assert nslot == 1 and len(pools) == 1 and gen == c.L.odp_amd_cls_generation()
        assert slot_cap[0] == 1536 and sorted(set(cos_slot.tolist())) == [0, 0xFF]
        assert int((cos_slot == 0).sum()) == 1
        assert c.pool_table(1536)[0].stamp != tab.stamp
    finally:
        c.close()


def test_struct_mirrors(built):
    from odp_amd import cls
    assert C.sizeof(cls.PoolTab) == 8 + 64 + 256 + 8 and cls.PoolTab.stamp.offset == 328
    assert C.sizeof(cls.PoolOut) == 4 * cls.POOL_OUT_WORDS == 160 and cls.PoolOut.need.offset == 32
    assert cls.POOL_OUT_DTYPE == PM.OUT_DTYPE and cls.POOL_OUT_DTYPE.itemsize == 160
    assert (cls.POOL_NONE, cls.POOL_INPLACE, cls.POOL_FRESH, cls.POOL_TOO_LONG, cls.POOL_SHORT) == \
        (PM.PF_NONE, PM.PF_INPLACE, PM.PF_FRESH, PM.PF_TOO_LONG, PM.PF_SHORT)
    assert cls.POOL_SLOTS == PM.SLOTS and cls.POOL_NO_IDX == PM.NO_IDX and cls.POOL_UNLIMITED == PM.UNLIMITED
    assert cls.POOL_TILE == 1024 and cls.POOL_TILE % 64 == 0 and cls.POOL_GRID == 256
    t = cls.pool_tab([1, 0], [100, 200])
    assert PM.ptable_of(t)[0].tolist() == [1, 0] + [0xFF] * 254 and t.nslot == 2
    w = np.arange(40, dtype=np.uint32)
    assert cls.pool_out_dict(w)["need"] == list(range(8, 24)) and cls.pool_out_dict(w)["used"] == list(range(24, 40))


def _args(cls, tab, have, base, out, n=0, arrays=None):
    u = C.c_uint32 * cls.POOL_SLOTS
    a = arrays or (None,) * 6   # res, len, own, res_out, dec, idx
    return (None, a[0], a[1], a[2], n, C.byref(tab) if tab else None, u(*have) if have is not None else None,
            u(*base) if base is not None else None, a[3], a[4], a[5], out.ctypes.data if out is not None else None)


def test_library_entries_without_a_context(built):
    """The table and the packets are checked first, with or without a device:
    a NULL table, have or base, more slots than the bound, a batch past
    MI_CLS_MAX_BATCH, or packets whose indexes would reach 0xFFFFFFFF are
    -EINVAL.  No context: -ENODEV where there is no device (-EINVAL where there
    is one).  Nothing is written."""
    from odp_amd import cls
    L = cls.lib()
    out = np.zeros(40, np.uint32)
    t = C.c_uint64(99)
    z = [0] * cls.POOL_SLOTS
    good = cls.pool_tab([0], [100])
    many = cls.pool_tab([0], [100], nslot=cls.POOL_SLOTS + 1)
    no_ctx = -errno.ENODEV if L.mi_cls_device_count() <= 0 else -errno.EINVAL
    cases = [((None, z, z, out), -errno.EINVAL), ((good, None, z, out), -errno.EINVAL),
             ((good, z, None, out), -errno.EINVAL), ((many, z, z, out), -errno.EINVAL),
             ((good, z, z, out, 1 << 28), -errno.EINVAL),
             ((good, [5] + z[1:], [0xFFFFFFFB] + z[1:], out, 5), -errno.EINVAL),
             ((good, [cls.POOL_UNLIMITED] + z[1:], [0xFFFFFFFE] + z[1:], out, 1), -errno.EINVAL),
             ((good, z, z, out), no_ctx),
             # a slot that is not in use may hold anything; base + min(have, n) may reach 0xFFFFFFFE
             ((good, [0, 9], [0, 0xFFFFFFFF], out), no_ctx),
             ((good, [cls.POOL_UNLIMITED] + z[1:], [0xFFFFFFFE] + z[1:], out, 0), no_ctx)]
    for a, rc in cases:
        a = _args(cls, *a)
        assert L.mi_cls_pool_plan(*a, None) == rc
        assert L.mi_cls_pool_plan_host(*a) == rc
        t.value = 99
        assert L.mi_cls_pool_plan_host_submit(*a, C.byref(t)) == rc and t.value == 0
    assert L.mi_cls_pool_plan_host_submit(*_args(cls, good, z, z, out), None) == -errno.EINVAL
    assert L.mi_cls_pool_plan_host_wait(None, 1) == no_ctx
    assert not out.any()


def test_pktio_entries_of_an_empty_batch(built):
    """The pktio forms create the context on first use: -ENODEV without a GPU;
    with one, an empty batch's out is all zeros."""
    from odp_amd import cls
    have = cls.lib().mi_cls_device_count() > 0
    c = cls.Classifier(gpu=0)
    try:
        c.apply([R.cos("a", queue=11), ("default", 0)])
        tab = c.pool_table(1536)[0]
        res, ln = np.zeros(0, R.RESULT_DTYPE), np.zeros(0, np.uint16)
        w = np.zeros(0, np.uint32)
        z = [0] * cls.POOL_SLOTS
        for submit in (False, True):
            out = np.full(40, 7, np.uint32)
            if have:
                c.pool_plan_host(res, ln, None, z, z, res, w, w, out, tab, submit=submit)
                assert not out.any()
            else:
                with pytest.raises(RuntimeError, match=f"{-errno.ENODEV}"):
                    c.pool_plan_host(res, ln, None, z, z, res, w, w, out, tab, submit=submit)
    finally:
        c.close()
