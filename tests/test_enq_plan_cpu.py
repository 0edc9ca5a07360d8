"""The enqueue plan without a GPU: the model (tests/enq_model.py) against a
stable argsort, the table builder odp_amd_cls_enqtab_fill against the control
plane it reads, and what the library entries answer without a device.
"""
import ctypes as C
import errno

import numpy as np
import pytest

from odp_amd import rules as R
from tests import enq_model as M


@pytest.mark.parametrize("seed,n,ndst", [(1, 0, 3), (2, 1, 1), (3, 500, 1), (4, 3000, 7), (5, 3000, 300),
                                         (6, 9000, 8192), (7, 2000, 0)])
def test_model_is_a_stable_sort(seed, n, ndst):
    """plan() -- the per-record loop -- equals np.argsort(kind="stable") over
    the keys, on random records of every outcome, stale ones among them."""
    rng = np.random.default_rng(seed)
    table, entry_of = M.make_table(rng, ndst)
    dst = M.distribution(rng, "mixed", n, ndst) if ndst else M.drops(n)
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    # records the table does not map: random (cos, queue) on a fifth of them
    wild = rng.integers(0, 5, n) == 0
    rec["outcome"][wild] = M.OUT_ENQ
    rec["cos"][wild] = rng.integers(0, 256, int(wild.sum()))
    rec["queue"][wild] = rng.integers(0, 70, int(wild.sum()))
    perm, gbeg, ctr = M.plan(rec, lens, table)
    k, stale = M.keys(rec, table)
    assert np.array_equal(perm, np.argsort(k, kind="stable"))
    assert np.array_equal(gbeg, np.concatenate([[0], np.cumsum(np.bincount(k, minlength=ndst + 1))]))
    assert gbeg[0] == 0 and gbeg[-1] == n and gbeg.shape[0] == ndst + 2
    assert ctr["stale"] == int(stale.sum()) and (n == 0 or ndst == 0 or ctr["stale"] > 0 or n < 10)
    assert ctr["delivered"] == int(gbeg[ndst])
    sperm, sgbeg, sctr = M.plan_sorted(rec, lens, table)
    assert np.array_equal(perm, sperm) and np.array_equal(gbeg, sgbeg) and ctr == sctr


def test_model_counters_by_hand():
    """Each counter's rule on records written out one by one."""
    table = (np.array([2] + [0] * 255, np.uint8), np.zeros(256, np.uint16),
             np.array([1, 0] + [0xFFFF] * (M.ENT - 2), np.uint16), 2)
    rows = [  # err, outcome, cos, queue, len
        (0, M.OUT_ENQ, 0, 0, 100),          # -> id 1
        (4, M.OUT_ENQ, 0, 1, 200),          # -> id 0, an error: delivered, not in packets
        (0, M.OUT_COS_DROP, 0, 0, 300),     # silent
        (0, M.OUT_DISCARD, 0, 0, 400),
        (1, M.OUT_PARSE_DROP, 0, 0, 500),   # one error, not two
        (0, M.OUT_PARSE_DROP, 0, 0, 600),
        (0, M.OUT_LOOP, 0, 0, 700),
        (0, M.OUT_ENQ, 0, 2, 800),          # slot at the CoS's count: stale
        (0, M.OUT_ENQ, 1, 0, 900),          # a CoS without queues: stale
        (0, M.OUT_ENQ, 0, 1, 65535),        # -> id 0
        (8, M.OUT_DISCARD, 255, 9, 0),      # an error and a discard
    ]
    rec = np.zeros(len(rows), R.RESULT_DTYPE)
    for i, (err, outcome, cos, queue, _) in enumerate(rows):
        rec[i]["err"], rec[i]["outcome"], rec[i]["cos"], rec[i]["queue"] = err, outcome, cos, queue
    lens = np.array([r[4] for r in rows], np.uint16)
    perm, gbeg, ctr = M.plan(rec, lens, table)
    assert perm.tolist() == [1, 9, 0, 2, 3, 4, 5, 6, 7, 8, 10]
    assert gbeg.tolist() == [0, 2, 3, 11]
    assert ctr == {"in_errors": 4, "in_discards": 3, "packets": 2, "octets": 100 + 65535, "delivered": 3,
                   "stale": 2}


@pytest.fixture
def classifier(built):
    from odp_amd.cls import Classifier
    c = Classifier(gpu=0)
    yield c
    c.close()


def test_enqtab_fill(classifier):
    """Two CoS on one queue share an id, a hash CoS of 4 queues has 4 ids, a
    drop CoS no entries; ids in order of first appearance; ndst and queues[]
    exact; the generation is the control plane's."""
    c = classifier
    prog = [R.cos("a", queue=11), R.cos("b", queue=22), R.cos("drop", action=1, queue=33),
            R.cos("h", num_queue=4, hash_proto=R.HP_IPV4_UDP), R.cos("a2", queue=11), R.cos("c", queue=5),
            ("default", 0)]
    cos, _ = c.apply(prog)
    tab, queues, gen = c.enq_table()
    assert gen == c.L.odp_amd_cls_generation()
    nq, q0, ent, ndst = M.table_of(tab)
    idx = [int(c.L.odp_cos_to_u64(h)) - 1 for h in cos]   # cos_t.index of each: the handle less one
    hq = (C.c_void_p * 4)()
    assert c.L.odp_cls_cos_queues(cos[3], hq, 4) == 4
    hash_queues = [int(hq[j]) for j in range(4)]
    assert len(set(hash_queues)) == 4
    assert ndst == 7 and tab.ndst == 7
    assert idx == sorted(idx)   # created in index order: first appearance is creation order
    assert queues == [11, 22] + hash_queues + [5]
    assert [int(nq[i]) for i in idx] == [1, 1, 0, 4, 1, 1]
    assert int(nq.sum()) == 8 and np.count_nonzero(nq) == 5
    ids = [ent[int(q0[i]): int(q0[i]) + int(nq[i])].tolist() for i in idx]
    assert ids == [[0], [1], [], [2, 3, 4, 5], [0], [6]]
    # (cos, slot) -> queue is what the data path's lookup says
    for i in idx:
        for j in range(int(nq[i])):
            assert queues[ent[int(q0[i]) + j]] == (c.L.odp_amd_cls_queue_of(i, j) or 0)
    # a rewritten table has a new stamp; a control-plane change moves the generation
    tab2, queues2, gen2 = c.enq_table()
    assert tab2.stamp != tab.stamp and gen2 == gen and queues2 == queues
    c.apply([R.cos("d", queue=77)])
    tab3, queues3, gen3 = c.enq_table()
    assert gen3 != gen and queues3 == queues + [77] and tab3.ndst == 8


def test_enqtab_fill_empty_and_full(built):
    """No CoS: no destinations.  Thirty hash CoS of 32 queues (the queue
    table holds 1024): 960 ids, entry k's id is k.  The API's limits, 255 CoS
    of 32 hash queues, fit the table's bounds."""
    from odp_amd.cls import Classifier, ENQ_DST_MAX, ENQ_ENT
    assert 255 * 32 <= min(ENQ_DST_MAX, ENQ_ENT)
    c = Classifier(gpu=0)
    try:
        tab, queues, _ = c.enq_table()
        assert tab.ndst == 0 and queues == [] and not np.ctypeslib.as_array(tab.cos_nq).any()
        for i in range(30):
            assert c.cos_create(f"h{i}", num_queue=32, hash_proto=R.HP_IPV4_UDP)
        tab, queues, _ = c.enq_table()
        assert tab.ndst == 960 and len(set(queues)) == 960
        assert np.array_equal(np.ctypeslib.as_array(tab.ent_dst)[:960], np.arange(960))
        assert np.ctypeslib.as_array(tab.cos_nq)[:31].tolist() == [32] * 30 + [0]
    finally:
        c.close()


def test_enqtab_fill_bad_arguments(built):
    from odp_amd import cls
    L = cls.lib()
    nd, gen = C.c_uint32(), C.c_uint64()
    q = (C.c_void_p * cls.ENQ_DST_MAX)()
    assert L.odp_amd_cls_enqtab_fill(None, q, C.byref(nd), C.byref(gen)) == -errno.EINVAL
    assert L.odp_amd_cls_enqtab_fill(C.byref(cls.EnqTab()), None, C.byref(nd), C.byref(gen)) == -errno.EINVAL


def test_struct_mirrors(built):
    from odp_amd import cls
    assert C.sizeof(cls.EnqTab) == 8 + 256 + 512 + 2 * cls.ENQ_ENT + 8
    assert cls.EnqTab.ent_dst.offset == 776 and cls.EnqTab.stamp.offset % 8 == 0
    assert C.sizeof(cls.EnqOut) == 48 and len(cls.ENQ_OUT_FIELDS) == 6
    assert cls.ENQ_OUT_FIELDS == M.FIELDS


def test_library_entries_without_a_context(built):
    """More destinations than the bound: -E2BIG, with or without a device.  No
    context: -ENODEV where there is no device (-EINVAL where there is one)."""
    from odp_amd import cls
    L = cls.lib()
    tab = cls.enq_tab([], [], [], cls.ENQ_DST_MAX + 1)
    gbeg = np.zeros(4, np.uint32)
    out = np.zeros(6, np.uint64)
    t = C.c_uint64(99)
    dev = (None, None, None, 0, C.byref(tab), None, gbeg.ctypes.data, out.ctypes.data)
    assert L.mi_cls_enq_plan(*dev, None) == -errno.E2BIG
    assert L.mi_cls_enq_plan_host(*dev) == -errno.E2BIG
    assert L.mi_cls_enq_plan_host_submit(*dev, C.byref(t)) == -errno.E2BIG and t.value == 0
    tab = cls.enq_tab([], [], [], 2)
    dev = (None, None, None, 0, C.byref(tab), None, gbeg.ctypes.data, out.ctypes.data)
    no_ctx = -errno.ENODEV if L.mi_cls_device_count() <= 0 else -errno.EINVAL
    assert L.mi_cls_enq_plan(*dev, None) == no_ctx
    assert L.mi_cls_enq_plan_host(*dev) == no_ctx
    assert L.mi_cls_enq_plan_host_submit(*dev, C.byref(t)) == no_ctx
    assert L.mi_cls_enq_plan_host_wait(None, 1) == no_ctx
    assert L.mi_cls_enq_plan(None, None, None, 0, None, None, gbeg.ctypes.data, out.ctypes.data, None) == \
        -errno.EINVAL
    assert not gbeg.any() and not out.any()


def test_pktio_entries_of_an_empty_batch(built):
    """The pktio forms create the context on first use: -ENODEV without a GPU;
    with one, an empty batch's plan is all zeros."""
    from odp_amd import cls
    have = cls.lib().mi_cls_device_count() > 0
    c = cls.Classifier(gpu=0)
    try:
        c.apply([R.cos("a", queue=11), ("default", 0)])
        res, ln, perm = np.zeros(0, R.RESULT_DTYPE), np.zeros(0, np.uint16), np.zeros(0, np.uint32)
        for submit in (False, True):
            gbeg, out = np.full(3, 7, np.uint32), np.full(6, 7, np.uint64)
            if have:
                c.enq_plan_host(res, ln, perm, gbeg, out, submit=submit)
                assert not gbeg.any() and not out.any()
            else:
                with pytest.raises(RuntimeError, match=f"{-errno.ENODEV}"):
                    c.enq_plan_host(res, ln, perm, gbeg, out, submit=submit)
    finally:
        c.close()
