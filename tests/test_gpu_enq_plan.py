"""The enqueue plan on the GPU (mi_cls_enq_plan / odp_amd_cls_enq_plan and
their host forms) against the CPU model (tests/enq_model.py): perm[0:n], all
of gbeg and every counter compared for equality.  Every output word holds
poison before each call, with a guard word past each array.

The model is the per-record loop (enq_model.plan) for batches up to LOOP_MAX
records and its stable-sort statement (plan_sorted, held equal to the loop by
tests/test_enq_plan_cpu.py) above, where a Python loop per record would take
seconds.
"""
import ctypes as C
import errno

import numpy as np
import pytest

from odp_amd import cls
from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import enq_model as M
from tests import zoo
from tests.helpers import oracle_run

pytestmark = pytest.mark.gpu

T, G = cls.ENQ_TILE, cls.ENQ_GRID
ONE_PASS = (1 << cls.ENQ_DIGIT) - 1   # the most destinations one digit pass groups
LOOP_MAX = 4 * T
POISON = 0xA5A5A5A5


@pytest.fixture(scope="module")
def ctx(built, gpu):
    c = cls.EnqContext(0)
    yield c
    c.close()


def model(rec, lens, table):
    return (M.plan if rec.shape[0] <= LOOP_MAX else M.plan_sorted)(rec, lens, table)


def tab_of(table):
    return cls.enq_tab(*table)


def check(got, exp, what):
    perm, gbeg, ctr = got
    eperm, egbeg, ectr = exp
    assert ctr == ectr, f"{what}: counters {ctr} != {ectr}"
    if not np.array_equal(gbeg, egbeg):
        g = int(np.nonzero(gbeg != egbeg)[0][0])
        raise AssertionError(f"{what}: gbeg[{g}] = {gbeg[g]:#x}, model {egbeg[g]} ({gbeg.shape[0]} words)")
    if not np.array_equal(perm, eperm):
        j = int(np.nonzero(perm != eperm)[0][0])
        raise AssertionError(f"{what}: perm[{j}] = {perm[j]:#x}, model {eperm[j]} (n {perm.shape[0]})")


def shape(n, ndst):
    """(digit passes, grid) the header's constants give a batch."""
    tiles = (n + T - 1) // T
    return (0 if n == 0 else 1 if ndst <= ONE_PASS else 2), min(G, tiles)


# ---- synthetic records ------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, G * T + 1)
NDSTS = (1, 2, 63, 64, 65, ONE_PASS, ONE_PASS + 1, 1024, 1025, 8192)


@pytest.mark.parametrize("ndst", NDSTS)
@pytest.mark.parametrize("n", SIZES)
def test_synthetic(ctx, n, ndst):
    """n x ndst under every distribution: all to one destination, round-robin,
    none delivered, only the last record delivered, a heavy skew, a mix.  Every
    outcome value, err on delivered and dropped records and lens 0 and 65535
    are among the records (enq_model.make_records)."""
    rng = np.random.default_rng(1000 * ndst + n)
    table, entry_of = M.make_table(rng, ndst)
    tab = tab_of(table)
    for name in M.DISTRIBUTIONS:
        rec, lens = M.make_records(rng, n, M.distribution(rng, name, n, ndst), entry_of, R.RESULT_DTYPE)
        got = ctx.plan(rec, lens, tab, poison=POISON)
        check(got, model(rec, lens, table), f"n {n} ndst {ndst} {name}")
        info = ctx.last_launch()
        assert (info[0], info[1], info[6]) == (128 + T // 64,) + shape(n, ndst), info
    if n >= T - 1:   # the mix
        assert got[2]["packets"] and got[2]["in_errors"] and got[2]["in_discards"] and got[2]["octets"]
        assert got[2]["delivered"] > got[2]["packets"]   # err set on delivered records too


def test_every_destination_once_descending(ctx):
    """n = ndst = 8192, record i to destination ndst - 1 - i: perm is the
    reversal and every group has one record."""
    n = ndst = 8192
    rng = np.random.default_rng(5)
    table, entry_of = M.make_table(rng, ndst)
    rec, lens = M.make_records(rng, n, np.arange(n)[::-1], entry_of, R.RESULT_DTYPE)
    got = ctx.plan(rec, lens, tab_of(table), poison=POISON)
    check(got, M.plan(rec, lens, table), "descending")
    assert np.array_equal(got[0], np.arange(n, dtype=np.uint32)[::-1])
    assert np.array_equal(got[1], np.minimum(np.arange(ndst + 2), n))


def test_long_runs_keep_arrival_order(ctx):
    """More tiles than blocks (each block walks several) with two destinations
    256 ids apart -- equal low digit, told apart by the second pass -- in long
    alternating runs."""
    n = 3 * G * T + 77
    rng = np.random.default_rng(6)
    table, entry_of = M.make_table(rng, 600)
    dst = np.where((np.arange(n) // 1500) % 2 == 0, 3, 259)
    dst[rng.integers(0, 50, n) == 0] = -1 - M.OUT_DISCARD
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    got = ctx.plan(rec, lens, tab_of(table), poison=POISON)
    check(got, model(rec, lens, table), "long runs")
    assert ctx.last_launch()[6] == G


# ---- stale table ------------------------------------------------------------
def test_stale_table(ctx):
    """Enqueue records the table does not map -- a CoS without queues, a slot
    at and one past the CoS's count, CoS 255, an entry past the table, an id
    at and past ndst -- go to the last group and are counted in `stale`;
    nothing else changes: the plan is that of the same batch with those
    records dropped silently."""
    rng = np.random.default_rng(7)
    ndst = 100
    (cos_nq, cos_q0, ent_dst, _), entry_of = M.make_table(rng, ndst)
    assert cos_nq[4] == 0 and cos_nq[255] == 0 and cos_nq[0] == M.NQ
    cos_nq[200], cos_q0[200] = 8, M.ENT - 4          # slots 4..7 lie past the table
    ent_dst[M.ENT - 4:] = [5, ndst, ndst + 1, 0xFFFF]   # an id at and past ndst
    table = (cos_nq, cos_q0, ent_dst, ndst)
    n = 3 * T + 5
    rec, lens = M.make_records(rng, n, M.distribution(rng, "mixed", n, ndst), entry_of, R.RESULT_DTYPE)
    rec["err"][::3] = 0
    stale = [(4, 0), (0, M.NQ), (0, M.NQ + 1), (255, 0), (255, 31), (200, 4), (200, 7), (200, 1), (200, 2),
             (200, 3), (0, 0xFFFF)]
    at = rng.choice(n, 40 * len(stale), replace=False)
    for j, i in enumerate(at):
        rec[i]["outcome"] = M.OUT_ENQ
        rec[i]["cos"], rec[i]["queue"] = stale[j % len(stale)]
    rec[at[0]]["err"] = 9   # a stale record with an error: counted in in_errors
    got = ctx.plan(rec, lens, tab_of(table), poison=POISON)
    exp = M.plan(rec, lens, table)
    check(got, exp, "stale")
    assert got[2]["stale"] == at.shape[0]
    assert set(at.tolist()) <= set(got[0][got[1][ndst]:].tolist())
    # (200, 0) is mapped: its entry's id is 5
    ok = rec.copy()
    ok[at[1]]["cos"], ok[at[1]]["queue"] = 200, 0
    got_ok = ctx.plan(ok, lens, tab_of(table), poison=POISON)
    check(got_ok, M.plan(ok, lens, table), "stale, one mapped")
    assert got_ok[2]["stale"] == at.shape[0] - 1 and at[1] in got_ok[0][got_ok[1][5]:got_ok[1][6]]
    # the same batch with the stale records dropped silently: only `stale` differs
    silent = rec.copy()
    silent["outcome"][at] = M.OUT_COS_DROP
    sp, sg, sc = M.plan(silent, lens, table)
    assert np.array_equal(got[0], sp) and np.array_equal(got[1], sg)
    assert dict(sc, stale=got[2]["stale"]) == got[2]


# ---- forms --------------------------------------------------------------------
def _case(seed, n, ndst, name="mixed"):
    rng = np.random.default_rng(seed)
    table, entry_of = M.make_table(rng, ndst)
    rec, lens = M.make_records(rng, n, M.distribution(rng, name, n, ndst), entry_of, R.RESULT_DTYPE)
    return table, rec, lens


def _host_arrays(n, ndst, pinned):
    """res, lens, perm (+ guard), gbeg (+ guard), out (+ guard), poisoned; and
    what to close."""
    counts = (n, n, n + 1, ndst + 3, 7)
    dts = (R.RESULT_DTYPE, np.uint16, np.uint32, np.uint32, np.uint64)
    if pinned:
        mem = [cls.PinnedArray((k * np.dtype(dt).itemsize + 15) // 16 * 16 + 16) for k, dt in zip(counts, dts)]
        arrs = [m.view(dt)[:k] for m, k, dt in zip(mem, counts, dts)]
    else:
        mem = []
        arrs = [np.zeros(k, dt) for k, dt in zip(counts, dts)]
    for a in arrs[2:]:
        a.view(np.uint32)[:] = POISON
    return arrs, mem


@pytest.mark.parametrize("submit", [False, True], ids=["wait", "submit"])
@pytest.mark.parametrize("pinned", [True, False], ids=["in_place", "staged"])
@pytest.mark.parametrize("n,ndst", [(0, 5), (1, 1), (T + 1, 65), (5 * T + 3, 1025)])
def test_host_forms(ctx, n, ndst, pinned, submit):
    """The host form in place (page-locked arrays) and staged (pageable), as
    one call and as submit / wait; nothing is written past an array."""
    table, rec, lens = _case(31 * n + ndst, n, ndst)
    (res, ln, perm, gbeg, out), mem = _host_arrays(n, ndst, pinned)
    try:
        res[:] = rec
        ln[:] = lens
        ctx.plan_host(res, ln, tab_of(table), perm, gbeg, out, submit=submit)
        assert perm[n] == POISON and gbeg[ndst + 2] == POISON and out[6] == (POISON << 32 | POISON)
        got = (perm[:n].copy(), gbeg[:ndst + 2].copy(), {k: int(v) for k, v in zip(M.FIELDS, out[:6])})
        check(got, model(rec, lens, table), f"host n {n} ndst {ndst}")
        assert np.array_equal(res, rec) and np.array_equal(ln, lens)   # the inputs are only read
    finally:
        for m in mem:
            m.close()


def test_submit_several_then_wait(ctx):
    """Tickets of the context's ring: more batches submitted than the ring
    holds, each with buffers of its own, waited for in order afterwards."""
    L = ctx.L
    cases = [_case(50 + k, 300 + 700 * k, (3, 300)[k % 2]) for k in range(10)]
    tabs = [tab_of(c[0]) for c in cases]
    bufs, tickets = [], []
    for (table, rec, lens), tab in zip(cases, tabs):
        n, ndst = rec.shape[0], table[3]
        arrs, _ = _host_arrays(n, ndst, pinned=False)
        arrs[0][:], arrs[1][:] = rec, lens
        t = C.c_uint64()
        rc = L.mi_cls_enq_plan_host_submit(ctx.ctx, arrs[0].ctypes.data, arrs[1].ctypes.data, n, C.byref(tab),
                                           arrs[2].ctypes.data, arrs[3].ctypes.data, arrs[4].ctypes.data,
                                           C.byref(t))
        assert rc == 0 and t.value > (tickets[-1] if tickets else 0)
        bufs.append(arrs)
        tickets.append(t.value)
    for (table, rec, lens), arrs, t in zip(cases, bufs, tickets):
        assert L.mi_cls_enq_plan_host_wait(ctx.ctx, t) == 0
        n, ndst = rec.shape[0], table[3]
        got = (arrs[2][:n], arrs[3][:ndst + 2], {k: int(v) for k, v in zip(M.FIELDS, arrs[4][:6])})
        check(got, M.plan(rec, lens, table), f"ticket {t}")
    assert L.mi_cls_enq_plan_host_wait(ctx.ctx, tickets[-1] + 1) == -errno.EINVAL


def test_large_then_small_on_one_context(built, gpu):
    """A small call after a large one on a fresh context sees nothing of the
    first one's scratch or counters; then a larger one again (the scratch
    grows), in both digit-pass shapes."""
    c = cls.EnqContext(0)
    try:
        for k, (n, ndst) in enumerate([(40 * T + 9, 2000), (70, 2000), (3, 2), (0, 2), (90 * T, 2), (T, 300)]):
            table, rec, lens = _case(70 + k, n, ndst, "skew" if k % 2 else "mixed")
            check(c.plan(rec, lens, tab_of(table), poison=POISON), model(rec, lens, table), f"call {k}")
    finally:
        c.close()


def test_two_tables_then_the_first_again(ctx):
    """The device keeps the copy of the last table it was given: A, B, A
    again, then A rewritten in place under a new stamp."""
    rng = np.random.default_rng(9)
    ta, entry_a = M.make_table(rng, 40)
    tb, _ = M.make_table(rng, 40)
    assert not np.array_equal(ta[2], tb[2])
    rec, lens = M.make_records(rng, 2 * T, M.distribution(rng, "mixed", 2 * T, 40), entry_a, R.RESULT_DTYPE)
    tab_a, tab_b = tab_of(ta), tab_of(tb)
    ea, eb = M.plan(rec, lens, ta), M.plan(rec, lens, tb)
    assert not np.array_equal(ea[0], eb[0])
    for what, tab, exp in (("A", tab_a, ea), ("B", tab_b, eb), ("A again", tab_a, ea), ("A once more", tab_a, ea)):
        check(ctx.plan(rec, lens, tab, poison=POISON), exp, what)
    np.ctypeslib.as_array(tab_a.ent_dst)[:] = tb[2]
    np.ctypeslib.as_array(tab_a.cos_nq)[:] = tb[0]
    tab_a.stamp = tab_b.stamp + 1000
    check(ctx.plan(rec, lens, tab_a, poison=POISON), eb, "A rewritten")


def test_device_form_follows_a_launch_on_its_stream(ctx):
    """The device form is stream-ordered: records written by copies queued on
    a side stream just before it, planned on that stream."""
    import torch
    table, rec, lens = _case(12, 9 * T + 1, 700)
    n, ndst = rec.shape[0], 700
    tab = tab_of(table)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(dev)
    h_res = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).pin_memory()
    h_len = torch.from_numpy(lens.view(np.int16).copy()).pin_memory()
    t_res = torch.full((16 * n,), 0xA5, dtype=torch.uint8, device=dev)
    t_len = torch.zeros(n, dtype=torch.int16, device=dev)
    t_perm = torch.full((n,), -1, dtype=torch.int32, device=dev)
    t_gbeg = torch.full((ndst + 2,), -1, dtype=torch.int32, device=dev)
    t_out = torch.full((6,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        t_res.copy_(h_res, non_blocking=True)
        t_len.copy_(h_len, non_blocking=True)
        rc = ctx.plan_device(t_res.data_ptr(), t_len.data_ptr(), n, tab, t_perm.data_ptr(), t_gbeg.data_ptr(),
                             t_out.data_ptr(), side.cuda_stream)
    assert rc == 0
    side.synchronize()
    got = (t_perm.cpu().numpy().view(np.uint32), t_gbeg.cpu().numpy().view(np.uint32),
           {k: int(v) for k, v in zip(M.FIELDS, t_out.cpu().numpy().view(np.uint64))})
    check(got, model(rec, lens, table), "side stream")
    # and the next plan, on the default stream, is ordered after it
    check(ctx.plan(rec[:T], lens[:T], tab, poison=POISON), M.plan(rec[:T], lens[:T], table), "default stream")


# ---- errors ---------------------------------------------------------------------
def test_errors(ctx):
    """NULL arrays with n > 0 and a NULL gbeg / out / table: -EINVAL; ndst past
    the bound: -E2BIG; nothing is launched."""
    import torch
    table, rec, lens = _case(3, 10, 4)
    tab = tab_of(table)
    d = torch.zeros(4096, dtype=torch.int32, device="cuda:0")
    p = d.data_ptr()
    good = [p, p + 1024, 10, tab, p + 2048, p + 3072, p + 4096]
    assert ctx.plan_device(*good) == 0
    torch.cuda.synchronize()
    for k in (0, 1, 4, 5, 6):
        bad = list(good)
        bad[k] = 0
        assert ctx.plan_device(*bad) == -errno.EINVAL, k
    assert ctx.plan_device(p, p, 10, tab, p, p, p + 4) == -errno.EINVAL   # out not 8-byte aligned
    assert ctx.plan_device(0, 0, 0, tab, 0, p, p + 4096) == 0             # n == 0 needs no arrays
    torch.cuda.synchronize()
    big = cls.enq_tab(*table[:3], cls.ENQ_DST_MAX + 1)
    assert ctx.plan_device(p, p, 10, big, p, p, p) == -errno.E2BIG
    L = ctx.L
    gbeg, out = np.zeros(8, np.uint32), np.zeros(6, np.uint64)
    perm = np.zeros(10, np.uint32)
    t = C.c_uint64(5)
    assert L.mi_cls_enq_plan_host(ctx.ctx, None, lens.ctypes.data, 10, C.byref(tab), perm.ctypes.data,
                                  gbeg.ctypes.data, out.ctypes.data) == -errno.EINVAL
    assert L.mi_cls_enq_plan_host(ctx.ctx, rec.ctypes.data, lens.ctypes.data, 10, C.byref(tab), None,
                                  gbeg.ctypes.data, out.ctypes.data) == -errno.EINVAL
    assert L.mi_cls_enq_plan_host_submit(ctx.ctx, rec.ctypes.data, lens.ctypes.data, 10, C.byref(big),
                                         perm.ctypes.data, gbeg.ctypes.data, out.ctypes.data,
                                         C.byref(t)) == -errno.E2BIG and t.value == 0
    assert L.mi_cls_enq_plan_host_submit(ctx.ctx, rec.ctypes.data, lens.ctypes.data, 10, C.byref(tab),
                                         perm.ctypes.data, gbeg.ctypes.data, out.ctypes.data,
                                         None) == -errno.EINVAL
    assert L.mi_cls_enq_plan_host(None, rec.ctypes.data, lens.ctypes.data, 10, C.byref(tab), perm.ctypes.data,
                                  gbeg.ctypes.data, out.ctypes.data) == -errno.EINVAL   # a device, no context


# ---- end to end -----------------------------------------------------------------
def _end_to_end(prog, batch, what, min_delivered=1):
    """Classify on the GPU, plan on the pktio's context and the same stream;
    the model over the oracle's records."""
    exp_rec, _ = oracle_run(prog, batch)
    c = cls.Classifier(gpu=0)
    try:
        c.apply(prog)
        got_rec = c.classify(batch)
        assert np.array_equal(got_rec, exp_rec), what
        tab, queues, gen = c.enq_table()
        assert gen == c.L.odp_amd_cls_generation()
        got = c.enq_plan(got_rec, batch.len, tab, poison=POISON)
        table = M.table_of(tab)
        exp = model(exp_rec, batch.len, table)
        check(got, exp, what)
        perm, gbeg, ctr = got
        assert ctr["stale"] == 0 and ctr["delivered"] >= min_delivered
        # every delivered packet sits in the group of the queue the data path's lookup names
        for g in np.nonzero(np.diff(gbeg[:-1]))[0]:
            i = int(perm[gbeg[g]])
            assert queues[g] == (c.L.odp_amd_cls_queue_of(int(exp_rec[i]["cos"]), int(exp_rec[i]["queue"])) or 0)
        return got, exp_rec, queues
    finally:
        c.close()


def test_end_to_end_zoo(built, gpu):
    """The zoo's frames, error frames among them, under the everything program."""
    b, _ = zoo.zoo_batch()
    got, rec, _ = _end_to_end(zoo.prog_everything(), b, "zoo")
    assert got[2]["in_errors"] > 0 and np.count_nonzero(rec["err"]) > 0


def test_end_to_end_hash_cos_and_shared_queue(built, gpu):
    """A hash CoS of 4 queues, two CoS on one queue, a drop CoS."""
    frames = [pg.udp4_frame(size=60 + (i % 40), sport=1000 + i, dport=(53, 80, 443, 9)[i % 4]) for i in range(3000)]
    b = pg.batch_from_frames(frames)
    prog = [R.cos("default", queue=0x1100), R.cos("hash", num_queue=4, hash_proto=R.HP_IPV4_UDP),
            R.cos("shared", queue=0x1100), R.cos("drop", action=1, queue=0x3300), ("default", 0),
            ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 53)], 0, 1, 0), ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 80)], 0, 2, 3),
            ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 443)], 0, 3, 0)]
    got, rec, queues = _end_to_end(prog, b, "hash + shared")
    perm, gbeg, ctr = got
    assert len(queues) == 5 and queues[0] == 0x1100 and 0x3300 not in queues
    # the shared queue's group holds the packets of both CoS in arrival order
    g0 = perm[gbeg[0]:gbeg[1]]
    assert set(rec["cos"][g0].tolist()) == {0, 2} and np.all(np.diff(g0.astype(np.int64)) > 0)
    assert all(gbeg[g + 1] > gbeg[g] for g in range(1, 5))   # every hash queue got packets
    assert gbeg[6] - gbeg[5] == 750 and ctr["delivered"] == 2250   # the drop CoS' packets: the last group


def test_end_to_end_no_default_cos(built, gpu):
    """No default CoS: what matches no rule is discarded."""
    b, _ = zoo.zoo_batch()
    got, rec, _ = _end_to_end(zoo.prog_no_default(), b, "no default", min_delivered=0)
    assert got[2]["in_discards"] == np.count_nonzero(np.isin(rec["outcome"], (M.OUT_DISCARD, M.OUT_LOOP))) > 0


def test_end_to_end_config3_200k(built, gpu):
    """About 200 k packets of config 3's traffic."""
    b, prog = R.config3(200_000)
    got, _, queues = _end_to_end(prog, b, "config 3", min_delivered=100_000)
    assert got[1][-1] == 200_000 and len(queues) > 1
