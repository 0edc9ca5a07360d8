"""The pool plan on the GPU (mi_cls_pool_plan / odp_amd_cls_pool_plan and their
host forms) against the CPU model (tests/pool_model.py): every word of res_out,
dec, idx and out compared for equality.  Every output word holds poison before
each call, with a guard past each array.

The model is the per-record loop (pool_model.plan_pools) for batches up to
LOOP_MAX records and its numpy statement (plan_pools_np, held equal to the loop
by tests/test_pool_plan_cpu.py) above.  The shapes follow the kernels' exported
constants: T records per tile, at most G blocks.
"""
import ctypes as C
import errno

import numpy as np
import pytest

from odp_amd import cls
from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import enq_model as M
from tests import pool_model as PM
from tests import zoo
from tests.helpers import oracle_run

pytestmark = pytest.mark.gpu

T, G = cls.POOL_TILE, cls.POOL_GRID
LOOP_MAX = 4 * T
POISON = 0xA5A5A5A5
BIG = 600_011          # three tiles per block, the last block's run cut short
UNL = cls.POOL_UNLIMITED
Z = [0] * cls.POOL_SLOTS


@pytest.fixture(scope="module")
def ctx(built, gpu):
    c = cls.EnqContext(0)
    yield c
    c.close()


def model(rec, lens, own, ptable, have, base):
    return (PM.plan_pools if rec.shape[0] <= LOOP_MAX else PM.plan_pools_np)(rec, lens, own, ptable, have, base)


def check(got, exp, what):
    """got: (res_out, dec, idx, out) of a call whose outputs were poisoned."""
    res_out, dec, idx, out = got
    eres, edec, eidx, eout = exp
    assert out == eout, f"{what}: out {out} != {eout}"
    for name, a, b in (("dec", dec, edec), ("idx", idx, eidx)):
        if not np.array_equal(a, b):
            j = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{what}: {name}[{j}] = {a[j]:#x}, model {b[j]:#x} (n {a.shape[0]})")
    a, b = res_out.view(np.uint32).reshape(-1, 4), eres.view(np.uint32).reshape(-1, 4)
    if not np.array_equal(a, b):
        j = int(np.nonzero((a != b).any(axis=1))[0][0])
        raise AssertionError(f"{what}: res_out[{j}] = {res_out[j]}, model {eres[j]}")


def run(ctx, rec, lens, own, ptable, have, base, in_place=False, what=""):
    got = ctx.pools(rec, lens, own, cls.pool_tab(*ptable), have, base, poison=POISON, in_place=in_place)
    check(got, model(rec, lens, own, ptable, have, base), what)
    return got


def wild_records(rng, n, ndst=40):
    """Random records of every outcome, a ninth of them enqueue records of any
    CoS; lens of every size, 0 and 65535 among them."""
    table, entry_of = M.make_table(rng, ndst)
    dst = np.where(rng.integers(0, 4, n) == 0, M.drops(n), rng.integers(0, ndst, n))
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    wild = rng.integers(0, 9, n) == 0
    rec["outcome"][wild] = M.OUT_ENQ
    rec["cos"][wild] = rng.integers(0, 256, int(wild.sum()))
    return rec, lens, table


def need_of(rec, lens, own, ptable):
    return np.array(PM.plan_pools_np(rec, lens, own, ptable, [UNL] * 16, Z)[3]["need"])


def one_slot_records(n, cos=0, length=60):
    """n enqueue records of one CoS, nothing else."""
    rec = np.zeros(n, R.RESULT_DTYPE)
    rec["outcome"], rec["cos"] = M.OUT_ENQ, cos
    rec["in_flags"] = np.arange(n, dtype=np.uint32) * 2654435761 & 0xFFFFFFFF
    return rec, np.full(n, length, np.uint16)


# ---- batch sizes --------------------------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, G * T + 1, BIG)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n):
    """Random records over five slots, CoS without a slot and with a slot past
    nslot among them; own NULL (disjoint res_out) and given (in place); a third
    of each slot's need at hand, non-zero bases."""
    rng = np.random.default_rng(n + 1)
    rec, lens, _ = wild_records(rng, n)
    ptable = PM.make_ptable(rng, 5)
    for own, in_place in ((None, False), (PM.make_own(rng, rec, ptable), True)):
        need = need_of(rec, lens, own, ptable)
        have = (need // 3).tolist()
        base = (7 + np.cumsum(need) - need).tolist()
        got = run(ctx, rec, lens, own, ptable, have, base, in_place, what=f"n {n} in_place {in_place}")
        info = ctx.last_launch()
        assert (info[0], info[1], info[6]) == (256 + T // 64, 3 if n else 1, min(G, (n + T - 1) // T)), info
        assert info[2:6] == [0, 0, 0, 0]
    if n >= T - 1:
        out = got[3]
        # the generator's own sanity: every fate occurs
        assert out["inplace"] and out["fresh"] and out["too_long"] and out["shorted"] and not any(out["need"][5:])


# ---- ranks carried across waves, tiles and blocks ------------------------------
@pytest.mark.parametrize("one_slot", [False, True], ids=["slot_per_pair", "one_slot"])
def test_ranks_across_edges(ctx, one_slot):
    """3 G T records, three tiles per block, all NONE but pairs of frames of
    one slot: in one wave, in neighbouring waves, across a tile edge, across a
    whole tile without that slot, across a block edge and across many blocks.
    Only the carried counts can give the second frame of a pair its rank."""
    n = 3 * G * T
    B = 3 * T   # records per block
    pairs = [(10, 20), (3 * 64 + 60, 4 * 64 + 2), (2 * B + T - 1, 2 * B + T), (4 * B + 100, 4 * B + 2 * T + 100),
             (6 * B - 1, 6 * B), (10 * B + 17, 200 * B + 33)]
    rec = np.zeros(n, R.RESULT_DTYPE)
    rec["outcome"] = np.array(M.NOT_DELIVERED, np.uint8)[np.arange(n) % len(M.NOT_DELIVERED)]
    rec["cos"] = np.arange(n) % 251
    lens = np.full(n, 64, np.uint16)
    cos_slot = (np.arange(256) % 16).astype(np.uint8)
    ptable = (cos_slot, np.full(16, 1500, np.uint32), 16)
    for k, (a, b) in enumerate(pairs):
        for i in (a, b):
            rec["outcome"][i] = M.OUT_ENQ
            rec["cos"][i] = 3 if one_slot else 2 * k + 1
    base = [1000 * (s + 1) for s in range(16)]
    got = run(ctx, rec, lens, None, ptable, [UNL] * 16, base, what=f"one_slot {one_slot}")
    idx = got[2]
    flat = sorted(i for p in pairs for i in p)
    for k, (a, b) in enumerate(pairs):
        if one_slot:
            assert (idx[a], idx[b]) == (4000 + flat.index(a), 4000 + flat.index(b))
        else:
            assert (idx[a], idx[b]) == (base[2 * k + 1], base[2 * k + 1] + 1)
    assert int((idx != PM.NO_IDX).sum()) == 12 and got[3]["fresh"] == 12


@pytest.mark.parametrize("have", [0, 1, 63, 64, T - 1, T, T + 1, 3 * T, 3 * T + 1, 100 * 3 * T, UNL])
def test_have_cut_at_boundaries_whole_batch_on_one_slot(ctx, have):
    """Every record on slot 2 (three tiles per block): have cut at 0, at a wave,
    a tile and a block boundary and beside them, and unlimited; a non-zero base."""
    n = 2 * G * T + 5
    rec, lens = one_slot_records(n, cos=9)
    cos_slot = np.full(256, 0xFF, np.uint8)
    cos_slot[9] = 2
    ptable = (cos_slot, np.array([10, 10, 60], np.uint32), 3)
    got = run(ctx, rec, lens, None, ptable, [5, 5, have], [0, 0, 123456], what=f"have {have}")
    cut = min(have, n)
    assert np.array_equal(got[2][:cut], 123456 + np.arange(cut)) and np.all(got[2][cut:] == PM.NO_IDX)
    assert np.all(got[0]["outcome"][:cut] == M.OUT_ENQ) and np.all(got[0]["outcome"][cut:] == M.OUT_DISCARD)
    assert got[3]["need"][2] == n and got[3]["used"][2] == cut and got[3]["shorted"] == n - cut


def test_all_slots_in_one_wave(ctx):
    """64 records, four of each of the 16 slots in one wave, two packets at
    hand per slot, every slot with a base of its own."""
    rec, lens = one_slot_records(64)
    rec["cos"] = (np.arange(64) * 7) % 16
    ptable = ((15 - np.arange(256) % 16).astype(np.uint8), np.full(16, 60, np.uint32), 16)
    base = [50 * s + 3 for s in range(16)]
    got = run(ctx, rec, lens, None, ptable, [2] * 16, base, what="16 slots")
    assert got[3]["need"] == [4] * 16 and got[3]["used"] == [2] * 16 and got[3]["shorted"] == 32


def test_slots_and_own_past_the_table(ctx):
    """cos_slot >= nslot (0xFF and in-range values of an unused slot) selects
    nothing, whatever own says; own values past nslot select nothing."""
    rng = np.random.default_rng(5)
    n = 3 * T + 17
    rec, lens = one_slot_records(n)
    rec["cos"] = rng.integers(0, 256, n)
    cos_slot = rng.integers(0, 16, 256).astype(np.uint8)
    cos_slot[rng.integers(0, 4, 256) == 0] = 0xFF
    ptable = (cos_slot, np.array([100] * 6 + [7] * 10, np.uint32), 6)   # slots 6 .. 15 are not in use
    own = rng.integers(0, 256, n).astype(np.uint8)
    own[::5] = (cos_slot[rec["cos"][::5]].astype(np.int64) + 1).astype(np.uint8)   # 0xFF + 1 wraps to 0: none
    got = run(ctx, rec, lens, own, ptable, [UNL] * 6 + [3] * 10, [100 * s for s in range(16)], what="past")
    past = cos_slot[rec["cos"]] >= 6
    assert past.sum() > n // 2 and np.all(got[1][past] == 0) and np.all(got[2][past] == PM.NO_IDX)
    assert not any(got[3]["need"][6:]) and got[3]["inplace"] > n // 20
    # without own every record of a slot in use is ranked
    got = run(ctx, rec, lens, None, ptable, [UNL] * 16, Z, what="past, no own")
    assert got[3]["inplace"] == 0 and got[3]["fresh"] == int((~past).sum())


# ---- forms ------------------------------------------------------------------------------
def _case(seed, n, nslot=4):
    rng = np.random.default_rng(seed)
    rec, lens, _ = wild_records(rng, n)
    ptable = PM.make_ptable(rng, nslot)
    own = PM.make_own(rng, rec, ptable)
    need = need_of(rec, lens, own, ptable)
    return rec, lens, own, ptable, (need // 2).tolist(), (11 + np.cumsum(need) - need).tolist()


NAMES = ("res", "len", "own", "res_out", "dec", "idx", "out")


def _host_arrays(n, pinned):
    """res, lens, own, res_out (+ guard), dec (+ guard), idx (+ guard), out (+
    guard), the outputs poisoned; pinned: the names of the page-locked ones."""
    counts = (n, n, n, n + 1, n + 1, n + 1, 42)
    dts = (R.RESULT_DTYPE, np.uint16, np.uint8, R.RESULT_DTYPE, np.uint32, np.uint32, np.uint32)
    arrs, mem = {}, []
    for name, k, dt in zip(NAMES, counts, dts):
        if name in pinned:
            m = cls.PinnedArray((k * np.dtype(dt).itemsize + 15) // 16 * 16 + 16)
            mem.append(m)
            arrs[name] = m.view(dt)[:k]
        else:
            arrs[name] = np.zeros(k, dt)
    for name in NAMES[3:]:
        arrs[name].view(np.uint32)[:] = POISON
    return arrs, mem


def _host_result(a, n, res_out=None):
    ro = a["res_out"] if res_out is None else res_out
    assert a["dec"][n] == POISON and a["idx"][n] == POISON and np.all(a["out"][40:] == POISON)
    assert np.all(a["res_out"].view(np.uint32)[4 * n if res_out is None else 0:] == POISON)
    return ro[:n].copy(), a["dec"][:n].copy(), a["idx"][:n].copy(), cls.pool_out_dict(a["out"][:40])


@pytest.mark.parametrize("submit", [False, True], ids=["wait", "submit"])
@pytest.mark.parametrize("pinned", [NAMES, (), tuple(x for x in NAMES if x != "dec"),
                                    tuple(x for x in NAMES if x != "own")],
                         ids=["in_place", "staged", "dec_pageable", "own_pageable"])
@pytest.mark.parametrize("n", [0, 1, T + 1, 5 * T + 3])
def test_host_forms(ctx, n, pinned, submit):
    """The host form in place (page-locked arrays) and staged (pageable arrays,
    or one pageable array among page-locked ones), as one call and as submit /
    wait, with own given and NULL, res_out disjoint and res itself; nothing is
    written past an array and the inputs are only read."""
    rec, lens, own, ptable, have, base = _case(31 * n + len(pinned), n)
    tab = cls.pool_tab(*ptable)
    for with_own, same in ((True, False), (False, True)):
        a, mem = _host_arrays(n, pinned)
        try:
            a["res"][:], a["len"][:], a["own"][:] = rec, lens, own
            ow = a["own"] if with_own else None
            ro = a["res"] if same else a["res_out"][:n]
            ctx.pools_host(a["res"], a["len"], ow, tab, have, base, ro, a["dec"][:n], a["idx"][:n], a["out"],
                           submit=submit)
            got = _host_result(a, n, a["res"] if same else None)
            check(got, model(rec, lens, own if with_own else None, ptable, have, base),
                  f"host n {n} pinned {pinned} own {with_own} same {same}")
            assert np.array_equal(a["len"], lens) and np.array_equal(a["own"], own)
            assert same or np.array_equal(a["res"], rec)
        finally:
            for m in mem:
                m.close()


@pytest.mark.parametrize("pinned", [NAMES, ()], ids=["in_place", "staged"])
def test_two_tickets_outstanding(ctx, pinned):
    """Two batches submitted, each with buffers of its own, before the first is
    waited for; then ten in a row, more than the ring holds."""
    cases = [_case(50 + k, 300 + 700 * k) for k in range(10)]
    tabs = [cls.pool_tab(*c[3]) for c in cases]
    bufs, tickets, keep = [], [], []
    try:
        for (rec, lens, own, ptable, have, base), tab in zip(cases, tabs):
            n = rec.shape[0]
            a, mem = _host_arrays(n, pinned)
            keep += mem
            a["res"][:], a["len"][:], a["own"][:] = rec, lens, own
            t = ctx.pools_host(a["res"], a["len"], a["own"], tab, have, base, a["res_out"][:n], a["dec"][:n],
                               a["idx"][:n], a["out"], submit="ticket")
            assert t > (tickets[-1] if tickets else 0)
            bufs.append(a)
            tickets.append(t)
            if len(tickets) == 2:   # two outstanding: the first one's result is its own
                ctx.pools_wait(tickets[0])
                check(_host_result(bufs[0], cases[0][0].shape[0]), PM.plan_pools(*cases[0]), "first of two")
        for (rec, lens, own, ptable, have, base), a, t in zip(cases, bufs, tickets):
            ctx.pools_wait(t)
            check(_host_result(a, rec.shape[0]), PM.plan_pools(rec, lens, own, ptable, have, base), f"ticket {t}")
        assert ctx.L.mi_cls_pool_plan_host_wait(ctx.ctx, tickets[-1] + 1) == -errno.EINVAL
    finally:
        for m in keep:
            m.close()


def test_large_then_small_and_tables_again(built, gpu):
    """On a fresh context: a small call after a large one sees nothing of the
    first one's counts, staged and on the device; the device keeps the last
    table's copy: A, B, A again, then A rewritten in place under a new stamp."""
    c = cls.EnqContext(0)
    try:
        for k, n in enumerate([40 * T + 9, 70, 3, 0, 90 * T, T]):
            rec, lens, own, ptable, have, base = _case(70 + k, n)
            run(c, rec, lens, own, ptable, have, base, what=f"call {k}")
            a, _ = _host_arrays(n, ())
            a["res"][:], a["len"][:], a["own"][:] = rec, lens, own
            c.pools_host(a["res"], a["len"], a["own"], cls.pool_tab(*ptable), have, base, a["res_out"][:n],
                         a["dec"][:n], a["idx"][:n], a["out"])
            check(_host_result(a, n), model(rec, lens, own, ptable, have, base), f"staged call {k}")
        rec, lens, own, pa, have, base = _case(80, 2 * T)
        pb = (pa[0][::-1].copy(), pa[1], pa[2])
        tab_a, tab_b = cls.pool_tab(*pa), cls.pool_tab(*pb)
        ea, eb = PM.plan_pools(rec, lens, own, pa, have, base), PM.plan_pools(rec, lens, own, pb, have, base)
        assert ea[3] != eb[3]
        for what, t, exp in (("A", tab_a, ea), ("B", tab_b, eb), ("A again", tab_a, ea), ("A once more", tab_a, ea)):
            check(c.pools(rec, lens, own, t, have, base, poison=POISON), exp, what)
        np.ctypeslib.as_array(tab_a.cos_slot)[:] = pb[0]
        tab_a.stamp = tab_b.stamp + 1000
        check(c.pools(rec, lens, own, tab_a, have, base, poison=POISON), eb, "A rewritten")
    finally:
        c.close()


# ---- with real records: classify -> pool plan -> enqueue plan on one stream --
def test_pools_follow_classify_and_the_enqueue_plan_follows_them(built, gpu):
    """The zoo's program with CoS pools on a few thousand frames: mi_cls_classify,
    the pool plan and the enqueue plan over res_out on one stream, nothing
    synchronised between them; the deliveries, the freed packets and the counters
    are reference_loop()'s on the oracle's records.  Then the pktio forms, and
    -ENOTSUP on a pktio over several devices."""
    import torch
    frames = [f for _, f in zoo.all_frames()]
    frames = (frames * (3000 // len(frames) + 1))[:3000]
    b = pg.batch_from_frames(frames)
    prog = zoo.prog_everything()
    exp_rec, _ = oracle_run(prog, b)
    c = cls.Classifier(gpu=0)
    try:
        c.apply(prog)
        # pool handles 1 .. 3 on two CoS in three; the pktio's own pool is 9
        for i, h in enumerate(c.cos):
            if i % 3:
                assert c.L.odp_cls_cos_pool_set(h, i % 3 + (i % 2) * 2) == 0
        caps = {9: 1536, 1: 70, 2: 9000, 3: 128, 4: 64}
        ptab, pools, _ = c.pool_table(caps, pktio_pool=9)
        ptable = PM.ptable_of(ptab)
        assert pools[0] == 9 and ptable[2] == len(pools) == 5
        tab = c.enq_table()[0]
        table = M.table_of(tab)
        need = need_of(exp_rec, b.len, None, ptable)
        have = (need * 2 // 3).tolist()
        base = (np.cumsum(need) - need).tolist()
        dev = torch.device("cuda:0")
        n, ng = b.n, table[3] + 2
        side = torch.cuda.Stream(dev)
        t_buf = torch.from_numpy(np.ascontiguousarray(b.buf)).to(dev)
        t_off = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        t_rec = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
        t_dec = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t_idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t_pout = torch.full((40,), -1, dtype=torch.int32, device=dev)
        t_perm = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t_gbeg = torch.full((ng,), -1, dtype=torch.int32, device=dev)
        t_eout = torch.full((6,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        u = C.c_uint32 * cls.POOL_SLOTS
        with torch.cuda.stream(side):
            s = side.cuda_stream
            assert c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_rec.data_ptr(), s) == 0
            assert c.L.odp_amd_cls_pool_plan(c.pktio, t_rec.data_ptr(), t_len.data_ptr(), None, n, C.byref(ptab),
                                             u(*have), u(*base), t_rec.data_ptr(), t_dec.data_ptr(),
                                             t_idx.data_ptr(), t_pout.data_ptr(), s) == 0
            assert c.L.odp_amd_cls_enq_plan(c.pktio, t_rec.data_ptr(), t_len.data_ptr(), n, C.byref(tab),
                                            t_perm.data_ptr(), t_gbeg.data_ptr(), t_eout.data_ptr(), s) == 0
        side.synchronize()
        exp = PM.plan_pools(exp_rec, b.len, None, ptable, have, base)
        got = (t_rec.cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE), t_dec.cpu().numpy().view(np.uint32),
               t_idx.cpu().numpy().view(np.uint32), cls.pool_out_dict(t_pout.cpu().numpy().view(np.uint32)))
        check(got, exp, "after classify")
        assert exp[3]["fresh"] > 500 and exp[3]["shorted"] > 100 and exp[3]["too_long"] > 10
        queues, freed, ctr = PM.reference_loop(exp_rec, b.len, None, ptable, have, table)
        perm, gbeg = t_perm.cpu().numpy().view(np.uint32), t_gbeg.cpu().numpy().view(np.uint32)
        ndst = table[3]
        for g in range(ndst):
            assert perm[gbeg[g]:gbeg[g + 1]].tolist() == queues[g], g
        assert perm[gbeg[ndst]:].tolist() == freed
        eout = dict(zip(M.FIELDS, (int(v) for v in t_eout.cpu().numpy().view(np.uint64))))
        assert {k: eout[k] for k in ctr} == ctr and eout["stale"] == 0
        # the pktio's forms: the binding on the device, the host form staged
        own = PM.make_own(np.random.default_rng(1), exp_rec, ptable)
        expo = PM.plan_pools(exp_rec, b.len, own, ptable, have, base)
        check(c.pool_plan(exp_rec, b.len, own, have, base, ptab, poison=POISON), expo, "pktio, device")
        for submit in (False, True):
            a, _ = _host_arrays(n, ())
            a["res"][:], a["len"][:], a["own"][:] = exp_rec, b.len, own
            c.pool_plan_host(a["res"], a["len"], a["own"], have, base, a["res_out"][:n], a["dec"][:n], a["idx"][:n],
                             a["out"], ptab, submit=submit)
            check(_host_result(a, n), expo, f"pktio, host, submit {submit}")
    finally:
        c.close()
    m = cls.Classifier(gpus=[0, 0])
    try:
        m.apply(prog)
        out = np.zeros(40, np.uint32)
        w = np.zeros(0, np.uint32)
        r0, l0 = np.zeros(0, R.RESULT_DTYPE), np.zeros(0, np.uint16)
        args = (m.pktio, None, None, None, 0, C.byref(ptab), u(*Z), u(*Z), None, None, None, out.ctypes.data)
        t = C.c_uint64(7)
        assert m.L.odp_amd_cls_pool_plan(*args, None) == -errno.ENOTSUP
        assert m.L.odp_amd_cls_pool_plan_host(*args) == -errno.ENOTSUP
        assert m.L.odp_amd_cls_pool_plan_host_submit(*args, C.byref(t)) == -errno.ENOTSUP and t.value == 0
        with pytest.raises(RuntimeError, match=f"{-errno.ENOTSUP}"):
            m.pool_plan_host(r0, l0, None, Z, Z, r0, w, w, out, ptab)
        assert not out.any()
    finally:
        m.close()


# ---- errors -------------------------------------------------------------------------------
def test_errors(ctx):
    """NULL arrays with n > 0 (own may be NULL), a NULL out or table, a
    misaligned out, res or res_out, too many slots, a batch past the bound,
    packets that would reach index 0xFFFFFFFF: -EINVAL; nothing is launched."""
    import torch
    rec, lens, own, ptable, have, base = _case(3, 10)
    tab = cls.pool_tab(*ptable)
    d = torch.zeros(8192, dtype=torch.int32, device="cuda:0")
    p = d.data_ptr()
    # res, len, own, n, tab, have, base, res_out, dec, idx, out
    good = [p, p + 1024, p + 2048, 10, tab, have, base, p + 4096, p + 8192, p + 12288, p + 16384]
    assert ctx.pools_device(*good) == 0
    torch.cuda.synchronize()
    for k in (0, 1, 7, 8, 9, 10):
        bad = list(good)
        bad[k] = 0
        assert ctx.pools_device(*bad) == -errno.EINVAL, k
    for k, v in ((0, p + 8), (7, p + 4096 + 4), (10, p + 16388), (3, 1 << 28),
                 (4, cls.pool_tab(ptable[0], ptable[1], nslot=17)),
                 (6, [0xFFFFFFFF - 4] + [0] * 15), (5, [UNL] * 16)):
        bad = list(good)
        bad[k] = v
        if k == 5:
            bad[6] = [0xFFFFFFFF - 9] + [0] * 15   # base + min(have, n) = 0xFFFFFFFF
        if k == 6:
            bad[5] = [5] + [0] * 15
        assert ctx.pools_device(*bad) == -errno.EINVAL, k
    ok = list(good)
    ok[2] = 0                                                  # own may be NULL
    ok[5], ok[6] = [UNL] * 16, [0xFFFFFFFF - 11] + [0] * 15    # the last index is 0xFFFFFFFE
    assert ctx.pools_device(*ok) == 0
    assert ctx.pools_device(0, 0, 0, 0, tab, have, base, 0, 0, 0, p + 16384) == 0   # n == 0 needs no arrays
    torch.cuda.synchronize()
    L = ctx.L
    ro, dec, idx, out = np.zeros(10, R.RESULT_DTYPE), np.zeros(10, np.uint32), np.zeros(10, np.uint32), \
        np.zeros(40, np.uint32)
    t = C.c_uint64(5)
    u = C.c_uint32 * cls.POOL_SLOTS
    host = [ctx.ctx, rec.ctypes.data, lens.ctypes.data, own.ctypes.data, 10, C.byref(tab), u(*have), u(*base),
            ro.ctypes.data, dec.ctypes.data, idx.ctypes.data, out.ctypes.data]
    for k in (1, 2, 5, 6, 7, 8, 9, 10, 11, 0):   # the last: a device, no context
        bad = list(host)
        bad[k] = None
        assert L.mi_cls_pool_plan_host(*bad) == -errno.EINVAL, k
        t.value = 5
        assert L.mi_cls_pool_plan_host_submit(*bad, C.byref(t)) == -errno.EINVAL and t.value == 0
    assert L.mi_cls_pool_plan_host_submit(*host, None) == -errno.EINVAL
    assert not dec.any() and not out.any()
