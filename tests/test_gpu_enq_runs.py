"""The run plan on the GPU (mi_cls_enq_runs / odp_amd_cls_enq_runs and their
host forms) against the CPU model (tests/run_model.py): seq[0:n], the runs
that fit run_cap and every word of out compared for equality.  Every output
word holds poison before each call, with a guard past each array; the runs past
min(nruns, run_cap) must still hold it afterwards.

The model is the per-record loop (run_model.plan_runs) for batches up to
LOOP_MAX records and its numpy statement (plan_runs_np, held equal to the loop
by tests/test_enq_runs_cpu.py) above.  The shapes follow the kernels' exported
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
from tests import run_model as RM
from tests.helpers import oracle_run

pytestmark = pytest.mark.gpu

T, G = cls.RUN_TILE, cls.RUN_GRID
LOOP_MAX = 4 * T
POISON = 0xA5A5A5A5
BIG = 600_011          # three tiles per block, the last block's run cut short
RUN_POISON = np.full(4, POISON, np.uint32).view(cls.RUN_DTYPE)[0]


@pytest.fixture(scope="module")
def ctx(built, gpu):
    c = cls.EnqContext(0)
    yield c
    c.close()


def model(rec, lens, table, rtable, burst=0):
    return (RM.plan_runs if rec.shape[0] <= LOOP_MAX else RM.plan_runs_np)(rec, lens, table, rtable, burst)


def check(got, exp, what):
    """got: (seq, runs[run_cap], out) of a call whose outputs were poisoned."""
    seq, runs, out = got
    eseq, eruns, eout = exp
    assert out == eout, f"{what}: out {out} != {eout}"
    if not np.array_equal(seq, eseq):
        j = int(np.nonzero(seq != eseq)[0][0])
        raise AssertionError(f"{what}: seq[{j}] = {seq[j]:#x}, model {eseq[j]} (n {seq.shape[0]})")
    k = min(eruns.shape[0], runs.shape[0])
    if not np.array_equal(runs[:k], eruns[:k]):
        r = int(np.nonzero(runs[:k] != eruns[:k])[0][0])
        raise AssertionError(f"{what}: runs[{r}] = {runs[r]}, model {eruns[r]} ({eruns.shape[0]} runs)")
    assert np.all(runs[k:] == RUN_POISON), f"{what}: a run past min(nruns, run_cap) = {k} was written"


def run(ctx, rec, lens, table, rtable, burst=0, run_cap=None, what=""):
    got = ctx.runs(rec, lens, cls.enq_tab(*table), cls.run_tab(*rtable), burst, run_cap, poison=POISON)
    check(got, model(rec, lens, table, rtable, burst), what)
    return got


def stretches(rng, n, ndst, longest=12, drop_one_in=5):
    """dst[n]: stretches of 1 .. longest records to one destination, one record
    in drop_one_in not delivered (0: none)."""
    ln = rng.integers(1, longest + 1, 4 * n // (longest + 1) + 2)
    ln = np.concatenate([ln, [max(0, n - int(ln.sum()))]])
    dst = np.repeat(rng.integers(0, ndst, ln.shape[0]), ln)[:n]
    if drop_one_in:
        dst = np.where(rng.integers(0, drop_one_in, n) == 0, M.drops(n), dst)
    return dst


def undelivered(rec, table, at):
    """Make the records `at` not delivered, every such outcome in turn and
    stale records (a CoS without queues, a slot past its CoS's) among them."""
    assert table[0][255] == 0 and 0 < table[0][0] <= 60
    at = np.asarray(at)
    nd = len(M.NOT_DELIVERED)
    k = np.arange(at.shape[0]) % (nd + 2)
    rec["outcome"][at] = np.array(M.NOT_DELIVERED + (M.OUT_ENQ, M.OUT_ENQ), np.uint8)[k]
    rec["cos"][at[k == nd]], rec["queue"][at[k == nd]] = 255, 0
    rec["cos"][at[k == nd + 1]], rec["queue"][at[k == nd + 1]] = 0, 60


# ---- batch sizes --------------------------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, G * T + 1, BIG)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n):
    """Random stretches to 300 destinations over CoS of every mode, a fifth of
    the records dropped, in one burst and in bursts of 100."""
    rng = np.random.default_rng(n + 1)
    table, entry_of = M.make_table(rng, 300)
    rtable = RM.make_rtable(rng)
    rec, lens = M.make_records(rng, n, stretches(rng, n, 300), entry_of, R.RESULT_DTYPE)
    for burst in (0, 100):
        got = run(ctx, rec, lens, table, rtable, burst, what=f"n {n} burst {burst}")
        info = ctx.last_launch()
        assert (info[0], info[1], info[6]) == (192 + T // 64, 5 if n else 1, min(G, (n + T - 1) // T)), info
    if n >= T - 1:
        out = got[2]
        assert out["nruns"] > n // 100 and out["vectors"] and out["in_errors"] and out["in_discards"]
        assert out["delivered"] > out["packets"] and sum(out["vec_need"]) == out["vectors"]


# ---- the previous delivered record far away -----------------------------------
@pytest.mark.parametrize("same_key", [True, False], ids=["same_key", "other_key"])
def test_previous_delivered_record_far_away(ctx, same_key):
    """2 G T records, two tiles per block, nearly all of them not delivered.
    Pairs of delivered records with only undelivered ones between them: in one
    wave, in the next wave, across a tile edge, across a whole undelivered
    tile, across a block edge, across a whole block's run of tiles, and across
    many blocks.  With the same key a pair is one run, with another key two."""
    n = 2 * G * T
    B = 2 * T   # records per block
    pairs = [(3, 40), (70, 130), (T - 2, T + 1), (5 * B + 9, 5 * B + 2 * T - 4), (9 * B - 1, 9 * B),
             (12 * B + T - 1, 14 * B + 5), (20 * B + 63, 90 * B + 64), (n - B - 1, n - 1)]
    pairs[3] = (4 * B + T - 3, 5 * B + T + 2)   # tile 1 of block 4 .. tile 1 of block 5: a whole tile between
    rng = np.random.default_rng(11)
    table, entry_of = M.make_table(rng, 8)
    dst = np.zeros(n, np.int64)
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    keep = np.zeros(n, bool)
    for k, (a, b) in enumerate(pairs):
        keep[[a, b]] = True
        da, db = k % 8, (k if same_key else k + 4) % 8
        for i, d in ((a, da), (b, db)):
            rec[i]["cos"], rec[i]["queue"] = entry_of[d] // M.NQ, entry_of[d] % M.NQ
    undelivered(rec, table, np.nonzero(~keep)[0])
    rtable = RM.uniform_rtable(RM.VEC, 2)
    for burst in (0, 4096):
        got = run(ctx, rec, lens, table, rtable, burst, what=f"far burst {burst}")
        out = got[2]
        assert out["delivered"] == 2 * len(pairs) and out["stale"] > n // 8
        if burst == 0:
            # neighbouring pairs have different keys either way
            assert out["nruns"] == (len(pairs) if same_key else 2 * len(pairs))
            assert out["vectors"] == (len(pairs) if same_key else 0)


def test_only_the_last_record_delivered(ctx):
    """Every block but the last delivers nothing: the carry is `none` all the
    way, and the one delivered record is a head."""
    n = G * T + 1
    rng = np.random.default_rng(12)
    table, entry_of = M.make_table(rng, 3)
    rec, lens = M.make_records(rng, n, np.zeros(n, np.int64), entry_of, R.RESULT_DTYPE)
    undelivered(rec, table, np.arange(n - 1))
    got = run(ctx, rec, lens, table, RM.uniform_rtable(RM.VEC, 4), what="last only")
    assert got[2]["nruns"] == 1 and got[1][0]["count"] == 1 and got[0][0] == n - 1


# ---- one key over the whole batch ----------------------------------------------
def test_one_key_over_the_whole_batch(ctx):
    """More than 65535 records to one (id, cos): one run whose count does not
    fit 16 bits, under vector sizes 1, 2, 256 and 65535 and every mode."""
    n = 70_001
    rng = np.random.default_rng(13)
    table, entry_of = M.make_table(rng, 5)
    rec, lens = M.make_records(rng, n, np.full(n, 2), entry_of, R.RESULT_DTYPE)
    undelivered(rec, table, np.arange(10, n, 997))
    for vmax in (1, 2, 256, 65535):
        for mode in (0, RM.AGGR, RM.VEC, RM.VEC | RM.AGGR):
            got = run(ctx, rec, lens, table, RM.uniform_rtable(mode, vmax, 7), what=f"one key vmax {vmax} mode {mode}")
            seq, runs, out = got
            cnt = out["delivered"]
            assert out["nruns"] == 1 and runs[0]["count"] == cnt > 65535
            nvec = -(-cnt // vmax) if mode & RM.VEC else 0
            assert runs[0]["nvec"] == nvec == out["vectors"] == out["vec_need"][7]
            assert runs[0]["flags"] == (RM.VEC if mode & RM.VEC else mode & RM.AGGR)


# ---- alternating keys, run_cap ---------------------------------------------------
def test_alternating_keys_and_run_cap(ctx):
    """Every delivered record is a run of its own; run_cap exact, one short,
    and none: out.nruns is the true count and nothing past the runs that fit
    is touched."""
    n = 3 * T + 5
    rng = np.random.default_rng(14)
    table, entry_of = M.make_table(rng, 2)
    rec, lens = M.make_records(rng, n, np.arange(n) % 2, entry_of, R.RESULT_DTYPE)
    gone = np.concatenate([np.arange(4, n, 6), np.arange(5, n, 6)])   # two at a time: the neighbours still differ
    undelivered(rec, table, gone)
    rtable = RM.uniform_rtable(RM.VEC | RM.AGGR, 4)
    nruns = model(rec, lens, table, rtable)[2]["nruns"]
    assert nruns == n - gone.shape[0]
    for cap in (nruns, nruns - 1, 0, nruns + 3):
        got = run(ctx, rec, lens, table, rtable, run_cap=cap, what=f"run_cap {cap}")
        assert got[2]["nruns"] == got[2]["delivered"] == nruns and got[2]["vectors"] == 0
        assert np.all(got[1][:min(cap, nruns)]["flags"] == RM.AGGR)


# ---- key breaks -------------------------------------------------------------------
def test_key_breaks(ctx):
    """CoS 0 has two entries of id 0 and one of id 1, CoS 1 one entry of id 0:
    the same id under another CoS breaks a run, the same CoS with another id
    breaks it, two entries that share an id do not."""
    table = (np.array([3, 1] + [0] * 254, np.uint8), np.array([0, 3] + [0] * 254, np.uint16),
             np.array([0, 0, 1, 0] + [0xFFFF] * (M.ENT - 4), np.uint16), 2)
    rtable = RM.uniform_rtable(RM.VEC, 3, 1)
    hand = [(0, 0), (0, 1), (0, 0), (1, 0), (1, 0), (0, 2), (0, 2), (0, 1), (0, 0)]
    rec = np.zeros(len(hand), R.RESULT_DTYPE)
    rec["cos"], rec["queue"] = [h[0] for h in hand], [h[1] for h in hand]
    lens = np.full(len(hand), 64, np.uint16)
    got = run(ctx, rec, lens, table, rtable, what="key breaks by hand")
    assert [(r["count"], r["dst"], r["cos"]) for r in got[1][:4]] == [(3, 0, 0), (2, 0, 1), (2, 1, 0), (2, 0, 0)]
    assert got[2]["nruns"] == 4
    # the same four (cos, slot) pairs at random over three tiles
    rng = np.random.default_rng(15)
    n = 3 * T + 1
    pick = np.repeat(rng.integers(0, 4, n), rng.integers(1, 4, n))[:n]
    rec = np.zeros(n, R.RESULT_DTYPE)
    rec["cos"] = np.array([0, 0, 0, 1], np.uint8)[pick]
    rec["queue"] = np.array([0, 1, 2, 0], np.uint16)[pick]
    lens = rng.integers(0, 65536, n).astype(np.uint16)
    got = run(ctx, rec, lens, table, rtable, what="key breaks")
    key = np.array([0, 0, 1, 2])[pick]   # the three (id, cos) among the four pairs
    assert got[2]["nruns"] == 1 + np.count_nonzero(np.diff(key))


# ---- bursts -------------------------------------------------------------------------
@pytest.mark.parametrize("burst", [1, 7, 1000, 4096])
@pytest.mark.parametrize("n", [2 * 4096 + 100, BIG], ids=["one_tile_per_block", "three_tiles_per_block"])
def test_bursts(ctx, n, burst):
    """A burst's end ends a run: one key over the whole batch, so only bursts
    (and nothing else) cut it; then long random stretches.  burst 1: every
    delivered record is a head; 7 and 1000 cut inside a wave; 4096 at a tile
    edge, which is a block's edge in the small batch and lies inside a block's
    run in the large one.  The first record of many bursts is not delivered."""
    rng = np.random.default_rng(n + burst)
    table, entry_of = M.make_table(rng, 6)
    rtable = RM.uniform_rtable(RM.VEC, 5, 3)
    first = np.arange(0, n, burst)[::3]
    for what, dst in (("one key", np.full(n, 4)), ("stretches", stretches(rng, n, 6, longest=3000, drop_one_in=9))):
        rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
        if burst > 1:
            undelivered(rec, table, first)
        got = run(ctx, rec, lens, table, rtable, burst, what=f"{what} n {n} burst {burst}")
        out = got[2]
        if burst == 1:
            assert out["nruns"] == out["delivered"] and out["vectors"] == 0
        elif what == "one key":
            assert out["nruns"] == (n + burst - 1) // burst


# ---- vec_need -------------------------------------------------------------------------
@pytest.mark.parametrize("nslots", [1, 2, 16])
def test_vec_need(ctx, nslots):
    """The vectors each pool must supply, over 1, 2 and 16 slots."""
    n = 5 * T + 3
    rng = np.random.default_rng(20 + nslots)
    table, entry_of = M.make_table(rng, 600)   # 24 CoS
    mode, vmax, _ = RM.make_rtable(rng, vmaxes=(1, 2, 3))
    mode |= RM.VEC
    vslot = (np.arange(256) % nslots).astype(np.uint8)
    rec, lens = M.make_records(rng, n, stretches(rng, n, 600), entry_of, R.RESULT_DTYPE)
    got = run(ctx, rec, lens, table, (mode, vmax, vslot), what=f"{nslots} slots")
    need = got[2]["vec_need"]
    assert all(need[:nslots]) and not any(need[nslots:]) and sum(need) == got[2]["vectors"] > 0


# ---- forms ------------------------------------------------------------------------------
def _case(seed, n, ndst=300):
    rng = np.random.default_rng(seed)
    table, entry_of = M.make_table(rng, ndst)
    rec, lens = M.make_records(rng, n, stretches(rng, n, ndst), entry_of, R.RESULT_DTYPE)
    return table, RM.make_rtable(rng), rec, lens


def _host_arrays(n, cap, pinned):
    """res, lens, seq (+ guard), runs (+ guard), out (+ guard), poisoned; and
    what to close."""
    counts = (n, n, n + 1, cap + 1, 25)
    dts = (R.RESULT_DTYPE, np.uint16, np.uint32, cls.RUN_DTYPE, np.uint64)
    if pinned:
        mem = [cls.PinnedArray((k * np.dtype(dt).itemsize + 15) // 16 * 16 + 16) for k, dt in zip(counts, dts)]
        arrs = [m.view(dt)[:k] for m, k, dt in zip(mem, counts, dts)]
    else:
        mem = []
        arrs = [np.zeros(k, dt) for k, dt in zip(counts, dts)]
    for a in arrs[2:]:
        a.view(np.uint32)[:] = POISON
    return arrs, mem


def _host_result(arrs, n, cap):
    res, ln, seq, runs, out = arrs
    assert seq[n] == POISON and runs[cap] == RUN_POISON and out[24] == (POISON << 32 | POISON)
    return seq[:n].copy(), runs[:cap].copy(), cls.run_out_dict(out[:24])


@pytest.mark.parametrize("submit", [False, True], ids=["wait", "submit"])
@pytest.mark.parametrize("pinned", [True, False], ids=["in_place", "staged"])
@pytest.mark.parametrize("n,cap", [(0, 4), (1, 1), (T + 1, 2 * T), (5 * T + 3, 700)])
def test_host_forms(ctx, n, cap, pinned, submit):
    """The host form in place (page-locked arrays) and staged (pageable), as
    one call and as submit / wait, with room for every run and truncated;
    nothing is written past an array or past the runs that fit."""
    table, rtable, rec, lens = _case(31 * n + cap, n)
    arrs, mem = _host_arrays(n, cap, pinned)
    try:
        arrs[0][:] = rec
        arrs[1][:] = lens
        ctx.runs_host(arrs[0], arrs[1], cls.enq_tab(*table), cls.run_tab(*rtable), 64, arrs[2][:n], arrs[3][:cap],
                      arrs[4], submit=submit)
        check(_host_result(arrs, n, cap), model(rec, lens, table, rtable, 64), f"host n {n} cap {cap}")
        assert np.array_equal(arrs[0], rec) and np.array_equal(arrs[1], lens)   # the inputs are only read
    finally:
        for m in mem:
            m.close()


def test_submit_several_then_wait(ctx):
    """Tickets of the context's ring: more batches submitted than the ring
    holds, each with buffers of its own, waited for in order afterwards."""
    L = ctx.L
    cases = [_case(50 + k, 300 + 700 * k) for k in range(10)]
    tabs = [(cls.enq_tab(*c[0]), cls.run_tab(*c[1])) for c in cases]
    bufs, tickets = [], []
    for k, ((table, rtable, rec, lens), (tab, rtab)) in enumerate(zip(cases, tabs)):
        n = rec.shape[0]
        arrs, _ = _host_arrays(n, n, pinned=False)
        arrs[0][:], arrs[1][:] = rec, lens
        t = C.c_uint64()
        rc = L.mi_cls_enq_runs_host_submit(ctx.ctx, arrs[0].ctypes.data, arrs[1].ctypes.data, n, C.byref(tab),
                                           C.byref(rtab), 10 * k, arrs[2].ctypes.data, arrs[3].ctypes.data, n,
                                           arrs[4].ctypes.data, C.byref(t))
        assert rc == 0 and t.value > (tickets[-1] if tickets else 0)
        bufs.append(arrs)
        tickets.append(t.value)
    for k, ((table, rtable, rec, lens), arrs, t) in enumerate(zip(cases, bufs, tickets)):
        assert L.mi_cls_enq_runs_host_wait(ctx.ctx, t) == 0
        n = rec.shape[0]
        check(_host_result(arrs, n, n), RM.plan_runs(rec, lens, table, rtable, 10 * k), f"ticket {t}")
    assert L.mi_cls_enq_runs_host_wait(ctx.ctx, tickets[-1] + 1) == -errno.EINVAL


def test_large_then_small_and_tables_again(built, gpu):
    """On a fresh context: a small call after a large one sees nothing of the
    first one's scratch or counters, then a larger one again (the scratch
    grows); the device keeps the last tables' copies: A, B, A again, then A
    rewritten in place under a new stamp."""
    c = cls.EnqContext(0)
    try:
        for k, n in enumerate([40 * T + 9, 70, 3, 0, 90 * T, T]):
            table, rtable, rec, lens = _case(70 + k, n)
            run(c, rec, lens, table, rtable, burst=(0, 50)[k % 2], what=f"call {k}")
        table, ra, rec, lens = _case(80, 2 * T)
        rb = RM.make_rtable(np.random.default_rng(81))
        tab, tab_a, tab_b = cls.enq_tab(*table), cls.run_tab(*ra), cls.run_tab(*rb)
        ea, eb = RM.plan_runs(rec, lens, table, ra), RM.plan_runs(rec, lens, table, rb)
        assert ea[2]["vec_need"] != eb[2]["vec_need"]
        for what, rt, exp in (("A", tab_a, ea), ("B", tab_b, eb), ("A again", tab_a, ea), ("A once more", tab_a, ea)):
            check(c.runs(rec, lens, tab, rt, poison=POISON), exp, what)
        for name, src in zip(("mode", "vmax", "vslot"), rb):
            np.ctypeslib.as_array(getattr(tab_a, name))[:] = src
        tab_a.stamp = tab_b.stamp + 1000
        check(c.runs(rec, lens, tab, tab_a, poison=POISON), eb, "A rewritten")
    finally:
        c.close()


def test_runs_follow_classify_on_its_stream(built, gpu):
    """odp_amd_cls_enq_runs on the classification's stream right after
    classify_device, no synchronisation between the two: the records never
    leave the device.  A hash CoS of 4 queues, two CoS on one queue, a drop CoS;
    the model over the oracle's records."""
    import torch
    frames = [pg.udp4_frame(size=60 + (i % 40), sport=1000 + (i // 5), dport=(53, 80, 443, 9)[(i // 3) % 4])
              for i in range(3000)]
    b = pg.batch_from_frames(frames)
    prog = [R.cos("default", queue=0x1100), R.cos("hash", num_queue=4, hash_proto=R.HP_IPV4_UDP),
            R.cos("shared", queue=0x1100), R.cos("drop", action=1, queue=0x3300), ("default", 0),
            ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 53)], 0, 1, 0), ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 80)], 0, 2, 3),
            ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 443)], 0, 3, 0)]
    exp_rec, _ = oracle_run(prog, b)
    c = cls.Classifier(gpu=0)
    try:
        c.apply(prog)
        tab = c.enq_table()[0]
        rtab0, vpools, _ = c.run_table()
        assert vpools == []
        rtable = (np.array([RM.VEC, RM.AGGR, RM.VEC, 0], np.uint8), np.array([4, 0, 2, 0], np.uint16),
                  np.array([0, 0, 1, 0], np.uint8))
        rtab = cls.run_tab(*rtable)
        dev = torch.device("cuda:0")
        n = b.n
        side = torch.cuda.Stream(dev)
        t_buf = torch.from_numpy(np.ascontiguousarray(b.buf)).to(dev)
        t_off = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        t_rec = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
        t_seq = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t_runs = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
        t_out = torch.full((24,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_rec.data_ptr(),
                                   side.cuda_stream)
            assert rc == 0
            rc = c.L.odp_amd_cls_enq_runs(c.pktio, t_rec.data_ptr(), t_len.data_ptr(), n, C.byref(tab),
                                          C.byref(rtab), 32, t_seq.data_ptr(), t_runs.data_ptr(), n,
                                          t_out.data_ptr(), side.cuda_stream)
            assert rc == 0
        side.synchronize()
        got_rec = t_rec.cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE)
        assert np.array_equal(got_rec, exp_rec)
        runs = t_runs.cpu().numpy().view(np.uint32).reshape(-1).view(cls.RUN_DTYPE)
        exp = RM.plan_runs(exp_rec, b.len, M.table_of(tab), rtable, 32)
        nruns = exp[2]["nruns"]
        assert 100 < nruns < n and np.all(runs[nruns:].view(np.uint32) == 0xFFFFFFFF)
        got = (t_seq.cpu().numpy().view(np.uint32), runs[:nruns],
               cls.run_out_dict(t_out.cpu().numpy().view(np.uint64)))
        check(got, exp, "after classify")
        assert exp[2]["vec_need"][0] and exp[2]["vec_need"][1] and exp[2]["stale"] == 0
        # the binding's form, tables built from the control plane: no vectors
        got = c.enq_runs(exp_rec, b.len, burst=32, poison=POISON)
        check(got, RM.plan_runs(exp_rec, b.len, M.table_of(tab), RM.rtable_of(rtab0), 32), "binding")
        assert got[2]["vectors"] == 0 and got[2]["nruns"] == nruns
    finally:
        c.close()


# ---- errors -------------------------------------------------------------------------------
def test_errors(ctx):
    """NULL arrays with n > 0, a NULL out or table, a misaligned out or runs:
    -EINVAL; ndst past the bound: -E2BIG; a vector CoS without a size or with a
    slot past the bound: -EINVAL; nothing is launched."""
    import torch
    table, rtable, rec, lens = _case(3, 10, 4)
    tab, rtab = cls.enq_tab(*table), cls.run_tab(*rtable)
    d = torch.zeros(8192, dtype=torch.int32, device="cuda:0")
    p = d.data_ptr()
    # res, len, n, tab, rtab, burst, seq, runs, run_cap, out
    good = [p, p + 1024, 10, tab, rtab, 0, p + 2048, p + 4096, 10, p + 8192]
    assert ctx.runs_device(*good) == 0
    torch.cuda.synchronize()
    for k in (0, 1, 6, 7, 9):
        bad = list(good)
        bad[k] = 0
        assert ctx.runs_device(*bad) == -errno.EINVAL, k
    bad = list(good)
    bad[7], bad[8] = 0, 0
    assert ctx.runs_device(*bad) == 0                    # no room asked for: runs may be NULL
    bad[9] = p + 8196
    assert ctx.runs_device(*bad) == -errno.EINVAL        # out not 8-byte aligned
    bad = list(good)
    bad[7] = p + 4096 + 8
    assert ctx.runs_device(*bad) == -errno.EINVAL        # runs not 16-byte aligned
    assert ctx.runs_device(0, 0, 0, tab, rtab, 0, 0, 0, 0, p + 8192) == 0   # n == 0 needs no arrays
    torch.cuda.synchronize()
    big = cls.enq_tab(*table[:3], cls.ENQ_DST_MAX + 1)
    novmax = cls.run_tab([cls.RUN_VEC], [0], [0])
    badslot = cls.run_tab([0, cls.RUN_VEC | cls.RUN_AGGR], [1, 1], [0, cls.RUN_VSLOTS])
    for k, v, rc in ((3, big, -errno.E2BIG), (4, novmax, -errno.EINVAL), (4, badslot, -errno.EINVAL)):
        bad = list(good)
        bad[k] = v
        assert ctx.runs_device(*bad) == rc
    L = ctx.L
    seq, runs, out = np.zeros(10, np.uint32), np.zeros(10, cls.RUN_DTYPE), np.zeros(24, np.uint64)
    t = C.c_uint64(5)
    host = [ctx.ctx, rec.ctypes.data, lens.ctypes.data, 10, C.byref(tab), C.byref(rtab), 0, seq.ctypes.data,
            runs.ctypes.data, 10, out.ctypes.data]
    for k, v, rc in ((1, None, -errno.EINVAL), (7, None, -errno.EINVAL), (8, None, -errno.EINVAL),
                     (4, C.byref(big), -errno.E2BIG), (5, C.byref(novmax), -errno.EINVAL),
                     (0, None, -errno.EINVAL)):   # the last: a device, no context
        bad = list(host)
        bad[k] = v
        assert L.mi_cls_enq_runs_host(*bad) == rc, k
        t.value = 5
        assert L.mi_cls_enq_runs_host_submit(*bad, C.byref(t)) == rc and t.value == 0
    assert L.mi_cls_enq_runs_host_submit(*host, None) == -errno.EINVAL
    assert not seq.any() and not out.any()
