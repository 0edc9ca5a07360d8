"""The vector fill on the GPU (mi_cls_vec_fill, include/mi_cls.h) against
tests/vec_model.py.

Everything a run reads or writes lies in one rx_harness.Arena, filled with a
non-zero pattern first; afterwards the whole arena equals the image before the
call with the model's writes applied: ev[0 .. ev_span), evr[0 .. nruns), out,
the size word and the table of every vector written, and lost[0 .. out.lost)
as a set.  An unwritten slot, a write past ev_span or nruns, or a touched
refused vector shows as a compare failure.  The declared vector arena is one
region of it: addresses a guard must refuse point into the regions before and
behind.
"""
import ctypes as C
import errno

import numpy as np
import pytest

from odp_amd import cls
from odp_amd import rules as R
from tests import enq_model as M
from tests import run_model as RM
from tests import rx_harness as H
from tests import vec_model as VM

pytestmark = pytest.mark.gpu

TILE, GRID = cls.VEC_TILE, cls.VEC_GRID
BIG = GRID * TILE + 40            # the second tile of a block, cut short
SIZE_OFF, TBL_OFF = 12, 24        # a vector: [.. size ..][tbl]
E2H = 64                          # ent_to_handle
VEC, AGGR = RM.VEC, RM.AGGR


@pytest.fixture(scope="module")
def ctx(built, gpu):
    c = cls.EnqContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arena(built, gpu):
    a = H.Arena(96 << 20)
    yield a
    a.close()


def make_runs(rng, counts, rtable, cos=None):
    """Runs of the given lengths, one behind the other, under random CoS
    (neighbours differ) and destinations: flags and nvec by the run plan's rule."""
    mode, vmax, vslot = (np.asarray(x).astype(np.int64) for x in rtable)
    counts = np.asarray(counts, np.int64)
    nr = counts.shape[0]
    runs = np.zeros(nr, RM.RUN_DTYPE)
    if cos is None:
        cos = rng.integers(0, 256, nr)
        cos[1:] = np.where(cos[1:] == cos[:-1], (cos[1:] + 1) % 256, cos[1:])
    cos = np.broadcast_to(np.asarray(cos, np.int64), (nr,))
    vec = (counts >= 2) & ((mode[cos] & VEC) != 0)
    runs["first"] = np.cumsum(counts) - counts
    runs["count"], runs["cos"], runs["dst"] = counts, cos, rng.integers(0, 50, nr)
    runs["flags"] = np.where(vec, VEC, mode[cos] & AGGR)
    runs["nvec"] = np.where(vec, -(-counts // np.maximum(vmax[cos], 1)), 0)
    need = np.bincount(vslot[cos][vec], weights=runs["nvec"][vec], minlength=16).astype(np.int64)
    return runs, need


def random_counts(rng, d, hi=13):
    c = rng.integers(1, hi, d + 1)
    c = c[: int(np.searchsorted(np.cumsum(c), d, side="left")) + 1]
    c[-1] -= int(c.sum()) - d
    return c[c > 0] if d else c[:0]


class Case:
    """One run's memory, laid out in the arena."""

    def __init__(self, arena, seed, n, runs, need, rtable, *, vhave=None, holes=0.05, run_cap=None, spoil=False):
        rng = np.random.default_rng(seed)
        self.a, self.n, self.rtable, self.need = arena, n, rtable, np.asarray(need, np.int64)
        nr = self.nr = runs.shape[0]
        d = self.d = int(runs["count"].astype(np.int64).sum())
        assert d <= n
        self.run_cap = cap = nr + 3 if run_cap is None else run_cap
        vhave = need if vhave is None else np.asarray(vhave, np.int64)
        self.vhave = vhave
        self.vbase = np.cumsum(vhave) - vhave + 2          # two entries nobody may touch in front
        self.nvgot = nvgot = int(vhave.sum()) + 5
        vmax, vslot = np.asarray(rtable[1], np.int64), np.asarray(rtable[2], np.int64)
        vecmode = (np.asarray(rtable[0]) & VEC) != 0
        self.vcap = np.array([int(vmax[vecmode & (vslot == s)].max(initial=1)) for s in range(16)])
        arena.reset()
        m, mc = max(n, 1), max(cap, nr, 1)
        self.o = {}
        for name, dt, cnt in (("seq", "<u4", m), ("runs", RM.RUN_DTYPE, mc), ("rout", "<u8", 24), ("ent", "<u8", m),
                              ("vgot", "<u8", nvgot), ("ev", "<u8", m), ("evr", VM.EVRUN_DTYPE, mc),
                              ("lost", "<u8", m), ("out", "<u8", 24)):
            self.o[name], arr = arena.array(name, dt, cnt)
            setattr(self, name, arr)
        # the vectors: before, inside and behind the declared arena; slot s's hold vcap[s] entries
        vsize = TBL_OFF + 8 * self.vcap
        self.before = arena.alloc("before", 4 * (TBL_OFF + 64), 64)
        per = np.repeat(vsize, vhave)
        start = arena.alloc("vectors", int(per.sum()) + 8, 8, 8)
        at = start + np.cumsum(per) - per
        self.lo_off, self.hi_off = start, start + int(per.sum())
        arena.top = self.hi_off       # the last vector's table ends the declared arena
        self.behind = arena.alloc("behind", 4 * (TBL_OFF + 64), 64)
        arena.fill(seed)
        self.seq[:n] = rng.permutation(n)
        self.runs[:nr] = runs
        self.rout[4], self.rout[6] = d, nr
        self.ent[:n] = VM.make_ent(rng, n, base=0x7100_0000_0000, stride=0x40, holes=holes)
        self.vgot[:] = 0
        order = np.concatenate([self.vbase[s] + rng.permutation(int(vhave[s])) for s in range(16)]).astype(np.int64)
        self.vgot[order] = arena.ptr + at
        if spoil and len(at) >= 6:
            # 0, misaligned, before and behind the arena; all with room for a table
            k = rng.choice(order[:-1], 5, replace=False)
            self.vgot[k[0]] = 0
            self.vgot[k[1]] += 4
            self.vgot[k[2]] = arena.ptr + self.before
            self.vgot[k[3]] = arena.ptr + self.behind
            self.vgot[k[4]] = arena.ptr + self.hi_off - 8     # its table reaches past the end
        self.arena_bytes = self.hi_off - self.lo_off
        # the vector at the highest address: its index in vgot and its offset
        self.last_vi, self.last_at = (int(order[-1]), int(at[-1])) if len(at) else (None, None)

    def args(self, **over):
        b = self.a.ptr
        kw = dict(seq=b + self.o["seq"], runs=b + self.o["runs"], run_out=b + self.o["rout"], ent=b + self.o["ent"],
                  vgot=b + self.o["vgot"], n=self.n, run_cap=self.run_cap, nvgot=self.nvgot, size_off=SIZE_OFF,
                  tbl_off=TBL_OFF, ent_to_handle=E2H, varena_lo=b + self.lo_off, varena_bytes=self.arena_bytes,
                  ev=b + self.o["ev"], evr=b + self.o["evr"], lost=b + self.o["lost"], out=b + self.o["out"])
        kw.update(over)
        return cls.vec_args(cls.run_tab(*self.rtable), vbase=self.vbase, vhave=self.vhave, vcap=self.vcap, **kw)

    def model(self):
        ok = VM.arena_ok(self.a.ptr + self.lo_off, self.arena_bytes, TBL_OFF)
        return VM.fill_np(self.seq[: self.n], self.runs[: self.nr], self.ent[: self.n], self.rtable, self.vgot,
                          self.vbase, self.vhave, E2H, ok)

    def expect(self, res=None, truncated=False):
        """(image, care, result) after the fill, from the arena as it is now."""
        exp = self.a.snapshot()
        care = np.ones(len(exp), np.uint8)
        if truncated:
            out = VM.truncated()
            res = {"out": out, "lost": np.zeros(0, np.uint64)}
        else:
            res = res or self.model()
            out = res["out"]
            o = self.o
            exp[o["ev"]: o["ev"] + 8 * out["ev_span"]] = res["ev"].view(np.uint8)
            exp[o["evr"]: o["evr"] + 16 * self.nr] = res["evr"].view(np.uint8)
            care[o["lost"]: o["lost"] + 8 * out["lost"]] = 0
            v = self.vgot[res["vec_idx"]].astype(np.int64) - self.a.ptr
            sz = res["vec_size"]
            e32 = exp[: len(exp) & ~3].view(np.uint32)
            e32[(v + SIZE_OFF) // 4] = sz
            e64 = exp[: len(exp) & ~7].view(np.uint64)
            first = np.cumsum(sz) - sz
            where = np.repeat((v + TBL_OFF) // 8 - first, sz) + np.arange(int(sz.sum()))
            e64[where] = res["vec_tbl"]
        words = np.array([out[k] for k in VM.FIELDS[:8]] + out["vec_used"], np.uint64)
        exp[self.o["out"]: self.o["out"] + 192] = words.view(np.uint8)
        return exp, care, res

    def check(self, exp, care, res):
        H.compare(self.a, self.a.u8[: self.a.top], exp, care)
        got = np.sort(self.lost[: res["out"]["lost"]])
        assert np.array_equal(got, res["lost"]), "the lost packets differ"


def run(ctx, case, **over):
    exp, care, res = case.expect()
    ctx.fill(case.args(**over))
    case.check(exp, care, res)
    return res["out"]


def random_case(arena, seed, n, stock="exact", nslots=3, vmaxes=(1, 2, 3, 8), **kw):
    rng = np.random.default_rng(seed)
    rtable = RM.make_rtable(rng, nslots=nslots, vmaxes=vmaxes)
    d = n - n // 7                 # a seventh of the records is not delivered
    runs, need = make_runs(rng, random_counts(rng, d), rtable)
    vhave = {"exact": need, "none": need * 0, "half": need // 2,
             "mixed": np.array([(0, max(x - 1, 0), x, x + 5)[s % 4] for s, x in enumerate(need.tolist())])}[stock]
    return Case(arena, seed, n, runs, need, rtable, vhave=vhave, **kw)


# ---- record counts ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, BIG])
def test_sizes(ctx, arena, n):
    """Random plans of every mode over three slots, a stock that is exact, holes
    in ent, a seventh of the records not delivered; the launch's shape."""
    case = random_case(arena, 100 + n % 97, n)
    out = run(ctx, case)
    assert out["lost"] == 0 and out["truncated"] == 0
    info = ctx.last_launch()
    tiles = (n + TILE - 1) // TILE
    assert info == [384 + 16, 4 if n else 1, 0, 0, 0, 0, min(GRID, tiles)]
    if n >= 1023:
        assert out["vectors"] > 10 and out["holes"] > 0 and out["events"] < case.d


# ---- run shapes ------------------------------------------------------------------------
@pytest.mark.parametrize("vmax", [1, 3, 4096])
def test_one_run_of_the_whole_batch(ctx, arena, vmax):
    """One run spreads over the whole grid: as many vectors as packets (vmax
    1), vectors that straddle every tile (3), 4096."""
    rng = np.random.default_rng(vmax)
    rtable = RM.uniform_rtable(VEC, vmax, 7)
    runs, need = make_runs(rng, [BIG], rtable, cos=9)
    assert need[7] == -(-BIG // vmax)
    out = run(ctx, Case(arena, 200 + vmax, BIG, runs, need, rtable))
    assert (out["vectors"], out["in_vectors"], out["events"], out["ev_span"]) == (need[7], BIG, need[7], need[7])
    # the stock ends in the middle of the run
    have = need.copy()
    have[7] = need[7] // 2
    out = run(ctx, Case(arena, 210 + vmax, BIG, runs, need, rtable, vhave=have))
    assert out["vectors"] == have[7] and out["lost"] == BIG - have[7] * vmax and out["ev_span"] == need[7]


def test_every_run_of_one_packet(ctx, arena):
    """As many runs as packets: no vector at all, ev is the handles in seq order."""
    rng = np.random.default_rng(3)
    rtable = RM.make_rtable(rng)
    runs, need = make_runs(rng, np.ones(BIG - 100, np.int64), rtable)
    assert not need.any()
    out = run(ctx, Case(arena, 220, BIG, runs, need, rtable))
    assert out["events"] == out["ev_span"] == BIG - 100 and out["vectors"] == 0


@pytest.mark.parametrize("vmax", [3, 64])
def test_runs_around_the_vector_size(ctx, arena, vmax):
    """Runs of exactly vmax, vmax - 1, vmax + 1 and 2 * vmax packets, over two
    slots, with every stock: none, one short, exact, ample."""
    rng = np.random.default_rng(vmax)
    mode, vm, vslot = RM.uniform_rtable(VEC, vmax, 0)
    vslot[1::2] = 1
    counts = np.tile([vmax, vmax - 1, vmax + 1, 2 * vmax], 700)
    runs, need = make_runs(rng, counts, (mode, vm, vslot))
    n = int(counts.sum()) + 17
    for k, have in enumerate((need, need * 0, np.maximum(need - 1, 0), need + 5)):
        out = run(ctx, Case(arena, 230 + k, n, runs, need, (mode, vm, vslot), vhave=have))
        assert out["vectors"] == int(np.minimum(need, have).sum())


def test_heads_at_tile_and_block_ends(ctx, arena):
    """vmax 3: a run whose head is the last place of a tile, and one at the last
    place of a block's run of tiles, so that a run and a vector straddle both
    boundaries; the runs before them end exactly there."""
    rng = np.random.default_rng(5)
    rtable = RM.uniform_rtable(VEC, 3, 2)
    tpb = -(-(-(-BIG // TILE)) // GRID)      # tiles per block of the fill launch
    assert tpb == 2
    block = tpb * TILE
    counts = [TILE - 1, 7, block - 1 - (TILE + 6), 8, 2 * block - 1 - (block + 7), 2]
    assert sum(counts[:1]) == TILE - 1 and sum(counts[:3]) == block - 1 and sum(counts[:5]) == 2 * block - 1
    counts += random_counts(rng, BIG - 50 - sum(counts)).tolist()
    runs, need = make_runs(rng, counts, rtable)
    out = run(ctx, Case(arena, 240, BIG, runs, need, rtable))
    assert out["lost"] == 0 and out["vectors"] == need[2]


# ---- slots and stock -------------------------------------------------------------------
@pytest.mark.parametrize("stock", ["mixed", "half", "none"])
def test_sixteen_slots(ctx, arena, stock):
    """16 slots in use; per slot a stock of 0, need - 1, need and need + 5
    (mixed), half the need (it ends in the middle of a run), nothing.  Plain
    runs with the aggregator bit are among them."""
    case = random_case(arena, 300, 40 * TILE + 11, stock=stock, nslots=16, vmaxes=(2, 3, 5))
    assert (case.runs["flags"][: case.nr] == AGGR).any() and case.need.all()
    out = run(ctx, case)
    assert out["vec_used"] == np.minimum(case.need, case.vhave).tolist()
    assert (out["lost"] > 0) and (out["vectors"] > 0) == (stock != "none")


def test_holes(ctx, arena):
    """Half of ent is 0: handle 0 in ev, in the tables and in lost, counted."""
    case = random_case(arena, 310, 5 * TILE + 3, stock="half", holes=0.5)
    out = run(ctx, case)
    assert out["holes"] > TILE and out["lost"] > 0


# ---- guards ----------------------------------------------------------------------------
def test_refused_vectors(ctx, arena):
    """vgot entries that are 0, misaligned, in the regions before and behind the
    declared arena, and one whose table would reach past its end: left
    unwritten, ev entry 0, counted.  Then an arena that ends exactly where the
    table of its last vector ends (taken), and one byte before (refused)."""
    case = random_case(arena, 400, 6 * TILE + 9, spoil=True)
    out = run(ctx, case)
    assert out["refused"] == 5
    for short, refused in ((0, 0), (1, 1)):
        case = random_case(arena, 401, 6 * TILE + 9)
        res = case.model()
        size = int(res["vec_size"][res["vec_idx"].tolist().index(case.last_vi)])
        case.arena_bytes = case.last_at + TBL_OFF + 8 * size - case.lo_off - short
        out = run(ctx, case)
        assert out["refused"] == refused


def test_bad_plans_stay_inside(ctx, arena):
    """seq values past n, runs that reach past the delivered count and vector
    counts that do not fit the runs: whatever is written lies inside the
    arrays (the gaps and guard regions of the arena keep their pattern)."""
    case = random_case(arena, 410, 3 * TILE + 5)
    rng = np.random.default_rng(9)
    case.seq[rng.integers(0, case.n, 40)] = rng.integers(case.n, 2 ** 32, 40)
    case.runs["count"][rng.integers(0, case.nr, 20)] = rng.integers(1, 2 ** 32, 20)
    case.runs["nvec"][rng.integers(0, case.nr, 20)] = rng.integers(1, 2 ** 32, 20)
    case.runs["first"][rng.integers(0, case.nr, 20)] = rng.integers(0, 2 ** 32, 20)
    before = case.a.snapshot()
    ctx.fill(case.args())
    after = case.a.snapshot()
    mask = np.ones(len(before), bool)
    o = case.o
    for name, nb in (("ev", 8 * case.n), ("evr", 16 * case.run_cap), ("lost", 8 * case.n), ("out", 192)):
        mask[o[name]: o[name] + nb] = False
    mask[case.lo_off: case.hi_off] = False
    assert np.array_equal(before[mask], after[mask])


def test_truncated_plan(ctx, arena):
    """run_cap below nruns: nothing is written but out, truncated = 1."""
    case = random_case(arena, 420, 4 * TILE, run_cap=100)
    assert case.nr > 100
    exp, care, res = case.expect(truncated=True)
    ctx.fill(case.args())
    case.check(exp, care, res)
    # room for exactly nruns: not truncated, nothing past evr[nruns) touched
    case = random_case(arena, 420, 4 * TILE)
    case.run_cap = case.nr
    run(ctx, case)


def test_errors(ctx, arena):
    case = random_case(arena, 430, 300)
    before = case.a.snapshot()
    b = case.a.ptr
    for over in (dict(seq=0), dict(runs=0), dict(run_out=0), dict(ent=0), dict(vgot=0), dict(ev=0), dict(evr=0),
                 dict(lost=0), dict(out=0), dict(runs=b + case.o["runs"] + 8), dict(evr=b + case.o["evr"] + 8),
                 dict(ent=b + case.o["ent"] + 4), dict(vgot=b + case.o["vgot"] + 4), dict(ev=b + case.o["ev"] + 4),
                 dict(lost=b + case.o["lost"] + 4), dict(out=b + case.o["out"] + 4), dict(size_off=SIZE_OFF + 2),
                 dict(size_off=TBL_OFF), dict(tbl_off=TBL_OFF + 4), dict(nvgot=case.nvgot - 6), dict(n=1 << 28)):
        assert ctx.fill_device(case.args(**over)) == -errno.EINVAL, over
    a = case.args()
    a.vcap[int(np.argmax(case.vcap))] -= 1
    assert ctx.fill_device(a) == -errno.EINVAL
    assert np.array_equal(case.a.snapshot(), before)


# ---- the host forms --------------------------------------------------------------------
@pytest.mark.parametrize("submit", [False, True])
def test_host_form_page_locked(ctx, arena, submit):
    case = random_case(arena, 500, 3 * TILE + 77, stock="half")
    exp, care, res = case.expect()
    assert ctx.fill_host(case.args(), submit=submit) == 0
    case.check(exp, care, res)


@pytest.mark.parametrize("submit", [False, True])
def test_host_form_staged(ctx, arena, submit):
    """The arrays in pageable memory, the vectors in place: what the fill leaves
    alone in ev, evr and lost comes back as it was."""
    case = random_case(arena, 510, 3 * TILE + 77, stock="half")
    exp, care, res = case.expect()
    names = ("seq", "runs", "rout", "ent", "vgot", "ev", "evr", "lost", "out")
    heap = {k: getattr(case, k).copy() for k in names}
    over = {("run_out" if k == "rout" else k): v.ctypes.data for k, v in heap.items()}
    before = case.a.snapshot()
    assert ctx.fill_host(case.args(**over), submit=submit) == 0
    # the arena's arrays were not used; its vectors were
    after = case.a.snapshot()
    for k in ("ev", "evr", "lost", "out"):
        o, nb = case.o[k], heap[k].nbytes
        assert np.array_equal(after[o: o + nb], before[o: o + nb])
        got, want = heap[k].view(np.uint8), exp[o: o + nb]
        if k == "lost":
            nl = res["out"]["lost"]
            assert np.array_equal(np.sort(heap[k][:nl]), res["lost"]) and np.array_equal(got[8 * nl:], want[8 * nl:])
        else:
            assert np.array_equal(got, want), k
    assert np.array_equal(after[case.lo_off: case.hi_off], exp[case.lo_off: case.hi_off])
    # vectors outside page-locked memory: refused before anything runs
    pageable = np.zeros(1 << 16, np.uint8)
    assert ctx.fill_host(case.args(varena_lo=pageable.ctypes.data, varena_bytes=4096)) == -errno.EINVAL
    assert ctx.fill_host(case.args(varena_bytes=0), submit=True) == -errno.EINVAL


# ---- run plan -> vector fill on one stream -----------------------------------------------
def test_the_chain_on_one_stream(ctx, arena):
    """mi_cls_enq_runs and mi_cls_vec_fill on one side stream, the fill reading
    the plan's out on the device and nothing synchronised between them; against
    run_model and vec_model on the same records."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(77)
    n, ndst = 9 * TILE + 123, 40
    table, entry_of = M.make_table(rng, ndst)
    rtable = RM.make_rtable(rng, nslots=4, vmaxes=(2, 3, 8))
    lens_ = rng.integers(1, 13, n + 1)
    dst = np.repeat(rng.integers(0, ndst, n + 1), lens_)[:n]
    dst = np.where(rng.integers(0, 6, n) == 0, M.drops(n), dst)
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    seq, runs, rout = RM.plan_runs_np(rec, lens, table, rtable, 512)
    need = np.array(rout["vec_need"], np.int64)
    case = Case(arena, 600, n, runs, need, rtable, vhave=need - need // 3)
    case.seq[:], case.runs[:], case.rout[:] = 0xA5A5A5A5, 0, 0xA5A5A5A5A5A5A5A5     # the plan writes them
    t_res = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    t_len = torch.from_numpy(lens.astype(np.uint16).view(np.int16).copy()).to(dev)
    tab, rtab = cls.enq_tab(*table), cls.run_tab(*rtable)
    b = arena.ptr
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    a = case.args()
    with torch.cuda.stream(side):
        s = side.cuda_stream
        assert ctx.runs_device(t_res.data_ptr(), t_len.data_ptr(), n, tab, rtab, 512, b + case.o["seq"],
                               b + case.o["runs"], case.run_cap, b + case.o["rout"], s) == 0
        assert ctx.fill_device(a, s) == 0
    side.synchronize()
    assert np.array_equal(case.seq[:n], seq) and np.array_equal(case.runs[: case.nr], runs)
    assert int(case.rout[6]) == case.nr == rout["nruns"]
    res = case.model()
    assert res["out"]["lost"] > 0 and res["out"]["vectors"] > 100
    got_evr = case.evr[: case.nr]
    assert np.array_equal(got_evr, res["evr"])
    assert np.array_equal(case.ev[: res["out"]["ev_span"]], res["ev"])
    assert np.array_equal(np.sort(case.lost[: res["out"]["lost"]]), res["lost"])
    assert cls.vec_out_dict(case.out) == res["out"]
    v = case.vgot[res["vec_idx"]].astype(np.int64) - b
    sizes = arena.u8.view(np.uint32)[(v + SIZE_OFF) // 4]
    assert np.array_equal(sizes, res["vec_size"])
    first = np.cumsum(res["vec_size"]) - res["vec_size"]
    where = np.repeat((v + TBL_OFF) // 8 - first, res["vec_size"]) + np.arange(int(res["vec_size"].sum()))
    assert np.array_equal(arena.u8[: arena.nbytes & ~7].view(np.uint64)[where], res["vec_tbl"])


def test_pktio_form(arena):
    """odp_amd_cls_vec_fill is the library's fill on the pktio's context."""
    import torch
    c = cls.Classifier(gpu=0)
    try:
        c.apply([R.cos("a", queue=11), ("default", 0)])
        case = random_case(arena, 520, 2 * TILE + 9, stock="half")
        exp, care, res = case.expect()
        assert c.vec_fill(case.args()) == 0
        torch.cuda.synchronize()
        case.check(exp, care, res)
        assert res["out"]["lost"] > 0 and res["out"]["vectors"] > 0
    finally:
        c.close()


def test_pktio_form_over_several_gpus(built, gpu):
    m = cls.Classifier(gpus=[0, 0])
    try:
        m.apply([R.cos("a", queue=11), ("default", 0)])
        out = np.zeros(24, np.uint64)
        z = cls.vec_args(cls.run_tab([], [], []), out=out.ctypes.data, size_off=8, tbl_off=16)
        t = C.c_uint64(7)
        assert m.vec_fill(z) == -errno.ENOTSUP and m.vec_fill_host(z) == -errno.ENOTSUP
        assert m.L.odp_amd_cls_vec_fill_host_submit(m.pktio, C.byref(z), C.byref(t)) == -errno.ENOTSUP
        assert t.value == 0 and not out.any()
    finally:
        m.close()
