"""The pool move on the GPU (mi_cls_pool_move, include/mi_cls.h) against
tests/move_model.py.

Everything a run reads or writes lies in one rx_harness.Arena, filled with a
non-zero pattern first; afterwards the whole arena equals the image before the
call with the model's writes applied, except the bytes between a copied frame's
end and its 16-byte copy extent.  The declared packet arena is one region of
it: addresses a guard must refuse point into the regions before and behind, so
a broken guard shows as a compare failure.
"""
import ctypes as C
import errno

import numpy as np
import pytest

from odp_amd import cls
from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import enq_model as M
from tests import move_model as MM
from tests import pool_model as PM
from tests import rx_harness as H
from tests import zoo
from tests.helpers import oracle_run

pytestmark = pytest.mark.gpu

TILE, GRID, ROUND = cls.MOVE_TILE, cls.MOVE_GRID, cls.MOVE_ROUND
WAVES = 4                        # of a block: mi_cls_last_launch info[0] - 320 (checked below)
HEADROOM, DFM = 128, 192
INPUT = 0x0DD0_0000_0000_0042
NDST = 24
NONE, INPLACE, FRESH, TOO_LONG, SHORT = PM.PF_NONE, PM.PF_INPLACE, PM.PF_FRESH, PM.PF_TOO_LONG, PM.PF_SHORT
LENGTHS = (0, 1, 15, 16, 17, 60, 64, 65, ROUND - 1, ROUND, ROUND + 1, 1518, 9000, 65535)
BIG = 2 * GRID * WAVES * TILE + 40       # a wave's third tile, cut short
LOOP_MAX = 5000                          # records the per-record model takes


@pytest.fixture(scope="module")
def ctx(built, gpu):
    c = cls.EnqContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arena(built, gpu):
    a = H.Arena(72 << 20)
    yield a
    a.close()


def records(rng, n):
    """Records of every outcome over a random enqueue table, enqueue records of
    CoS and queues outside it among them (dst_queue 0)."""
    table, entry_of = M.make_table(rng, NDST)
    dst = np.where(rng.integers(0, 6, n) == 0, M.drops(n), rng.integers(0, NDST, n))
    rec, _ = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    rec["l3_offset"] = rng.integers(0, 2 ** 16, n)
    rec["l4_offset"] = rng.integers(0, 2 ** 16, n)
    wild = rng.integers(0, 9, n) == 0
    rec["cos"][wild] = rng.integers(0, 256, int(wild.sum()))
    rec["queue"][wild] = rng.integers(0, 70, int(wild.sum()))
    dst_queue = (0x7000_0000_0000 + 64 * rng.permutation(NDST)).astype(np.uint64)
    return rec, table, dst_queue


class Case:
    """One run's memory, laid out in the arena.  addr0: the address byte 0 of
    the arena has for the device (the arena's own, or a device tensor's)."""

    def __init__(self, arena, seed, lens, fate, *, addr0=None, dfm=DFM, pk="own", loop=False, residue=None,
                 exact_end=True, tab=None):
        rng = np.random.default_rng(seed)
        self.a, self.dfm, self.rng = arena, dfm, rng
        self.addr0 = arena.ptr if addr0 is None else addr0
        n = self.n = len(lens)
        lens = self.lens_in = np.asarray(lens, np.uint16)
        fate = np.asarray(fate, np.uint32)
        self.rec, self.table, self.dst_queue = tab or records(rng, n)
        self.rec = self.rec[:n]
        arena.reset()
        m = max(n, 1)
        nfresh = int((fate == FRESH).sum())
        self.ngot = nfresh + 8
        self.o = {}
        for name, dt, cnt in (("off", "<u4", m), ("len", "<u2", m), ("res", R.RESULT_DTYPE, m), ("dec", "<u4", m),
                              ("idx", "<u4", m), ("got", "<u8", self.ngot), ("pk", "<u8", m), ("ent", "<u8", m),
                              ("out", "<u8", 4)):
            self.o[name], arr = arena.array(name, dt, cnt)
            setattr(self, name, arr)
        ln64 = lens.astype(np.int64)
        # the packets: [line 64 B][dfm - 64][data]; before, inside and behind the declared arena
        stride_own = dfm + ((ln64 + 63) & ~63) + 64          # room for a data_off above HEADROOM
        have_own = pk == "own" or loop
        self.before = arena.alloc("before", 4 * (dfm + 256), 64)
        own_at = np.zeros(n, np.int64)
        if have_own:
            start = arena.alloc("own", int(stride_own.sum()) + 64, 64)
            own_at = start + np.cumsum(stride_own) - stride_own
        f = np.nonzero(fate == FRESH)[0]
        stride_got = dfm + ((ln64[f] + 63) & ~63)
        start = arena.alloc("fresh", int(stride_got.sum()) + 8 * (dfm + 64), 64)
        got_at = start + np.cumsum(stride_got) - stride_got
        spare_at = start + int(stride_got.sum()) + (dfm + 64) * np.arange(8)
        self.lo_off = self.o_own = (int(own_at[0]) if have_own and n else start)
        self.hi_off = arena.top
        self.behind = arena.alloc("behind", 4 * (dfm + 256), 64)
        # the frames: inside the own packets (loop), or packed at every residue with the last one at the very end
        if loop:
            self.pkts_off, self.pkts_bytes = self.lo_off, self.hi_off - self.lo_off
            foff = own_at + dfm + 2 * rng.integers(0, 8, n) - self.pkts_off
        else:
            res16 = rng.integers(0, 16, n) if residue is None else np.full(n, residue)
            gap = rng.integers(0, 3, n) * 16
            pos = np.zeros(n, np.int64)
            at = 0
            for i in range(n):
                at += int(gap[i])
                at += (int(res16[i]) - at) % 16
                pos[i] = at
                at += int(ln64[i])
            size = at + (0 if exact_end else 7)
            self.pkts_off = arena.alloc("frames", size + 1, 64)   # one byte behind: not the buffer's
            self.pkts_bytes = size
            foff = pos
        arena.fill(seed)
        self.off[:n], self.len[:n], self.res[:n] = foff, lens, self.rec
        order = rng.permutation(nfresh)
        self.idx[:] = 0xFFFFFFFF
        self.idx[:n][f] = order
        self.idx[:n][fate == NONE] = rng.integers(0, 2 ** 32, int((fate == NONE).sum()))   # never looked at
        self.dec[:n] = fate | rng.integers(0, 16, n).astype(np.uint32) << 4
        self.got[:] = 0
        self.got[:nfresh][order] = self.addr0 + got_at
        self.got[nfresh:] = self.addr0 + spare_at
        self.use_pk = pk is not None
        self.pk[:] = 0
        if have_own and pk == "own":
            self.pk[:n] = self.addr0 + own_at
            for i in range(n):
                ml = self.line(int(self.pk[i]))
                ml["data_off"] = HEADROOM + int(foff[i] + self.pkts_off - own_at[i] - dfm) if loop else HEADROOM + 2 * (i % 5)
                ml["user_ptr"] = int(rng.integers(1, 2 ** 62))

    def line(self, addr, image=None):
        u8 = self.a.u8 if image is None else image
        return u8[addr - self.addr0: addr - self.addr0 + 64].view(H.META_DTYPE)[0]

    def args(self, base=None, **over):
        """The MoveArgs with every pointer into the arena at `base` (default:
        addr0)."""
        b = self.addr0 if base is None else base
        kw = dict(pkts=b + self.pkts_off, pkts_bytes=self.pkts_bytes, off=b + self.o["off"], len=b + self.o["len"],
                  res=b + self.o["res"], dec=b + self.o["dec"], idx=b + self.o["idx"], got=b + self.o["got"],
                  pk=b + self.o["pk"] if self.use_pk else 0, n=self.n, ngot=self.ngot, input=INPUT,
                  headroom=HEADROOM, data_from_meta=self.dfm, arena_lo=self.addr0 + self.lo_off,
                  arena_bytes=self.hi_off - self.lo_off, ent=b + self.o["ent"], out=b + self.o["out"])
        kw.update(over)
        return cls.move_args(cls.enq_tab(*self.table), self.dst_queue, **kw)

    def expect(self, arena_bytes=None):
        """(image, care, out) after the move, from the arena as it is now."""
        n = self.n
        snap = self.a.snapshot()
        care = np.ones(len(snap), np.uint8)
        pkts = snap[self.pkts_off: self.pkts_off + self.pkts_bytes]
        nb = self.hi_off - self.lo_off if arena_bytes is None else arena_bytes
        if n <= LOOP_MAX:
            ent, out, writes = MM.move(pkts, self.pkts_bytes, self.off[:n], self.len[:n], self.res[:n], self.dec[:n],
                                       self.idx[:n], self.got, self.pk[:n] if self.use_pk else None, self.table,
                                       self.dst_queue, INPUT, HEADROOM, self.dfm, self.addr0 + self.lo_off, nb,
                                       lambda addr: self.line(addr, snap))
            exp = snap.copy()
            MM.apply(writes, exp, self.addr0, self.dfm, care)
        else:
            assert not self.use_pk
            exp = snap.copy()
            ent, out = MM.move_np(exp, self.addr0, self.pkts_off, self.off[:n], self.len[:n], self.res[:n],
                                  self.dec[:n], self.idx[:n], self.got, self.table, self.dst_queue, INPUT, HEADROOM,
                                  self.dfm, care)
        exp[self.o["ent"]: self.o["ent"] + 8 * n] = ent.view(np.uint8)
        exp[self.o["out"]: self.o["out"] + 32] = np.array([out[k] for k in MM.OUT_FIELDS], np.uint64).view(np.uint8)
        return exp, care, out

    def check(self, exp, care, got=None):
        H.compare(self.a, self.a.u8[: self.a.top] if got is None else got, exp, care)


def run(ctx, case, **over):
    """The device form on the arena's own (device-mapped) addresses."""
    exp, care, out = case.expect(over.get("arena_bytes"))
    ctx.move(case.args(**over))
    case.check(exp, care)
    return out


def fates(rng, n, share=(1, 2, 3, 1, 1)):
    """Random fates, weighted NONE, INPLACE, FRESH, TOO_LONG, SHORT."""
    p = np.array(share, float)
    return rng.choice(5, n, p=p / p.sum()).astype(np.uint32)


# ---- sizes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, TILE * WAVES - 1, TILE * WAVES, TILE * WAVES + 1])
def test_sizes(ctx, arena, n):
    rng = np.random.default_rng(n)
    lens = rng.choice([0, 1, 17, 60, 64, 65, 300, 1518], n)
    case = Case(arena, 100 + n, lens, fates(rng, n))
    out = run(ctx, case)
    info = ctx.last_launch()
    assert info[0] == 320 + WAVES and info[1] == (2 if n else 1)
    assert info[6] == min(GRID, (n + TILE * WAVES - 1) // (TILE * WAVES))
    if n >= 63:
        assert out["moved"] and out["inplace"] and not out["refused"]


def test_three_tiles_per_wave(ctx, arena):
    """More than twice the grid's records: wave 0's third tile is cut short.
    60-B frames, every record FRESH, the data right behind the line."""
    case = Case(arena, 7, np.full(BIG, 60), np.full(BIG, FRESH), dfm=64, pk=None)
    out = run(ctx, case)
    assert out == {"moved": BIG, "inplace": 0, "bytes": 60 * BIG, "refused": 0}
    assert ctx.last_launch()[6] == GRID


# ---- lengths and source offsets ------------------------------------------------------------
@pytest.mark.parametrize("residue", range(16))
def test_lengths_at_every_source_residue(ctx, arena, residue):
    """Every length at one residue mod 16 of the source offset, all in one
    tile; the last frame ends exactly at pkts_bytes (65535 B at residue 0, one
    byte at the others: the byte-wise end of the buffer)."""
    lens = list(LENGTHS) + [3, 1][: 2 if residue else 0]
    case = Case(arena, 200 + residue, lens, np.full(len(lens), FRESH), residue=residue, pk=None, exact_end=True)
    assert int(case.off[case.n - 1]) + int(case.len[case.n - 1]) == case.pkts_bytes
    out = run(ctx, case)
    assert out["moved"] == len(lens) and out["bytes"] == sum(lens)


# ---- tile mixes ----------------------------------------------------------------------------
def _mix(name, rng):
    n = 3 * TILE
    lens = rng.choice([0, 1, 17, 60, 64, 65, 300, 1518, 9000], n)
    if name == "all_fresh":
        f = np.full(n, FRESH)
    elif name == "no_fresh":
        f = fates(rng, n, (1, 2, 0, 1, 1))
    elif name == "lane0":
        f = fates(rng, n, (1, 2, 0, 1, 1))
        f[::TILE] = FRESH
    elif name == "lane63":
        f = fates(rng, n, (1, 2, 0, 1, 1))
        f[TILE - 1::TILE] = FRESH
    elif name == "one_long":
        f = np.full(n, FRESH)
        lens[:] = 1
        lens[[5, TILE + 63, 2 * TILE]] = 65535
    else:
        f = fates(rng, n)
    return lens, f


@pytest.mark.parametrize("name", ["all_fresh", "no_fresh", "lane0", "lane63", "one_long", "random"])
def test_tile_mixes(ctx, arena, name):
    rng = np.random.default_rng(len(name))
    lens, f = _mix(name, rng)
    out = run(ctx, Case(arena, 300 + len(name), lens, f))
    assert out["moved"] == int((f == FRESH).sum()) and out["inplace"] == int((f == INPLACE).sum())


# ---- pk -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["null", "inplace", "fresh", "zero", "loop"])
def test_pk_variants(ctx, arena, variant):
    """pk NULL (an INPLACE record is then refused); pk given with INPLACE
    records (data_off and user_ptr stay); with FRESH ones (the user pointer
    travels); pk[i] == 0; the frames inside the pk packets' own data areas."""
    rng = np.random.default_rng(len(variant))
    n = 2 * TILE + 9
    lens = rng.choice([0, 1, 17, 60, 64, 65, 300, 1518], n)
    f = fates(rng, n, {"inplace": (1, 4, 0, 1, 1), "fresh": (1, 0, 4, 1, 1)}.get(variant, (1, 2, 3, 1, 1)))
    case = Case(arena, 400 + len(variant), lens, f, pk=None if variant == "null" else "own", loop=variant == "loop")
    if variant == "zero":
        case.pk[: n][::3] = 0
    out = run(ctx, case)
    ninpl = int((f == INPLACE).sum())
    if variant == "null":
        assert out["refused"] == ninpl and out["inplace"] == 0
    elif variant == "zero":
        assert out["refused"] == int((f[::3] == INPLACE).sum())
    else:
        assert out["refused"] == 0 and out["inplace"] == ninpl


# ---- guards -------------------------------------------------------------------------------
def test_guards(ctx, arena):
    """One record per guard beside valid ones: refused, counted, nothing of it
    written.  The addresses outside the declared arena lie in the arena's
    regions before and behind it."""
    n = TILE + 20
    f = np.full(n, FRESH, np.uint32)
    f[40:50] = INPLACE
    fresh = [i for i in range(n) if f[i] == FRESH]
    lens = np.full(n, 100)
    lens[fresh[25]] = 128
    case = Case(arena, 500, lens, f)
    a0, nf = case.addr0, len(fresh)
    spare = [int(x) for x in case.got[nf:]]
    # the declared arena ends 128 data bytes into the 4th spare packet
    nbytes = spare[3] - a0 + DFM + 128 - case.lo_off
    bad = {}

    def spoil(i, why, **kw):
        bad[i] = why
        for k, v in kw.items():
            arr = getattr(case, k)
            arr[int(case.idx[i]) if k == "got" else i] = v

    spoil(fresh[3], "idx == ngot", idx=case.ngot)
    spoil(fresh[5], "idx far past ngot", idx=0xFFFFFFFF)
    spoil(fresh[7], "packet 0", got=0)
    spoil(fresh[9], "packet not 64-B aligned", got=int(case.got[case.idx[fresh[9]]]) + 16)
    spoil(fresh[11], "packet before the arena", got=a0 + case.before)
    spoil(fresh[13], "packet behind the arena", got=a0 + case.behind)
    spoil(fresh[15], "data past the arena's end", got=spare[3] + 64)
    spoil(fresh[17], "line inside, data past the arena's end", got=spare[4])
    spoil(fresh[19], "frame one byte past pkts_bytes", off=case.pkts_bytes - 99)
    spoil(fresh[21], "frame far past pkts_bytes", off=0xFFFFFFFF)
    spoil(fresh[23], "a FRESH record's own packet outside the arena", pk=a0 + case.behind)
    spoil(41, "INPLACE, packet 0", pk=0)
    spoil(43, "INPLACE, not aligned", pk=int(case.pk[43]) + 32)
    spoil(45, "INPLACE, before the arena", pk=a0 + case.before + 64)
    spoil(47, "INPLACE, line right behind the arena", pk=a0 + case.lo_off + nbytes)
    # valid at the very edge: a packet whose data ends exactly at the arena's end
    case.got[case.idx[fresh[25]]] = spare[3]
    exp, care, out = case.expect(nbytes)
    ents = exp[case.o["ent"]: case.o["ent"] + 8 * n].view(np.uint64)
    assert out["refused"] == len(bad) and all(ents[i] == 0 for i in bad), bad
    assert ents[fresh[25]] == spare[3] and out["moved"] == nf - 11 and out["inplace"] == 6
    ctx.move(case.args(arena_bytes=nbytes))
    case.check(exp, care)


# ---- host forms ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["in_place", "staged", "submit", "staged_submit"])
@pytest.mark.parametrize("n", [0, 1, 3 * TILE + 5])
def test_host_forms(ctx, arena, n, form):
    rng = np.random.default_rng(n + len(form))
    lens = rng.choice([0, 1, 17, 60, 64, 65, 300, 1518, 9000], n)
    case = Case(arena, 600 + n, lens, fates(rng, n))
    exp, care, out = case.expect()
    orig = case.a.snapshot()
    submit = form.endswith("submit")
    if form.startswith("staged"):
        # pageable copies of every array and of the frames; ent and out come back into pageable memory
        keep = {k: getattr(case, k).copy() for k in ("off", "len", "res", "dec", "idx", "got", "pk")}
        frames = case.a.u8[case.pkts_off: case.pkts_off + case.pkts_bytes].copy() if n else np.zeros(16, np.uint8)
        ent, o = np.full(max(n, 1), 0x5A5A, np.uint64), np.full(4, 7, np.uint64)
        a = case.args(pkts=frames.ctypes.data, ent=ent.ctypes.data, out=o.ctypes.data,
                      **{k: v.ctypes.data for k, v in keep.items()})
    else:
        a = case.args()
    rc = ctx.move_host(a, submit="ticket" if submit else False)
    if submit:
        assert rc > 0
        ctx.move_wait(rc)
    else:
        assert rc == 0
    if form.startswith("staged"):
        lo, hi = case.o["ent"], case.o["out"] + 32
        assert ent[:n].tobytes() == exp[lo: lo + 8 * n].tobytes()
        assert o.tobytes() == exp[case.o["out"]: case.o["out"] + 32].tobytes()
        exp[lo: hi] = orig[lo: hi]             # the arena's own ent and out: not this call's
    case.check(exp, care)


def test_host_form_needs_a_mapped_arena(ctx, arena):
    """-EINVAL when either end of the packet arena is not page-locked memory
    the device addresses; nothing is written."""
    case = Case(arena, 700, np.full(10, 60), np.full(10, FRESH))
    before = case.a.snapshot()
    heap = np.zeros(1 << 16, np.uint8)
    for over in (dict(arena_lo=heap.ctypes.data, arena_bytes=4096),
                 dict(arena_bytes=arena.nbytes + (1 << 30)),
                 dict(arena_bytes=0)):
        assert ctx.move_host(case.args(**over)) == -errno.EINVAL
        assert ctx.move_host(case.args(**over), submit=True) == -errno.EINVAL
    assert np.array_equal(case.a.snapshot(), before)


def test_errors(ctx, arena):
    case = Case(arena, 701, np.full(4, 60), np.full(4, FRESH))
    before = case.a.snapshot()
    for over in (dict(pkts=0), dict(off=0), dict(len=0), dict(res=0), dict(dec=0), dict(idx=0), dict(ent=0),
                 dict(out=0), dict(got=0), dict(res=case.addr0 + case.o["res"] + 8),
                 dict(ent=case.addr0 + case.o["ent"] + 4), dict(out=case.addr0 + case.o["out"] + 4),
                 dict(data_from_meta=200), dict(pkts_bytes=1 << 32)):
        assert ctx.move_device(case.args(**over)) == -errno.EINVAL, over
    assert np.array_equal(case.a.snapshot(), before)


# ---- frames and packets in device memory -------------------------------------------------
def test_everything_in_hbm(ctx, arena):
    """The same image in a device tensor: arena_lo is the tensor's address."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(8)
    n = 5 * TILE + 3
    lens = rng.choice(LENGTHS[:-1] + (300, 300, 60, 60), n)
    t = torch.empty(arena.nbytes, dtype=torch.uint8, device=dev)
    case = Case(arena, 800, lens, fates(rng, n), addr0=t.data_ptr())
    exp, care, out = case.expect()
    top = case.a.top
    t[:top].copy_(torch.from_numpy(case.a.u8[:top]))
    ctx.move(case.args())
    case.check(exp, care, t[:top].cpu().numpy())
    assert out["moved"] and out["inplace"]


# ---- with real records: classify -> pool plan -> pool move -> enqueue plan on one stream ---
def test_the_chain_on_one_stream(built, gpu):
    """About 2000 zoo frames over the zoo's program with three CoS pools:
    classify, the pool plan, the pool move and the enqueue plan on one stream,
    nothing synchronised between them, against the oracle's records through
    pool_model, move_model and enq_model.  Through the pktio's forms
    (Classifier.pool_move), which are the library's on its context."""
    import torch
    frames = [f for _, f in zoo.all_frames()]
    frames = (frames * (2000 // len(frames) + 1))[:2000]
    b = pg.batch_from_frames(frames)
    prog = zoo.prog_everything()
    exp_rec, _ = oracle_run(prog, b)
    c = cls.Classifier(gpu=0)
    try:
        c.apply(prog)
        for i, h in enumerate(c.cos):
            if i % 3:
                assert c.L.odp_cls_cos_pool_set(h, i % 3) == 0
        caps = {9: 1536, 1: 128, 2: 9024}
        ptab, pools, _ = c.pool_table(caps, pktio_pool=9)
        ptable = PM.ptable_of(ptab)
        assert ptable[2] == len(pools) == 3
        tab, queues, _ = c.enq_table()
        table = M.table_of(tab)
        dst_queue = np.array(queues, np.uint64)
        n = b.n
        need = np.array(PM.plan_pools_np(exp_rec, b.len, None, ptable, [PM.UNLIMITED] * 16, [0] * 16)[3]["need"])
        have = (need * 2 // 3).tolist()
        base = (np.cumsum(need) - need).tolist()
        # the packets, in a device tensor: slot k's at base[k], of its capacity
        dev = torch.device("cuda:0")
        stride = [DFM + caps[p] for p in pools]
        starts = np.cumsum([0] + [have[k] * stride[k] for k in range(3)])
        t_pkt = torch.full((int(starts[-1]) + 64,), 0x5A, dtype=torch.uint8, device=dev)
        lo = (t_pkt.data_ptr() + 63) & ~63
        got = np.zeros(int(max(base[k] + have[k] for k in range(3))), np.uint64)
        for k in range(3):
            got[base[k]: base[k] + have[k]] = lo + int(starts[k]) + stride[k] * np.arange(have[k])
        t_got = torch.from_numpy(got.view(np.int64)).to(dev)
        t_buf = torch.from_numpy(np.ascontiguousarray(b.buf)).to(dev)
        t_off = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        t_len = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        t_rec = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
        t_dec = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t_idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t_pout = torch.full((40,), -1, dtype=torch.int32, device=dev)
        t_ent = torch.full((n,), -1, dtype=torch.int64, device=dev)
        t_mout = torch.full((4,), -1, dtype=torch.int64, device=dev)
        t_perm = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t_gbeg = torch.full((table[3] + 2,), -1, dtype=torch.int32, device=dev)
        t_eout = torch.full((6,), -1, dtype=torch.int64, device=dev)
        before = t_pkt.cpu().numpy()
        a = cls.move_args(tab, dst_queue, pkts=t_buf.data_ptr(), pkts_bytes=t_buf.numel(), off=t_off.data_ptr(),
                          len=t_len.data_ptr(), res=t_rec.data_ptr(), dec=t_dec.data_ptr(), idx=t_idx.data_ptr(),
                          got=t_got.data_ptr(), ngot=len(got), n=n, input=INPUT, headroom=HEADROOM,
                          data_from_meta=DFM, arena_lo=lo, arena_bytes=int(starts[-1]), ent=t_ent.data_ptr(),
                          out=t_mout.data_ptr())
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        u = C.c_uint32 * cls.POOL_SLOTS
        with torch.cuda.stream(side):
            s = side.cuda_stream
            assert c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_rec.data_ptr(), s) == 0
            assert c.L.odp_amd_cls_pool_plan(c.pktio, t_rec.data_ptr(), t_len.data_ptr(), None, n, C.byref(ptab),
                                             u(*have), u(*base), t_rec.data_ptr(), t_dec.data_ptr(),
                                             t_idx.data_ptr(), t_pout.data_ptr(), s) == 0
            assert c.pool_move(a, s) == 0
            assert c.L.odp_amd_cls_enq_plan(c.pktio, t_rec.data_ptr(), t_len.data_ptr(), n, C.byref(tab),
                                            t_perm.data_ptr(), t_gbeg.data_ptr(), t_eout.data_ptr(), s) == 0
        side.synchronize()
        # the models, on the oracle's records
        res_out, dec, idx, pout = PM.plan_pools(exp_rec, b.len, None, ptable, have, base)
        assert pout["fresh"] > 300 and pout["shorted"] > 50 and pout["too_long"] > 5
        ent, mout, writes = MM.move(np.ascontiguousarray(b.buf), t_buf.numel(), b.off, b.len, res_out, dec, idx, got,
                                    None, table, dst_queue, INPUT, HEADROOM, DFM, lo, int(starts[-1]), None)
        exp = before.copy()
        care = np.ones(len(exp), np.uint8)
        MM.apply(writes, exp, t_pkt.data_ptr(), DFM, care)
        after = t_pkt.cpu().numpy()
        assert np.array_equal(t_ent.cpu().numpy().view(np.uint64), ent)
        assert cls.move_out_dict(t_mout.cpu().numpy().view(np.uint64)) == mout and mout["refused"] == 0
        bad = np.nonzero((after != exp) & (care != 0))[0]
        assert not len(bad), f"{len(bad)} bytes of the packets differ, first at {bad[0]}"
        perm, gbeg, ctr = M.plan(res_out, b.len, table)
        assert np.array_equal(t_perm.cpu().numpy().view(np.uint32), perm)
        assert np.array_equal(t_gbeg.cpu().numpy().view(np.uint32), gbeg)
        assert dict(zip(M.FIELDS, (int(v) for v in t_eout.cpu().numpy().view(np.uint64)))) == ctr
        # every delivered record's packet is one the move wrote
        dlv = perm[: gbeg[table[3]]]
        assert (ent[dlv] != 0).all() and mout["moved"] >= len(dlv)
    finally:
        c.close()
    m = cls.Classifier(gpus=[0, 0])
    try:
        m.apply(prog)
        out = np.zeros(4, np.uint64)
        z = cls.move_args(tab, dst_queue, out=out.ctypes.data, data_from_meta=DFM)
        t = C.c_uint64(7)
        assert m.pool_move(z) == -errno.ENOTSUP and m.pool_move_host(z) == -errno.ENOTSUP
        assert m.L.odp_amd_cls_pool_move_host_submit(m.pktio, C.byref(z), C.byref(t)) == -errno.ENOTSUP
        assert t.value == 0 and not out.any()
    finally:
        m.close()
