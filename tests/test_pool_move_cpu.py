"""The pool move without a GPU: its model (tests/move_model.py) against the
reference's loop on packet objects and against the receive chain's model, and
the argument checks of the library's entry points."""
import ctypes as C
import errno

import numpy as np
import pytest

from odp_amd import rules as R
from tests import enq_model as M
from tests import move_model as MM
from tests import pool_model as PM
from tests import rx_model as RX

BASE = 0x7F12_3400_0000          # address of byte 0 of the flat memory
HEADROOM, DFM = 128, 192         # a fresh packet's data_off; from a line to its data
INPUT = 0x0DD0_0000_0000_0042
CAPS = (256, 1536, 9024)


class Flat:
    """A flat memory of packets: 64 bytes of header, the 64-byte line, then
    headroom and data.  Everything in it is the arena."""

    def __init__(self, rng, nbytes):
        self.u8 = rng.integers(1, 256, nbytes, dtype=np.uint8)
        self.top = 0

    def packet(self, cap):
        """The line address of a new packet of `cap` data bytes."""
        self.top = (self.top + 63) & ~63
        line = BASE + self.top + 64
        self.top += 64 + DFM + ((cap + 63) & ~63) + 64
        assert self.top <= len(self.u8)
        return line

    def line_at(self, addr, image=None):
        u8 = self.u8 if image is None else image
        return u8[addr - BASE: addr - BASE + 64].view(RX.META_DTYPE)[0]


def batch(rng, n, nslot, ndst=24, every_cos_has_a_slot=False):
    """Records, lens (short frames mostly), own and the two tables of one control
    plane, with enqueue records of CoS outside it among them."""
    table, entry_of = M.make_table(rng, ndst)
    dst = np.where(rng.integers(0, 5, n) == 0, M.drops(n), rng.integers(0, ndst, n))
    rec, lens = M.make_records(rng, n, dst, entry_of, R.RESULT_DTYPE)
    lens = np.where(rng.integers(0, 50, n) == 0, lens, lens % 700).astype(np.uint16)
    rec["l3_offset"] = rng.integers(0, 2 ** 16, n)
    rec["l4_offset"] = rng.integers(0, 2 ** 16, n)
    if every_cos_has_a_slot:
        ptable = (rng.integers(0, nslot, 256).astype(np.uint8), PM.make_ptable(rng, nslot, caps=CAPS)[1], nslot)
    else:
        ptable = PM.make_ptable(rng, nslot, cos_nq=table[0], caps=CAPS)
        wild = rng.integers(0, 15, n) == 0
        rec["outcome"][wild] = M.OUT_ENQ
        rec["cos"][wild] = rng.integers(0, 256, int(wild.sum()))
        rec["queue"][wild] = rng.integers(0, 70, int(wild.sum()))
    dst_queue = (0x7000_0000_0000 + 64 * rng.permutation(ndst)).astype(np.uint64)
    return rec, lens, PM.make_own(rng, rec, ptable), ptable, table, dst_queue


def lay_out(rng, rec, lens, own, ptable, have, loop):
    """The memory of a batch: with `loop` every frame sits in a packet of its
    own (pk[i]; own[i] says of which pool) with a user pointer and a headroom of
    its own; else the frames are packed one after another and pk is None.  Then
    have[k] fresh packets per slot.  Returns (mem, off, pk, got, base, pools):
    pools maps a fresh packet's line address to its slot."""
    n = len(rec)
    caps = [int(c) for c in ptable[1]]
    need = int(lens.astype(np.int64).sum()) + 512 * n + sum(int(h) * (caps[k] + 512) for k, h in enumerate(have))
    mem = Flat(rng, need + 4096)
    off = np.zeros(n, np.uint32)
    pk = None
    if loop:
        pk = np.zeros(n, np.uint64)
        for i in range(n):
            pk[i] = mem.packet(int(lens[i]))
            m = mem.line_at(int(pk[i]))
            m["data_off"] = HEADROOM + 2 * int(rng.integers(0, 8))
            m["user_ptr"] = int(rng.integers(1, 2 ** 62))
            # the frame starts data_off - HEADROOM into the data area
            off[i] = int(pk[i]) - BASE + DFM + int(m["data_off"]) - HEADROOM
    else:
        at = mem.top
        for i in range(n):
            off[i] = at
            at += int(lens[i])
        mem.top = at
    got, base, pools = [], [], {}
    for k, h in enumerate(have):
        base.append(len(got))
        for _ in range(int(h)):
            got.append(mem.packet(caps[k]))
            pools[got[-1]] = k
    return mem, off, pk, np.array(got, np.uint64), base, pools


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("seed,n,nslot,share", [(1, 0, 1, 1), (2, 1, 1, 1), (3, 400, 1, 3), (4, 900, 3, 3),
                                                (5, 900, 16, 1), (6, 600, 4, 2)])
def test_plan_and_move_are_the_reference_loop(seed, n, nslot, share, loop):
    """pool_model.plan_pools then move_model.move leave every delivered frame
    where the reference's loop leaves it: in its own packet when that is of the
    CoS's pool, else in the next free packet of that pool, with its bytes, its
    metadata and the user pointer odp_packet_copy carries; every other frame in
    no packet.  share: have = need // share (a short pool beyond 1)."""
    rng = np.random.default_rng(seed)
    rec, lens, own, ptable, table, dst_queue = batch(rng, n, nslot)
    own = own if loop else None
    need = np.array(PM.plan_pools(rec, lens, own, ptable, [PM.UNLIMITED] * PM.SLOTS, [0] * PM.SLOTS)[3]["need"])
    have = (need // share).tolist()
    mem, off, pk, got, base, pools = lay_out(rng, rec, lens, own, ptable, have, loop)
    res_out, dec, idx, pout = PM.plan_pools(rec, lens, own, ptable, have, base)
    before = mem.u8.copy()
    ent, out, writes = MM.move(mem.u8, len(mem.u8), off, lens, res_out, dec, idx, got, pk, table, dst_queue, INPUT,
                               HEADROOM, DFM, BASE, len(mem.u8), mem.line_at)
    after = before.copy()
    MM.apply(writes, after, BASE, DFM)
    assert np.array_equal(mem.u8, before)   # the model writes nothing itself
    # the reference, on packet objects
    frames = [before[int(off[i]): int(off[i]) + int(lens[i])] for i in range(n)]
    pkt_pool = [None] * n
    user_ptr = [0] * n
    if loop:
        pkt_pool = [int(o) - 1 if 1 <= int(o) <= nslot else None for o in own]
        user_ptr = [int(mem.line_at(int(p), before)["user_ptr"]) for p in pk]
    free = [[int(a) for a in got[base[k]: base[k] + have[k]]] for k in range(nslot)]
    ref = MM.reference_packets(frames, rec, pkt_pool, user_ptr, ptable, free, table, dst_queue, INPUT, HEADROOM)
    delivered = 0
    for i in range(n):
        p = ref[i]
        if p is None:
            assert ent[i] == 0
            continue
        delivered += 1
        line = int(ent[i])
        if p.name is None:      # it stayed in its own packet
            assert line == int(pk[i]) and pkt_pool[i] == p.pool
            doff, data = int(mem.line_at(line, before)["data_off"]), int(off[i])
        else:
            assert line == p.name and pools[line] == p.pool
            doff, data = p.headroom, line - BASE + DFM
        m = mem.line_at(line, after)
        assert after[data: data + p.len].tobytes() == p.data
        assert (int(m["data_off"]), int(m["len"]), int(m["in_flags"]), int(m["err"]), int(m["cos"]),
                int(m["cls_mark"]), int(m["l2"]), int(m["l3"]), int(m["l4"]), int(m["dst_queue"]), int(m["input"]),
                int(m["user_ptr"])) == (doff, p.len, p.in_flags, p.err, p.cos, p.mark, 0, p.l3, p.l4, p.dst_queue,
                                        p.input, p.user_ptr)
        assert (int(m["rsv0"]), int(m["rsv1"]), int(m["rsv2"])) == (0, 0, 0)
    assert out == {"moved": pout["fresh"], "inplace": pout["inplace"], "refused": 0,
                   "bytes": int(lens.astype(np.int64)[(dec & 15) == PM.PF_FRESH].sum())}
    assert delivered == pout["fresh"] + pout["inplace"] == len(writes)
    # nothing but the delivered packets' lines and copied data changed
    touched = np.zeros(len(after), bool)
    for line, _, frame in writes:
        touched[line - BASE: line - BASE + 64] = True
        if frame is not None:
            touched[line - BASE + DFM: line - BASE + DFM + len(frame)] = True
    assert np.array_equal(after[~touched], before[~touched])


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("seed,n,nslot,share", [(1, 1, 1, 1), (2, 700, 3, 1), (3, 8192, 16, 2), (4, 3000, 4, 3)])
def test_move_is_the_receive_chains_delivery(seed, n, nslot, share, loop):
    """For a burst the receive chain takes, ent and every written line are
    rx_model.decide's and chain_meta's on equivalent tables (every CoS has a
    slot there)."""
    rng = np.random.default_rng(seed)
    rec, lens, own, ptable, table, dst_queue = batch(rng, n, nslot, every_cos_has_a_slot=True)
    # the chain's table maps every enqueue record: keep the mapped ones
    stale = M.keys(rec, table)[1]
    rec["outcome"][stale] = M.OUT_DISCARD
    own = own if loop else None
    need = np.array(PM.plan_pools(rec, lens, own, ptable, [PM.UNLIMITED] * PM.SLOTS, [0] * PM.SLOTS)[3]["need"])
    have = (need // share).tolist()
    mem, off, pk, got, base, _ = lay_out(rng, rec, lens, own, ptable, have, loop)
    res_out, dec, idx, _ = PM.plan_pools(rec, lens, own, ptable, have, base)
    ent, out, writes = MM.move(mem.u8, len(mem.u8), off, lens, res_out, dec, idx, got, pk, table, dst_queue, INPUT,
                               HEADROOM, DFM, BASE, len(mem.u8), mem.line_at)
    cos_nq, cos_q0, ent_dst, ndst = table
    tab = np.zeros((), RX.RXTAB_DTYPE)
    tab["flags"], tab["npool"] = RX.RXT_CLS, nslot
    tab["pool_cap"], tab["cos_pool"] = ptable[1], ptable[0]
    tab["cos_nq"], tab["cos_q0"] = cos_nq, cos_q0
    tab["rt_slot"][:RX.RX_POOLS] = np.arange(1, RX.RX_POOLS + 1)   # pool handle p is slot p - 1
    nent = int(cos_q0.astype(np.int64).max()) + M.NQ
    assert nent <= RX.RX_QENT
    ids = ent_dst[:nent].astype(np.int64)
    tab["qh"][:nent] = np.where(ids < ndst, dst_queue[np.minimum(ids, ndst - 1)], 0)
    d = RX.decide(rec, lens, tab, PM._pad(have), PM._pad(base), got, pk=pk, ppool=own)
    assert np.array_equal(ent, d.ent)
    lines = {line: text for line, text, _ in writes}
    assert len(lines) == int(d.delivered.sum())
    for i in np.nonzero(d.delivered)[0]:
        old = mem.line_at(int(d.ent[i]))
        pm = mem.line_at(int(pk[i])) if loop else None
        assert lines[int(ent[i])] == RX.chain_meta(d, i, rec[i], int(lens[i]), HEADROOM, INPUT, old, pm)


@pytest.mark.parametrize("seed,n,nslot", [(1, 1, 1), (2, 900, 3), (3, 2000, 16)])
def test_model_pair(seed, n, nslot):
    """move_np() is move() then apply() where no record has a packet of its own
    and none is refused."""
    rng = np.random.default_rng(seed)
    rec, lens, _, ptable, table, dst_queue = batch(rng, n, nslot)
    need = np.array(PM.plan_pools(rec, lens, None, ptable, [PM.UNLIMITED] * PM.SLOTS, [0] * PM.SLOTS)[3]["need"])
    have = (need * 2 // 3).tolist()
    mem, off, _, got, base, _ = lay_out(rng, rec, lens, None, ptable, have, False)
    res_out, dec, idx, _ = PM.plan_pools(rec, lens, None, ptable, have, base)
    ent, out, writes = MM.move(mem.u8, len(mem.u8), off, lens, res_out, dec, idx, got, None, table, dst_queue, INPUT,
                               HEADROOM, DFM, BASE, len(mem.u8), mem.line_at)
    a, b = mem.u8.copy(), mem.u8.copy()
    ca, cb = np.ones(len(a), np.uint8), np.ones(len(a), np.uint8)
    MM.apply(writes, a, BASE, DFM, ca)
    ent2, out2 = MM.move_np(b, BASE, 0, off, lens, res_out, dec, idx, got, table, dst_queue, INPUT, HEADROOM, DFM, cb)
    assert np.array_equal(ent, ent2) and out == out2
    assert np.array_equal(ca, cb) and np.array_equal(a[ca != 0], b[cb != 0])


def test_model_guards():
    """Each guard refuses its record and nothing else."""
    rng = np.random.default_rng(9)
    table, entry_of = M.make_table(rng, 4)
    rec, _ = M.make_records(rng, 8, np.arange(8) % 4, entry_of, R.RESULT_DTYPE)
    lens = np.full(8, 100, np.uint16)
    mem = Flat(rng, 1 << 16)
    got = np.array([mem.packet(256) for _ in range(3)] + [0, BASE + 8, BASE + len(mem.u8) - 64], np.uint64)
    pk = np.array([mem.packet(256) for _ in range(8)], np.uint64)
    off = np.arange(8, dtype=np.uint32) * 128 + 40000
    dec = np.full(8, PM.PF_FRESH, np.uint32)
    idx = np.array([0, 1, 6, 3, 4, 5, 2, 2], np.uint32)   # 6: past ngot; 3, 4, 5: bad packets
    off[6] = len(mem.u8) - 99                             # one byte past the buffer
    dec[7] = PM.PF_INPLACE
    pk[7] = BASE + len(mem.u8)                            # behind the arena
    args = (mem.u8, len(mem.u8), off, lens, rec, dec, idx, got)
    rest = (table, np.arange(4, dtype=np.uint64) + 7, INPUT, HEADROOM, DFM, BASE, len(mem.u8), mem.line_at)
    ent, out, writes = MM.move(*args, pk, *rest)
    assert ent.tolist() == [int(got[0]), int(got[1]), 0, 0, 0, 0, 0, 0]
    assert out == {"moved": 2, "inplace": 0, "bytes": 200, "refused": 6} and len(writes) == 2
    dec[7] = PM.PF_INPLACE
    ent, out, _ = MM.move(*args, None, *rest)              # INPLACE without a pk
    assert ent[7] == 0 and out["refused"] == 6


# ---- the library's entry points --------------------------------------------
def test_struct_mirrors(built):
    from odp_amd import cls
    assert C.sizeof(cls.MoveOut) == 32 and cls.MOVE_OUT_FIELDS == MM.OUT_FIELDS
    assert C.sizeof(cls.MoveArgs) == 144 and cls.MoveArgs.n.offset == 72 and cls.MoveArgs.tab.offset == 80
    assert cls.MoveArgs.input.offset == 96 and cls.MoveArgs.arena_lo.offset == 112 and cls.MoveArgs.out.offset == 136
    assert (cls.MOVE_TILE, cls.MOVE_ROUND) == (64, 8192) and cls.MOVE_ROUND % (16 * cls.MOVE_TILE) == 0
    assert cls.MOVE_GRID == 512
    assert cls.move_out_dict([1, 2, 3, 4]) == {"moved": 1, "inplace": 2, "bytes": 3, "refused": 4}


def test_library_entries_without_a_context(built):
    """The table and the scalars are checked first, with or without a device.
    No context: -ENODEV where there is no device (-EINVAL where there is one).
    Nothing is written."""
    from odp_amd import cls
    L = cls.lib()
    out = np.zeros(4, np.uint64)
    good = cls.enq_tab([1], [0], [0], 1)
    many = cls.enq_tab([1], [0], [0], cls.ENQ_DST_MAX + 1)
    q = [5]
    no_ctx = -errno.ENODEV if L.mi_cls_device_count() <= 0 else -errno.EINVAL
    ok = dict(out=out.ctypes.data, data_from_meta=192, arena_lo=4096, arena_bytes=4096)
    cases = [((None, q, ok), -errno.EINVAL),
             ((good, None, ok), -errno.EINVAL),
             ((many, q, ok), -errno.E2BIG),
             ((good, q, dict(ok, data_from_meta=200)), -errno.EINVAL),
             ((good, q, dict(ok, data_from_meta=48)), -errno.EINVAL),
             ((good, q, dict(ok, n=1 << 28)), -errno.EINVAL),
             ((good, q, dict(ok, pkts_bytes=1 << 32)), -errno.EINVAL),
             ((good, q, dict(ok, arena_lo=(1 << 64) - 64, arena_bytes=128)), -errno.EINVAL),
             ((good, q, dict(ok, ngot=3)), -errno.EINVAL),
             ((good, q, ok), no_ctx),
             ((good, q, dict(ok, pkts_bytes=(1 << 32) - 1, n=(1 << 28) - 1)), no_ctx)]
    t = C.c_uint64(99)
    for (tab, dq, kw), rc in cases:
        a = cls.move_args(tab, dq, **kw)
        assert L.mi_cls_pool_move(None, C.byref(a), None) == rc
        assert L.mi_cls_pool_move_host(None, C.byref(a)) == rc
        t.value = 99
        assert L.mi_cls_pool_move_host_submit(None, C.byref(a), C.byref(t)) == rc and t.value == 0
    assert L.mi_cls_pool_move(None, None, None) == -errno.EINVAL
    assert L.mi_cls_pool_move_host_submit(None, C.byref(cls.move_args(good, q, **ok)), None) == -errno.EINVAL
    assert L.mi_cls_pool_move_host_wait(None, 1) == no_ctx
    assert not out.any()


def test_pktio_entries(built):
    """The pktio forms create the context on first use: -ENODEV without a GPU;
    with one, an empty batch's out is all zeros.  The geometry is the
    runtime's: -ENOENT while no pool is page-locked."""
    from odp_amd import cls
    have = cls.lib().mi_cls_device_count() > 0
    c = cls.Classifier(gpu=0)
    try:
        c.apply([R.cos("a", queue=11), ("default", 0)])
        tab, queues, _ = c.enq_table()
        rc, meta_off, dfm, lo, nb = c.pool_move_geom()
        assert rc in (0, -errno.ENOENT) and meta_off % 64 == 0 and dfm % 16 == 0 and dfm >= 64
        assert (rc == 0) == (nb != 0)
        for submit in (False, True):
            out = np.full(4, 7, np.uint64)
            a = cls.move_args(tab, queues, out=out.ctypes.data, data_from_meta=dfm, arena_lo=lo, arena_bytes=nb)
            rc = c.pool_move_host(a, submit=submit)
            assert rc == (0 if have else -errno.ENODEV)
            assert not out.any() if have else (out == 7).all()
    finally:
        c.close()
