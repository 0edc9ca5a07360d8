"""The receive delivery and receive-chain kernels (odp_amd/csrc/mi_cls_kd.hip:
mi_cls_deliver_kernel with dlv_group, mi_cls_rx_decide_kernel,
mi_cls_rx_deliver_kernel, mi_cls_rx_stage_kernel) called directly through
mi_cls_deliver_submit / mi_cls_rx_chain_submit and compared, bit for bit, with
the CPU model tests/rx_model.py (pinned to the reference-derived expectation
by tests/test_rx_model_cpu.py).

Every run works inside one page-locked arena (tests/rx_harness.py) filled
with a seeded non-zero pattern; after the wait the whole arena -- every output
array, every packet delivered or not, every gap -- must equal the image before
the submit with the model's outputs written in.  Only the bytes between a
copied frame's end and its 16-byte rounding are left open (rx_model.copy_extent).
"""
import numpy as np
import pytest

from odp_amd import cls
from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import rt_helpers as H
from tests import rx_harness as X
from tests import rx_model as M
from tests import zoo

pytestmark = pytest.mark.gpu

INPUT = 0xA1B2C3D4E5F60718
ARENA_BYTES = 80 << 20
FRAME_CAP = 1856       # rt_helpers.pcap_frames


# ------------------------------------------------------------------ fixtures
def chain_program():
    """zoo.prog_everything() with two 32-queue hash CoS in front of its rules
    (UDP / TCP to port 7777), so that a burst can use 64 queue groups."""
    p = zoo.prog_everything()
    at = next(i for i, op in enumerate(p) if op[0] == "pmr")
    ncos = sum(1 for op in p if op[0] == "cos")
    extra = [R.cos("h32u", num_queue=32, hash_proto=R.HP_IPV4_UDP),
             R.cos("h32t", num_queue=32, hash_proto=R.HP_IPV4_TCP),
             ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 7777)], 0, ncos, 0),
             ("pmr", [R.t_be16(R.PMR_TCP_DPORT, 7777)], 0, ncos + 1, 0x77)]
    return p[:at] + extra + p[at:]


def chain_frames():
    """Zoo frames, mutated ones and 600 UDP / TCP flows to port 7777, shuffled."""
    rng = np.random.default_rng(20)
    base = [f for _, f in zoo.all_frames()]
    fr = base + zoo.mutate_frames(rng, base, 300)
    for i in range(600):
        src = f"172.{16 + i % 8}.{int(rng.integers(0, 256))}.{int(rng.integers(1, 255))}"
        mk = pg.udp4_frame if i % 2 else pg.tcp4_frame
        fr.append(mk(src=src, dst="192.0.2.9", sport=int(rng.integers(1024, 65536)), dport=7777,
                     size=70 + i % 5))
    fr = H.pcap_frames(fr)
    return [fr[int(i)] for i in rng.permutation(len(fr))]


class World:
    """The rule program loaded on a device context, the frames and the
    oracle's records of every frame."""

    def __init__(self):
        self.prog = chain_program()
        self.frames = chain_frames()
        k = cls.Classifier(gpu=0)
        try:
            k.apply(self.prog)
            blob = k.compile()
        finally:
            k.close()
        self.ctx = X.Context(blob)
        self.host_side()

    def host_side(self):
        self.slots = H.cos_names(self.prog)
        self.enq_cos = [i for i, (_, a) in sorted(self.slots.items()) if a["action"] == 0]
        # the enqueue CoS by the frames they receive, busiest first
        cnt = {i: 0 for i in self.enq_cos}
        for r in self.records(self.frames):
            if int(r["outcome"]) == R.OUT_ENQ:
                cnt[int(r["cos"])] += 1
        self.by_traffic = sorted(self.enq_cos, key=lambda i: (-cnt[i], i))

    def burst(self, n, start=0):
        m = len(self.frames)
        return [self.frames[(start + i) % m] for i in range(n)]

    def records(self, frames):
        from oracle.oracle import Oracle
        o = Oracle()      # the oracle's tables are process-wide: set up per call
        o.apply(self.prog)
        return o.classify(pg.batch_from_frames(frames))


@pytest.fixture(scope="module")
def world(built, gpu):
    w = World()
    yield w
    w.ctx.close()


@pytest.fixture(scope="module")
def arena(built, gpu):
    a = X.Arena(ARENA_BYTES)
    yield a
    a.close()


# ------------------------------------------------- mi_cls_deliver_submit runs
def synthetic_records(rng, m):
    """Records with random fields; a third have every bit of in_flags, err and
    l4_offset set (they pin the parser-layer masks bit for bit)."""
    r = np.zeros(m, M.RESULT_DTYPE)
    r["in_flags"] = rng.integers(0, 1 << 32, m, dtype=np.uint64)
    r["err"] = rng.integers(0, 256, m)
    r["outcome"] = 0
    r["cos"] = rng.integers(0, 256, m)
    r["hops"] = rng.integers(0, 256, m)
    r["queue"] = rng.integers(0, 32, m)
    r["mark"] = rng.integers(0, 65536, m)
    r["l3_offset"] = rng.integers(0, 65536, m)
    r["l4_offset"] = rng.integers(0, 65536, m)
    full = np.arange(m) % 3 == 0
    r["in_flags"][full], r["err"][full], r["l4_offset"][full] = 0xFFFFFFFF, 0xFF, 0xFFFF
    return r


def run_deliver(ctx, A, res, ent, layer, src, pkt_cap, seed, expect=0):
    """One mi_cls_deliver_submit over entries `ent` (DLV_DTYPE; meta is set
    here: one packet per entry) whose frames lie in `src`; compares the arena
    with the model.  expect: the errno the host must refuse with."""
    n = len(ent)
    assert n == 0 or (int(ent["rec"].max()) < len(res) and int(ent["len"].max()) <= pkt_cap)
    assert n == 0 or int((ent["src"].astype(np.int64) + ent["len"]).max()) <= len(src)
    A.reset()
    base = A.alloc("frames", len(src) + 16)
    res_off, res_v = A.array("res", M.RESULT_DTYPE, len(res))
    dlv_off, dlv_v = A.array("dlv", M.DLV_DTYPE, max(1, n))
    perm_off, perm_v = A.array("perm", "<u4", max(1, n))
    gcnt_off, gcnt_v = A.array("gcnt", "<u4", M.DLV_GROUPS)
    pk, _ = A.packets("packet", max(1, n), pkt_cap)
    A.fill(seed)
    A.u8[base: base + len(src)] = src
    res_v[:] = res
    A.init_packets(pk, 3)
    ent = ent.copy()
    ent["meta"] = A.ptr + pk[:n] + X.META_OFF
    dlv_v[:n] = ent
    before = A.snapshot()
    args = X.DlvArgs(base=A.ptr + base, res=A.ptr + res_off, dlv=A.ptr + dlv_off, n=n, layer=layer,
                     input=INPUT, headroom=X.HEADROOM, data_from_meta=X.DATA_FROM_META,
                     perm=A.ptr + perm_off, gcnt=A.ptr + gcnt_off)
    rc, ticket = ctx.deliver_submit(args)
    if expect or n == 0:
        assert rc == -expect and ticket == 0
        assert np.array_equal(A.snapshot(), before), "a refused delivery wrote something"
        return None
    assert rc == 0 and ticket != 0
    assert ctx.wait(ticket) == 0
    got = A.snapshot()
    m = M.deliver(res, ent, layer, INPUT, X.HEADROOM, [A.meta(o, before) for o in pk[:n]])
    exp, care = before.copy(), np.ones(len(before), np.uint8)
    for j in range(n):
        e = ent[j]
        fr = src[int(e["src"]): int(e["src"]) + int(e["len"])] if int(e["flags"]) & M.DLV_COPY else None
        X.put_packet(A, exp, care, pk[j], m.lines[j], fr)
    exp[perm_off: perm_off + 4 * len(m.perm)] = m.perm.view(np.uint8)
    exp[gcnt_off: gcnt_off + 256] = m.gcnt.view(np.uint8)

    def describe(name, idx):
        if name in ("packet", "dlv") and idx < n:
            return f"entry {idx}: {ent[idx]} record {res[int(ent[idx]['rec'])]}"
        return ""
    X.compare(A, got, exp, care, describe)
    return m


def synthetic_entries(rng, n, m, qid, lens=None):
    """n entries over m records: every flag combination (all eight inside the
    first 16-packet block), records that are not the identity, unaligned
    sources, mostly 60-byte frames."""
    ent = np.zeros(n, M.DLV_DTYPE)
    ent["flags"] = rng.integers(0, 8, n)
    ent["flags"][: min(n, 16)] = (np.arange(min(n, 16)) * 3) % 8
    ent["rec"] = rng.integers(0, m, n)
    ent["qid"] = qid
    if lens is None:
        lens = np.where(rng.random(n) < 0.85, 60, rng.integers(1, 258, n))
    ent["len"] = lens
    ent["dst_queue"] = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    ent["user_ptr"] = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    ent["data_off"] = rng.integers(0, 256, n)
    ent["rsv"] = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    off, at = np.zeros(n, np.int64), 1
    for j in range(n):
        off[j] = at
        at += int(ent["len"][j]) + 1 + (j % 7)
    ent["src"] = off
    src = rng.integers(1, 256, at + 16, dtype=np.uint8)
    return ent, src


def mixed_qid(rng, n):
    q = rng.integers(0, M.DLV_GROUPS, n)
    q[rng.random(n) < 0.2] = 0xFF
    return q


@pytest.mark.parametrize("n,layer", [(1, 4), (15, 1), (16, 2), (17, 3), (255, 4), (256, 1), (257, 2),
                                     (257, 1), (257, 3), (257, 4), (4097, 3), (8192, 2)])
def test_deliver_sizes_and_layers(world, arena, n, layer):
    rng = np.random.default_rng(1000 + n + layer)
    res = synthetic_records(rng, n + 3)
    ent, src = synthetic_entries(rng, n, len(res), mixed_qid(rng, n))
    run_deliver(world.ctx, arena, res, ent, layer, src, 320, seed=n)


def _qid_case(rng, name, n):
    i = np.arange(n)
    if name == "one_group":
        return np.full(n, 37)
    if name == "round_robin_64":
        return i % 64
    if name == "random_with_none":
        return mixed_qid(rng, n)
    if name == "one_wave_of_one_chunk":      # group 7: entries 3*256+64 .. +127 only
        q = 8 + rng.integers(0, 56, n)
        q[3 * 256 + 64: 3 * 256 + 128] = 7
        return q
    if name == "every_chunk":                 # group 9: one entry of every 256-entry chunk
        q = 10 + rng.integers(0, 54, n)
        q[i % 256 == 5] = 9
        return q
    raise ValueError(name)


@pytest.mark.parametrize("dist", ["one_group", "round_robin_64", "random_with_none",
                                  "one_wave_of_one_chunk", "every_chunk"])
def test_deliver_group_distributions(world, arena, dist):
    n = 2003
    rng = np.random.default_rng(77)
    res = synthetic_records(rng, 64)
    ent, src = synthetic_entries(rng, n, len(res), _qid_case(rng, dist, n))
    m = run_deliver(world.ctx, arena, res, ent, 4, src, 320, seed=5)
    assert len(m.perm) == int((ent["qid"] < 64).sum())


def test_deliver_copy_lengths(world, arena):
    lens = np.array([1, 15, 16, 17, 255, 256, 257, 1535, 1536, 1537, 3073, 9000, 65535])
    rng = np.random.default_rng(9)
    res = synthetic_records(rng, 8)
    ent, src = synthetic_entries(rng, len(lens), len(res), np.arange(len(lens)) % 3, lens)
    ent["flags"] |= M.DLV_COPY
    assert any(int(s) % 16 for s in ent["src"])
    run_deliver(world.ctx, arena, res, ent, 4, src, 65536, seed=6)


def test_deliver_above_group_max(world, arena):
    n = M.DLV_GROUP_MAX + 1
    rng = np.random.default_rng(11)
    res = synthetic_records(rng, 16)
    ent, src = synthetic_entries(rng, n, len(res), np.full(n, 0xFF))
    m = run_deliver(world.ctx, arena, res, ent, 4, src, 320, seed=7)
    assert len(m.perm) == 0 and not m.gcnt.any()
    ent["qid"][n - 1] = 3
    run_deliver(world.ctx, arena, res, ent, 4, src, 320, seed=8, expect=X.E2BIG)


def test_deliver_empty(world, arena):
    rng = np.random.default_rng(12)
    res = synthetic_records(rng, 4)
    run_deliver(world.ctx, arena, res, np.zeros(0, M.DLV_DTYPE), 4, np.zeros(64, np.uint8), 320,
                seed=9)


# ------------------------------------------------ mi_cls_rx_chain_submit runs
def hand_table(world, case):
    """Hand-built tables over the program's enqueue CoS: a one pool and one
    queue group; b 16 pool slots with capacities that split the traffic; c 64
    queue groups; d a group shared by two CoS next to single-CoS groups (CoS
    index 0 among them); e no grouping."""
    tab = np.zeros((), M.RXTAB_DTYPE)
    tab["flags"] = M.RXT_CLS | (0 if case == "e" else M.RXT_GROUP)
    tab["pool_cap"][:] = FRAME_CAP
    tab["npool"] = 16 if case == "b" else 1
    tab["stamp"] = 1 + "abcde".index(case)
    qe = 0
    for idx in world.enq_cos:
        name, a = world.slots[idx]
        # b: the 16 busiest CoS each have a slot of their own
        tab["cos_pool"][idx] = world.by_traffic.index(idx) % 16 if case == "b" else 0
        tab["cos_nq"][idx], tab["cos_q0"][idx] = a["num_queue"], qe
        for s in range(a["num_queue"]):
            tab["qh"][qe] = 0x5000_0000_0000 + 0x100 * qe
            if case == "a":
                g = 0
            elif case == "c":     # the two 32-queue hash CoS: a group per queue
                g = s + (32 if name == "h32t" else 0) if name in ("h32u", "h32t") else qe % 64
            elif case == "d":     # CoS 0 alone in group 5; "err" and "hashq4" share group 6
                g = 5 if idx == 0 else 6 if name in ("err", "hashq4") else 8 + qe % 56
            else:
                g = qe % 64
            tab["qg"][qe] = g
            qe += 1
    if case == "b":               # capacities that split the traffic
        tab["pool_cap"][1:8:2] = 80
    return tab


_stamp = iter(range(1000, 1 << 30))


def restamp(tab):
    """A table written into table memory gets a stamp no earlier table had:
    the device keeps a copy per stamp (mi_cls_rxtab_t.stamp)."""
    tab["stamp"] = next(_stamp)
    return tab


class Burst:
    """One receive-chain burst laid out in an arena (pcap form: the frames
    packed in a region; loop form: each frame in its own packet)."""

    def __init__(self, A, world, frames, tab_off, tag="", loop=None, extra=2, cap=FRAME_CAP):
        self.A, self.world, self.frames, self.tab_off, self.loop = A, world, frames, tab_off, loop
        n = self.n = len(frames)
        self.lens = np.array([len(f) for f in frames], np.int64)
        assert self.lens.max() <= cap
        t = tag
        self.soff_off, self.soff = A.array(t + "soff", "<u4", n)
        self.slen_off, self.slen = A.array(t + "slen", "<u2", n)
        self.res_off, self.res = A.array(t + "res", M.RESULT_DTYPE, n)
        self.dec_off, self.dec = A.array(t + "dec", "<u4", n)
        self.ent_off, self.ent = A.array(t + "ent", "<u8", n)
        self.perm_off, self.perm = A.array(t + "perm", "<u4", n)
        self.gcnt_off, self.gcnt = A.array(t + "gcnt", "<u4", M.DLV_GROUPS)
        self.out_off, self.out = A.array(t + "out", M.RXOUT_DTYPE, 1)
        self.extra, self.cap = extra, cap
        if loop is None:
            self.off = np.zeros(n, np.int64)
            at = 3
            for i in range(n):
                self.off[i] = at
                at += int(self.lens[i]) + i % 3
            self.frames_off = A.alloc(t + "frames", at + 16)
            self.base_off = 0
        else:
            # loop["outside"]: frames whose packets lie below the burst's base
            self.pk_off, self.pk = A.array(t + "pk", "<u8", n)
            self.ppool_off, self.ppool = A.array(t + "ppool", "u1", n)
            self.pdoff_off, self.pdoff = A.array(t + "pdoff", "<u2", n)
            below = sorted(loop.get("outside", ()))
            lo, _ = A.packets(t + "own_below", max(1, len(below)), cap)
            own, size = A.packets(t + "own", n, cap)
            self.own = own.copy()
            for j, i in enumerate(below):
                self.own[i] = lo[j]
            self.base_off = int(own[0])
            self.own_end = int(own[-1]) + size
        self.got_need = None

    def take_packets(self, have):
        """The fresh packets of every slot: have[k] + extra handles each."""
        A, t = self.A, ""
        self.have = [int(h) for h in have]
        cnt = [h + self.extra for h in self.have]
        self.got_base = [int(x) for x in np.concatenate([[0], np.cumsum(cnt)[:-1]])]
        self.got_off, self.got = A.array("got", "<u8", sum(cnt))
        self.fresh, _ = A.packets("fresh", sum(cnt), self.cap)

    def write_inputs(self, tab, stage=0):
        A = self.A
        n = self.n
        if self.loop is None:
            for i, f in enumerate(self.frames):
                o = self.frames_off + int(self.off[i])
                A.u8[o: o + len(f)] = np.frombuffer(f, np.uint8)
            self.soff[:] = self.frames_off + self.off - self.base_off
            self.slen[:] = self.lens
        else:
            rp = self.loop["pools"]
            for i, f in enumerate(self.frames):
                o = int(self.own[i])
                A.init_packets([o], rp[i])
                m = A.meta(o)
                m["data_off"] = X.HEADROOM - 2 * (i % 5)
                m["len"] = len(f)
                d = o + X.META_OFF + 64 + int(m["data_off"])
                A.u8[d: d + len(f)] = np.frombuffer(f, np.uint8)
                self.pk[i] = A.ptr + o
                if not stage:
                    self.soff[i], self.slen[i] = d - self.base_off, len(f)
                    self.ppool[i] = rp[i] + 1
                self.pdoff[i] = int(m["data_off"])
        A.init_packets(self.fresh, 40)
        self.got[:] = A.ptr + self.fresh
        A.u8[self.tab_off: self.tab_off + M.RXTAB_DTYPE.itemsize] = np.frombuffer(
            restamp(tab).tobytes(), np.uint8)

    def args(self, stage=0, nbytes=None):
        A = self.A
        a = X.RxcArgs(base=A.ptr + self.base_off, soff=A.ptr + self.soff_off,
                      slen=A.ptr + self.slen_off, res=A.ptr + self.res_off, n=self.n, layer=4,
                      input=INPUT, headroom=X.HEADROOM, data_from_meta=X.DATA_FROM_META,
                      tab=A.ptr + self.tab_off, got=A.ptr + self.got_off, meta_off=X.META_OFF,
                      stage=stage, head_off=X.HEAD_OFF, pool_off=X.POOL_OFF,
                      dec=A.ptr + self.dec_off, ent=A.ptr + self.ent_off,
                      perm=A.ptr + self.perm_off, gcnt=A.ptr + self.gcnt_off,
                      out=A.ptr + self.out_off)
        for k in range(M.RX_POOLS):
            a.got_base[k], a.have[k] = self.got_base[k], self.have[k]
        # the device dereferences every handle: all of them arena memory
        for h in (self.got,) + ((self.pk,) if self.loop is not None else ()):
            assert ((h >= A.ptr) & (h < A.ptr + A.top)).all()
        if self.loop is not None:
            a.pk, a.ppool, a.pdoff = (A.ptr + self.pk_off, A.ptr + self.ppool_off,
                                      A.ptr + self.pdoff_off)
        self.nbytes = A.nbytes - self.base_off if nbytes is None else nbytes
        return a

    def model(self, tab, before, stage=0):
        """The model's outputs for this burst under `tab`, from the arena
        image before the submit."""
        A, n = self.A, self.n
        st = None
        frames, lens = self.frames, self.lens
        pk = ppool = None
        if self.loop is not None:
            pk = [A.ptr + int(o) for o in self.own]
            if stage:
                hd = []
                for o in self.own:
                    o = int(o)
                    m = A.meta(o, before)
                    hd.append((int(before[o + X.HEAD_OFF: o + X.HEAD_OFF + 8].view("<u8")[0]),
                               int(before[o + X.POOL_OFF: o + X.POOL_OFF + 2].view("<u2")[0]),
                               int(m["data_off"]), int(m["len"])))
                st = M.stage(hd, A.ptr + self.base_off, self.nbytes, tab["rt_pinned"])
                frames = [f if st.slen[i] or not len(f) else b"" for i, f in enumerate(frames)]
                lens = st.slen.astype(np.int64)
                ppool = st.ppool
            else:
                ppool = [p + 1 for p in self.loop["pools"]]
        recs = self.world.records(frames)
        d = M.decide(recs, lens, tab, self.have, self.got_base, self.got.copy(), pk, ppool)
        d.recs, d.stage, d.frames, d.lens = recs, st, frames, lens
        return d

    def expect(self, exp, care, d, before):
        """Write the model's outputs of this burst into the expected image."""
        A, n = self.A, self.n

        def put(off, arr):
            b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            exp[off: off + len(b)] = b
        put(self.dec_off, d.dec)
        put(self.ent_off, d.ent)
        put(self.res_off, d.recs)
        if d.grouped:
            put(self.perm_off, d.perm)
            put(self.gcnt_off, d.gcnt)
        o = np.frombuffer(exp[self.out_off: self.out_off + M.RXOUT_DTYPE.itemsize].tobytes(),
                          M.RXOUT_DTYPE).copy()
        for f in ("in_errors", "in_discards", "packets", "octets", "short_pool"):
            o[f] = getattr(d.out, f)
        o["used"], o["need"] = d.out.used, d.out.need
        if d.stage is not None:
            put(self.soff_off, d.stage.soff)
            put(self.slen_off, d.stage.slen)
            put(self.ppool_off, d.stage.ppool)
            if d.stage.not_in_place:
                o["not_in_place"] = 1
        put(self.out_off, o)
        for i in range(n):
            if not d.delivered[i]:
                continue
            fate = int(d.dec[i]) & 3
            pkt = int(d.ent[i]) - A.ptr
            own = A.meta(self.own[i], before) if self.loop is not None else None
            line = M.chain_meta(d, i, d.recs[i], int(d.lens[i]), X.HEADROOM, INPUT,
                                A.meta(pkt, before), own)
            fr = np.frombuffer(d.frames[i], np.uint8) if fate == M.RXF_FRESH else None
            X.put_packet(A, exp, care, pkt, line, fr)

    def describe(self, d, got):
        def f(name, idx):
            i = None
            if name.endswith(("dec", "ent", "res", "soff", "slen", "ppool")) and idx < self.n:
                i = idx
            elif name in ("fresh", "own"):
                size = X.META_OFF + X.DATA_FROM_META + ((self.cap + 63) & ~63) + X.TAIL
                base = self.fresh[0] if name == "fresh" else self.own[0]
                h = self.A.ptr + int(base) + idx * size
                hit = np.nonzero(d.ent == np.uint64(h))[0]
                i = int(hit[0]) if len(hit) else None
            if i is None:
                return ""
            gd = int(got[self.dec_off + 4 * i: self.dec_off + 4 * i + 4].view("<u4")[0])
            return (f"frame {i} len {int(d.lens[i])} record {d.recs[i]} dec model "
                    f"{int(d.dec[i]):#010x} device {gd:#010x}")
        return f


def needs_of(world, frames, tab, pk=None, ppool=None):
    """Fresh packets each slot's frames want (the model with plenty)."""
    recs = world.records(frames)
    lens = [len(f) for f in frames]
    n = len(frames)
    d = M.decide(recs, lens, tab, [n] * 16, [k * n for k in range(16)],
                 np.ones(16 * n, np.uint64), pk, ppool)
    return d.out.need, d


def run_chain(world, A, frames, tab, have_of=lambda need: [x + 5 for x in need], seed=1, loop=None,
              stage=0, nbytes_of=None, keep=False):
    """One chain burst compared with the model; returns (model, arena image)."""
    pk = ppool = None
    if loop is not None:
        pk, ppool = np.ones(len(frames), np.uint64), [p + 1 for p in loop["pools"]]
    need, _ = needs_of(world, frames, tab, pk, ppool)
    A.reset()
    tab_off = A.alloc("tab", M.RXTAB_DTYPE.itemsize)
    b = Burst(A, world, frames, tab_off, loop=loop)
    b.take_packets(have_of(need))
    A.fill(seed)
    b.write_inputs(tab, stage)
    a = b.args(stage, nbytes_of(b) if nbytes_of else None)
    before = A.snapshot()
    d = b.model(tab, before, stage)
    rc, ticket = world.ctx.chain_submit(A.ptr + b.base_off, b.nbytes, a)
    assert rc == 0 and ticket != 0, rc
    assert world.ctx.wait(ticket) == 0
    got = A.snapshot()
    exp, care = before.copy(), np.ones(len(before), np.uint8)
    b.expect(exp, care, d, before)
    X.compare(A, got, exp, care, b.describe(d, got))
    d.burst = b
    return d, got


CHAIN_N = [1, 63, 64, 65, 1023, 1024, 1025, 2049, 8191, 8192]


@pytest.mark.parametrize("n,case", [(n, "abcde"[i % 5]) for i, n in enumerate(CHAIN_N)] +
                         [(2049, c) for c in "abde"] + [(8192, "b"), (1025, "c")])
def test_chain_pcap_tables_and_sizes(world, arena, n, case):
    tab = hand_table(world, case)
    d, _ = run_chain(world, arena, world.burst(n, start=n), tab, seed=n)
    fates = set(int(x) & 3 for x in d.dec)
    if n >= 1023:
        assert fates >= {M.RXF_DROP, M.RXF_FRESH}
        assert case != "b" or M.RXF_DISCARD in fates
        cnt = d.gcnt & 0xFFFF
        if case == "a":
            assert (cnt != 0).sum() == 1 and not (int(d.gcnt[0]) >> 24) & 1
        if case == "b":
            assert all(x > 0 for x in d.out.need), d.out.need
        if case == "c":
            assert (cnt != 0).all()
        if case == "d":
            assert int(d.gcnt[5]) >> 16 == 0x100 and cnt[5]       # single CoS, index 0
            assert int(d.gcnt[6]) >> 16 == 0 and cnt[6]           # two CoS
            assert any((int(g) >> 24) & 1 and (int(g) >> 16) & 0xFF for g in d.gcnt)
        if case == "e":
            assert all((int(x) >> 8) & 0x7F == M.NO_GROUP for x in d.dec)


def test_chain_pool_capacity_edge(world, arena):
    """len == pool_cap[k] is delivered, len == pool_cap[k] + 1 discarded."""
    tab = hand_table(world, "b")
    frames = world.burst(3000)
    recs = world.records(frames)
    # a slot that receives frames of some length L and of L + 1
    by = {}
    for r, f in zip(recs, frames):
        if int(r["outcome"]) == R.OUT_ENQ:
            by.setdefault(int(tab["cos_pool"][int(r["cos"])]), set()).add(len(f))
    k, cap = next((k, ln) for k, s in sorted(by.items()) for ln in sorted(s) if ln + 1 in s)
    tab["pool_cap"][k] = cap
    d, _ = run_chain(world, arena, frames, tab, seed=31)
    at_cap = [i for i in range(len(frames)) if (int(d.dec[i]) >> 2) & 31 == k and
              int(recs[i]["outcome"]) == R.OUT_ENQ and len(frames[i]) in (cap, cap + 1)]
    assert {len(frames[i]) for i in at_cap} == {cap, cap + 1}
    for i in at_cap:
        assert int(d.dec[i]) & 3 == (M.RXF_FRESH if len(frames[i]) == cap else M.RXF_DISCARD)


@pytest.mark.parametrize("short", ["need", "need-1", "0"])
def test_chain_pool_shortage(world, arena, short):
    tab = hand_table(world, "b")
    frames = world.burst(1025, start=100)
    need, _ = needs_of(world, frames, tab)
    k = int(np.argmax(need))
    assert need[k] > 2

    def have_of(nd):
        h = [x + 5 for x in nd]
        h[k] = {"need": nd[k], "need-1": nd[k] - 1, "0": 0}[short]
        return h
    d, _ = run_chain(world, arena, frames, tab, have_of, seed=41)
    assert d.out.short_pool == (0 if short == "need" else 1)
    assert d.out.used[k] == have_of(need)[k] and d.out.need == need
    und = [i for i in range(len(frames)) if int(d.dec[i]) & 3 == M.RXF_FRESH and not d.ent[i]]
    assert len(und) == need[k] - have_of(need)[k]
    for i in und:
        assert (int(d.dec[i]) >> 2) & 31 == k and (int(d.dec[i]) >> 8) & 0x7F == M.NO_GROUP
        assert int(d.dec[i]) >> 16 >= have_of(need)[k]
    if short == "need-1":      # the rank exactly at have[k]
        assert [int(d.dec[i]) >> 16 for i in und] == [need[k] - 1]


def test_chain_refusals(world, arena):
    tab = hand_table(world, "a")
    frames = world.burst(64)
    A = arena
    A.reset()
    tab_off = A.alloc("tab", M.RXTAB_DTYPE.itemsize)
    b = Burst(A, world, frames, tab_off)
    b.take_packets([64] * 16)
    A.fill(51)
    b.write_inputs(tab)
    before = A.snapshot()
    a = b.args()
    a.n = M.DLV_GROUP_MAX + 1
    assert world.ctx.chain_submit(A.ptr, A.nbytes, a) == (-X.EINVAL, 0)
    a = b.args()
    assert world.ctx.chain_submit(A.ptr + 64, A.nbytes - 64, a) == (-X.EINVAL, 0)
    a = b.args()
    a.n = 0
    assert world.ctx.chain_submit(A.ptr, A.nbytes, a) == (0, 0)
    assert np.array_equal(A.snapshot(), before)


# ------------------------------------------------------- loop form and stage
def loop_setup(world, n, seed):
    """Runtime pools 2, 3, 4 hold the frames' packets; pool 2 is slot 0 and
    pool 3 slot 1 (a frame whose CoS uses its packet's slot is received in
    place), pool 4 has no slot (every frame of it switches pool)."""
    tab = hand_table(world, "d")
    tab["npool"] = 3
    for idx in world.enq_cos:
        tab["cos_pool"][idx] = idx % 3
    tab["rt_slot"][2], tab["rt_slot"][3] = 1, 2
    tab["rt_pinned"][[2, 3, 4, 40]] = 1
    rng = np.random.default_rng(seed)
    pools = [int(x) for x in rng.integers(2, 5, n)]
    return tab, {"pools": pools}


@pytest.mark.parametrize("n", [65, 1025, 2049])
def test_chain_loop_in_place_and_pool_switch(world, arena, n):
    tab, loop = loop_setup(world, n, n)
    frames = world.burst(n, start=7)
    d0, got0 = run_chain(world, arena, frames, tab, seed=61, loop=loop, stage=0)
    fates = [int(x) & 3 for x in d0.dec]
    assert fates.count(M.RXF_INPLACE) > n // 8 and fates.count(M.RXF_FRESH) > n // 8
    d1, got1 = run_chain(world, arena, frames, tab, seed=61, loop=loop, stage=1)
    assert d1.stage.not_in_place == 0
    b = d1.burst
    assert np.array_equal(d1.stage.soff, np.frombuffer(
        got0[b.soff_off: b.soff_off + 4 * n].tobytes(), "<u4"))
    # everything downstream of the descriptors is the stage = 0 run's (the
    # table memory, first in the arena, differs by its stamp)
    ts = M.RXTAB_DTYPE.itemsize
    assert b.tab_off == 0 and np.array_equal(got0[ts:], got1[ts:])


def test_chain_stage_not_in_place(world, arena):
    n = 300
    tab, loop = loop_setup(world, n, 5)
    frames = world.burst(n, start=11)
    unpinned, below, edge = 17, 123, n - 1
    loop["pools"][unpinned] = 5          # a pool that is not page-locked
    loop["outside"] = [below]            # its data lies below the burst's base

    def nbytes_of(b):
        # the batch ends 8 bytes behind the last packet's frame: its data
        # ends within the last 16 bytes
        o = int(b.own[edge])
        return o + X.META_OFF + 64 + (X.HEADROOM - 2 * (edge % 5)) + len(frames[edge]) + 8 - b.base_off
    assert len(frames[unpinned]) and len(frames[below]) and len(frames[edge])
    d, _ = run_chain(world, arena, frames, tab, seed=71, loop=loop, stage=1, nbytes_of=nbytes_of)
    assert d.stage.not_in_place == 1
    empty = [i for i in range(n) if d.stage.slen[i] == 0 and d.stage.soff[i] == 0]
    assert empty == sorted([unpinned, below, edge])


# ---------------------------------------------------------------- pipelining
def test_chain_pipelined_bursts_and_table_switch(world, arena):
    """Ten bursts submitted back to back (the ring of 8 wraps), alternating
    between two tables written into the same table memory; then the first
    burst again."""
    A = arena
    tabs = [hand_table(world, "b"), hand_table(world, "d")]
    A.reset()
    tab_off = A.alloc("tab", M.RXTAB_DTYPE.itemsize)
    bursts = []
    for j in range(10):
        fr = world.burst(300 + j, start=97 * j)
        need, _ = needs_of(world, fr, tabs[j % 2])
        b = Burst(A, world, fr, tab_off, tag=f"b{j}.", cap=FRAME_CAP)
        b.take_packets([x + 1 for x in need])
        bursts.append(b)
    A.fill(81)
    for j, b in enumerate(bursts):
        b.write_inputs(tabs[j % 2])
    args = [b.args() for b in bursts]
    before = A.snapshot()
    tickets = []
    for j, b in enumerate(bursts):
        t = restamp(tabs[j % 2].copy())
        A.u8[tab_off: tab_off + t.itemsize] = np.frombuffer(t.tobytes(), np.uint8)
        rc, ticket = world.ctx.chain_submit(A.ptr, A.nbytes, args[j])
        assert rc == 0 and ticket
        tickets.append(ticket)
    assert tickets == list(range(tickets[0], tickets[0] + 10))
    for t in tickets:
        assert world.ctx.wait(t) == 0
    got = A.snapshot()
    exp, care = before.copy(), np.ones(len(before), np.uint8)
    exp[tab_off: tab_off + M.RXTAB_DTYPE.itemsize] = got[tab_off: tab_off + M.RXTAB_DTYPE.itemsize]
    describes = {}
    for j, b in enumerate(bursts):
        d = b.model(tabs[j % 2], before)
        b.expect(exp, care, d, before)
        describes[f"b{j}."] = b.describe(d, got)

    def describe(name, idx):
        return describes[name[:3]](name, idx) if name[:3] in describes else ""
    X.compare(A, got, exp, care, describe)
    # the first burst again, under its table
    t = restamp(tabs[0].copy())
    A.u8[tab_off: tab_off + t.itemsize] = np.frombuffer(t.tobytes(), np.uint8)
    rc, ticket = world.ctx.chain_submit(A.ptr, A.nbytes, args[0])
    assert rc == 0 and world.ctx.wait(ticket) == 0
    again = A.snapshot()
    again[tab_off: tab_off + t.itemsize] = got[tab_off: tab_off + t.itemsize]
    differ = np.nonzero((again != got) & (care != 0))[0]
    assert not len(differ), A.where(int(differ[0]))
