"""CPU model of the pool plan (mi_cls_pool_plan, include/mi_cls.h).

plan_pools() is the per-record loop that transcribes the header's rule: each
record's fate (NONE, INPLACE, TOO_LONG, then FRESH or SHORT by its rank among
the earlier ranked records of its slot), dec, idx, res_out and out.
plan_pools_np() states the same with numpy; tests/test_pool_plan_cpu.py holds
the two equal on random records, and the GPU tests use the numpy form where a
Python loop per record would take seconds.

reference_loop() is something else: a direct per-packet statement of the
reference's receive loop with the pool switch in it (pktio/loop.c:319-337,
_odp_pktio_packet_to_pool, include/odp_packet_io_internal.h:352-371), which
keeps a free count per pool and knows nothing of ranks or plans.  The tests
hold the composition pool plan -> enqueue plan equal to it.

A pool table is the tuple (cos_slot[256], slot_cap[16], nslot) of
mi_cls_pool_tab_t; an enqueue table enq_model's tuple.
"""
import numpy as np

from tests import enq_model as M

SLOTS = 16
PF_NONE, PF_INPLACE, PF_FRESH, PF_TOO_LONG, PF_SHORT = 0, 1, 2, 3, 4
NO_IDX = 0xFFFFFFFF
UNLIMITED = 0xFFFFFFFF
OUT_DTYPE = np.dtype([("inplace", "<u8"), ("fresh", "<u8"), ("too_long", "<u8"), ("shorted", "<u8"),
                      ("need", "<u4", (SLOTS,)), ("used", "<u4", (SLOTS,))])


def ptable_of(tab):
    """(cos_slot, slot_cap, nslot) of a cls.PoolTab."""
    return (np.ctypeslib.as_array(tab.cos_slot).copy(), np.ctypeslib.as_array(tab.slot_cap).copy(),
            int(tab.nslot))


def _pad(v):
    a = np.zeros(SLOTS, np.int64)
    v = np.asarray(v, np.int64)
    a[:v.shape[0]] = v
    return a


def plan_pools(records, lens, own, ptable, have, base):
    """(res_out, dec, idx, out): the per-record loop."""
    cos_slot, slot_cap, nslot = ptable
    cs, cap = cos_slot.tolist(), _pad(slot_cap).tolist()
    have, base = _pad(have).tolist(), _pad(base).tolist()
    n = records.shape[0]
    ow = [0] * n if own is None else np.asarray(own).tolist()
    res_out = records.copy()
    dec = np.zeros(n, np.uint32)
    idx = np.full(n, NO_IDX, np.uint32)
    need = [0] * SLOTS
    cnt = {PF_INPLACE: 0, PF_FRESH: 0, PF_TOO_LONG: 0, PF_SHORT: 0}
    rec = zip(records["outcome"].tolist(), records["cos"].tolist(), np.asarray(lens).tolist())
    for i, (outcome, cos, ln) in enumerate(rec):
        slot = cs[cos]
        if outcome != M.OUT_ENQ or slot >= nslot:
            continue                      # NONE: dec 0, no index
        if ow[i] == slot + 1:
            fate = PF_INPLACE             # never too long: the pools are compared first
        elif ln > cap[slot]:
            fate = PF_TOO_LONG            # takes no rank
        else:
            rank = need[slot]
            need[slot] += 1
            if rank < have[slot]:
                fate = PF_FRESH
                idx[i] = base[slot] + rank
            else:
                fate = PF_SHORT
        cnt[fate] += 1
        dec[i] = fate | slot << 4
        if fate in (PF_TOO_LONG, PF_SHORT):
            res_out["outcome"][i] = M.OUT_DISCARD
    used = [min(need[k], have[k]) for k in range(SLOTS)]
    out = {"inplace": cnt[PF_INPLACE], "fresh": cnt[PF_FRESH], "too_long": cnt[PF_TOO_LONG],
           "shorted": cnt[PF_SHORT], "need": need, "used": used}
    return res_out, dec, idx, out


def plan_pools_np(records, lens, own, ptable, have, base):
    """plan_pools() without a loop per record."""
    cos_slot, slot_cap, nslot = ptable
    cap, have, base = _pad(slot_cap), _pad(have), _pad(base)
    n = records.shape[0]
    ow = np.zeros(n, np.int64) if own is None else np.asarray(own).astype(np.int64)
    s = cos_slot.astype(np.int64)[records["cos"]]
    ok = (records["outcome"] == M.OUT_ENQ) & (s < nslot)
    slot = np.where(ok, s, 0)
    inpl = ok & (ow == slot + 1)
    tl = ok & ~inpl & (np.asarray(lens).astype(np.int64) > cap[slot])
    ranked = ok & ~inpl & ~tl
    rank = np.zeros(n, np.int64)
    need = np.zeros(SLOTS, np.int64)
    for k in range(SLOTS):
        m = ranked & (slot == k)
        need[k] = int(m.sum())
        rank[m] = np.arange(need[k])
    fresh = ranked & (rank < have[slot])
    short = ranked & ~fresh
    fate = np.select([inpl, tl, fresh, short], [PF_INPLACE, PF_TOO_LONG, PF_FRESH, PF_SHORT], PF_NONE)
    dec = (fate | slot << 4).astype(np.uint32)
    idx = np.where(fresh, base[slot] + rank, NO_IDX).astype(np.uint32)
    res_out = records.copy()
    res_out["outcome"][tl | short] = M.OUT_DISCARD
    out = {"inplace": int(inpl.sum()), "fresh": int(fresh.sum()), "too_long": int(tl.sum()),
           "shorted": int(short.sum()), "need": need.tolist(), "used": np.minimum(need, have).tolist()}
    return res_out, dec, idx, out


def same(a, b):
    """Two plans are equal in every word."""
    assert a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes()
    assert a[1].dtype == b[1].dtype == np.uint32 and np.array_equal(a[1], b[1])
    assert a[2].dtype == b[2].dtype == np.uint32 and np.array_equal(a[2], b[2])
    assert a[3] == b[3]


def reference_loop(records, lens, own, ptable, avail, table):
    """The reference's receive loop, packet by packet (loop.c:319-337): parse
    result, classification result, then _odp_pktio_packet_to_pool -- nothing to
    do when the packet is of the CoS's pool already, else a copy into a packet
    allocated from that pool, which fails when the pool has no free packet or
    the frame is longer than its packets (the packet is freed, in_discards) --
    then the counters and the enqueue.  avail[k]: pool k's free packets before
    the batch; none returns during it.  Returns (per destination id the
    survivors in order, the freed packets in order, the four counters).
    A record of a CoS the pool table has no slot for, or that the enqueue table
    does not map, is not of this control plane: it is freed and counts nothing
    more (after its pool switch, where it has a slot)."""
    cos_slot, slot_cap, nslot = ptable
    cos_nq, cos_q0, ent_dst, ndst = table
    free = _pad(avail).tolist()
    cap = _pad(slot_cap).tolist()
    queues = [[] for _ in range(ndst)]
    freed = []
    c = {"in_errors": 0, "in_discards": 0, "packets": 0, "octets": 0}
    for i in range(records.shape[0]):
        r = records[i]
        err, outcome, cos, queue, ln = int(r["err"]), int(r["outcome"]), int(r["cos"]), int(r["queue"]), int(lens[i])
        if err != 0 or outcome == M.OUT_PARSE_DROP:
            c["in_errors"] += 1           # ret != 0 from the parser
        if outcome != M.OUT_ENQ:
            if outcome in (M.OUT_DISCARD, M.OUT_LOOP):
                c["in_discards"] += 1     # the classifier returned < 0
            freed.append(i)
            continue
        new_pool = int(cos_slot[cos])
        if new_pool >= nslot:
            freed.append(i)
            continue
        mine = (int(own[i]) - 1) if own is not None and int(own[i]) else None
        if new_pool != mine:              # _odp_pktio_packet_to_pool: odp_packet_copy(pkt, new_pool)
            if free[new_pool] == 0 or ln > cap[new_pool]:
                freed.append(i)
                c["in_discards"] += 1
                continue
            free[new_pool] -= 1
        e = int(cos_q0[cos]) + queue
        if not (queue < int(cos_nq[cos]) and e < M.ENT and int(ent_dst[e]) < ndst):
            freed.append(i)
            continue
        if err == 0:
            c["packets"] += 1
            c["octets"] += ln
        queues[int(ent_dst[e])].append(i)
    return queues, freed, c


# ---- synthetic pool tables and own[] ---------------------------------------
CAPS = (1000, 30000, 65535)


def make_ptable(rng, nslot, cos_nq=None, caps=CAPS):
    """nslot slots with capacities from caps.  cos_nq given: exactly the CoS
    with queues have a slot (a control plane's tables agree); else about three
    CoS in four have one, and a few name a slot past nslot."""
    cos_slot = rng.integers(0, nslot, 256).astype(np.uint8)
    if cos_nq is not None:
        cos_slot[np.asarray(cos_nq) == 0] = 0xFF
    else:
        cos_slot[rng.integers(0, 4, 256) == 0] = 0xFF
        if nslot < SLOTS:
            cos_slot[rng.integers(0, 16, 256) == 0] = nslot
    slot_cap = np.zeros(SLOTS, np.uint32)
    slot_cap[:nslot] = np.asarray(caps)[rng.integers(0, len(caps), nslot)]
    return cos_slot, slot_cap, nslot


def make_own(rng, records, ptable, share=3):
    """own[]: about one record in `share` sits in a packet of its CoS's slot, as
    many in one of another slot or of a pool without a slot (0, or a value
    past nslot), the rest in none."""
    cos_slot, _, nslot = ptable
    n = records.shape[0]
    s = cos_slot.astype(np.int64)[records["cos"]]
    pick = rng.integers(0, share, n)
    own = np.where(pick == 0, np.where(s < nslot, s + 1, 0), rng.integers(0, nslot + 3, n))
    return own.astype(np.uint8)
