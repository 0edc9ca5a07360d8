"""CPU model of the enqueue plan (mi_cls_enq_plan, include/mi_cls.h).

plan() is the literal per-record loop a pktio driver runs over a classified
batch's records (loopback_recv_gpu): one list per destination
id, one for the records that are not delivered, the pktio counters of
loopback_recv.  plan_sorted() states the same with a stable argsort of the
keys; tests/test_enq_plan_cpu.py holds the two equal on random records, and
the GPU tests use plan_sorted() where a Python loop per record would take
seconds.

A table is the tuple (cos_nq[256], cos_q0[256], ent_dst[ENT], ndst) of
mi_cls_enq_tab_t; table_of() takes it from the ctypes struct.
"""
import numpy as np

OUT_ENQ, OUT_COS_DROP, OUT_DISCARD, OUT_PARSE_DROP, OUT_LOOP = 0, 1, 2, 3, 4
ENT = 8192
DST_MAX = 8192
FIELDS = ("in_errors", "in_discards", "packets", "octets", "delivered", "stale")


def table_of(tab):
    """(cos_nq, cos_q0, ent_dst, ndst) of a cls.EnqTab."""
    return (np.ctypeslib.as_array(tab.cos_nq).copy(), np.ctypeslib.as_array(tab.cos_q0).copy(),
            np.ctypeslib.as_array(tab.ent_dst).copy(), int(tab.ndst))


def plan(records, lens, table):
    """(perm, gbeg, counters): the per-record loop."""
    cos_nq, cos_q0, ent_dst, ndst = table
    nq, q0, dst = cos_nq.tolist(), cos_q0.tolist(), ent_dst.tolist()
    groups = [[] for _ in range(ndst + 1)]   # the last one: not delivered
    c = dict.fromkeys(FIELDS, 0)
    rec = zip(records["err"].tolist(), records["outcome"].tolist(), records["cos"].tolist(),
              records["queue"].tolist(), np.asarray(lens).tolist())
    for i, (err, outcome, cos, queue, ln) in enumerate(rec):
        if err != 0 or outcome == OUT_PARSE_DROP:
            c["in_errors"] += 1
        if outcome in (OUT_DISCARD, OUT_LOOP):
            c["in_discards"] += 1
        g = ndst
        if outcome == OUT_ENQ:
            e = q0[cos] + queue
            if queue < nq[cos] and e < ENT and dst[e] < ndst:
                g = dst[e]
                c["delivered"] += 1
                if err == 0:
                    c["packets"] += 1
                    c["octets"] += ln
            else:
                c["stale"] += 1   # the table does not map the record
        groups[g].append(i)
    perm = np.array([i for g in groups for i in g], dtype=np.uint32)
    gbeg = np.zeros(ndst + 2, dtype=np.uint32)
    gbeg[1:] = np.cumsum([len(g) for g in groups])
    return perm, gbeg, c


def keys(records, table):
    """Each record's group: its destination id, ndst when it is not delivered;
    and which enqueue records the table does not map."""
    cos_nq, cos_q0, ent_dst, ndst = table
    cos = records["cos"].astype(np.int64)
    queue = records["queue"].astype(np.int64)
    e = cos_q0.astype(np.int64)[cos] + queue
    enq = records["outcome"] == OUT_ENQ
    ok = enq & (queue < cos_nq.astype(np.int64)[cos]) & (e < ENT)
    ids = np.where(ok, ent_dst.astype(np.int64)[np.minimum(e, ENT - 1)], ndst)
    ok &= ids < ndst
    return np.where(ok, ids, ndst), enq & ~ok


def plan_sorted(records, lens, table):
    """plan() by a stable sort of the keys."""
    ndst = table[3]
    k, stale = keys(records, table)
    dlv = k < ndst
    good = dlv & (records["err"] == 0)
    c = {"in_errors": int(np.count_nonzero((records["err"] != 0) | (records["outcome"] == OUT_PARSE_DROP))),
         "in_discards": int(np.count_nonzero(np.isin(records["outcome"], (OUT_DISCARD, OUT_LOOP)))),
         "packets": int(np.count_nonzero(good)),
         "octets": int(np.asarray(lens).astype(np.int64)[good].sum()),
         "delivered": int(np.count_nonzero(dlv)), "stale": int(np.count_nonzero(stale))}
    perm = np.argsort(k, kind="stable").astype(np.uint32)
    gbeg = np.zeros(ndst + 2, dtype=np.uint32)
    gbeg[1:] = np.cumsum(np.bincount(k, minlength=ndst + 1))
    return perm, gbeg, c


# ---- synthetic tables and records (no classification) ----------------------
NQ = 32   # queues per CoS of a synthetic table


def make_table(rng, ndst):
    """A table of ndst destination ids over CoS of NQ queues each (the last
    one what is left): every id has an entry, further entries share ids where
    there is room, ids in no order of the entries.  Returns (cos_nq, cos_q0,
    ent_dst, ndst) and entry_of[id], one entry per id."""
    nent = min(ENT, ndst + ndst // 4 + 1) if ndst else 0
    ent = np.concatenate([rng.permutation(ndst), rng.integers(0, max(1, ndst), nent - ndst)]).astype(np.uint16)
    rng.shuffle(ent)
    cos_nq = np.zeros(256, np.uint8)
    cos_q0 = np.zeros(256, np.uint16)
    ncos = (nent + NQ - 1) // NQ
    assert ncos <= 256
    for c in range(ncos):
        cos_q0[c] = c * NQ
        cos_nq[c] = min(NQ, nent - c * NQ)
    ent_dst = np.full(ENT, 0xFFFF, np.uint16)   # entries no CoS owns: never a valid id
    ent_dst[:nent] = ent
    entry_of = np.zeros(max(1, ndst), np.int64)
    entry_of[ent[::-1]] = np.arange(nent)[::-1]   # the first entry of each id
    return (cos_nq, cos_q0, ent_dst, ndst), entry_of


def make_records(rng, n, dst, entry_of, dtype):
    """n records: dst[i] >= 0 delivers record i to that id (through the id's
    entry), dst[i] < 0 gives it one of the outcomes that deliver nothing
    (-1 - dst[i], cycled by the caller).  err is set on about a seventh of the
    records, delivered or not; lens are random with 0 and 65535 among them."""
    dst = np.asarray(dst, np.int64)
    r = np.zeros(n, dtype)
    e = entry_of[np.maximum(dst, 0)]
    enq = dst >= 0
    r["outcome"] = np.where(enq, OUT_ENQ, -1 - dst).astype(np.uint8)
    r["cos"] = np.where(enq, e // NQ, rng.integers(0, 256, n)).astype(np.uint8)
    r["queue"] = np.where(enq, e % NQ, rng.integers(0, 40, n)).astype(np.uint16)
    r["err"] = np.where(rng.integers(0, 7, n) == 0, rng.integers(1, 128, n), 0).astype(np.uint8)
    r["in_flags"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    r["mark"] = rng.integers(0, 2 ** 16, n).astype(np.uint16)
    lens = rng.integers(0, 65536, n).astype(np.uint16)
    lens[rng.integers(0, 5, n) == 0] = 65535
    lens[rng.integers(0, 5, n) == 0] = 0
    return r, lens


NOT_DELIVERED = (OUT_COS_DROP, OUT_DISCARD, OUT_PARSE_DROP, OUT_LOOP, 5, 0xA5)   # the last two: no outcome


def drops(n):
    """dst values of n records that deliver nothing, every such outcome in turn."""
    return -1 - np.array(NOT_DELIVERED)[np.arange(n) % len(NOT_DELIVERED)]


def distribution(rng, name, n, ndst):
    """dst[n] of a named distribution (ndst >= 1)."""
    if name == "one":
        return np.full(n, ndst // 2)
    if name == "round_robin":
        return np.arange(n) % ndst
    if name == "none":
        return drops(n)
    if name == "last_only":
        d = drops(n)
        if n:
            d[-1] = ndst - 1
        return d
    if name == "skew":   # nine in ten to id 0, the rest anywhere or dropped
        d = np.where(rng.integers(0, 10, n) < 9, 0, rng.integers(0, ndst, n))
        return np.where(rng.integers(0, 20, n) == 0, drops(n), d)
    if name == "mixed":
        return np.where(rng.integers(0, 4, n) == 0, drops(n), rng.integers(0, ndst, n))
    raise ValueError(name)


DISTRIBUTIONS = ("one", "round_robin", "none", "last_only", "skew", "mixed")
