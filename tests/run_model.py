"""CPU model of the run plan (mi_cls_enq_runs, include/mi_cls.h).

plan_runs() is the literal per-record loop of a pktio driver with packet-vector
or aggregator CoS (_odp_cls_enq / _odp_cos_enq / _odp_cos_vector_enq,
odp_classification_internal.h:83-236): the delivered records in arrival order,
a new run whenever (destination id, cos) changes or a burst begins, each run's
flavour and vector count, the records that are not delivered, the counters.
plan_runs_np() states the same with numpy; tests/test_enq_runs_cpu.py holds the
two equal on random records, and the GPU tests use the numpy form where a
Python loop per record would take seconds.

A table is enq_model's tuple (cos_nq, cos_q0, ent_dst, ndst); a run table the
tuple (mode[256], vmax[256], vslot[256]) of mi_cls_run_tab_t.
"""
import numpy as np

from tests import enq_model as M

AGGR, VEC, VSLOTS = 1, 2, 16
RUN_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("dst", "<u2"), ("cos", "u1"), ("flags", "u1"),
                      ("nvec", "<u4")])
FIELDS = M.FIELDS + ("nruns", "vectors", "vec_need")


def rtable_of(rtab):
    """(mode, vmax, vslot) of a cls.RunTab."""
    return tuple(np.ctypeslib.as_array(getattr(rtab, k)).copy() for k in ("mode", "vmax", "vslot"))


def _finish(first, count, dst, cos, rtable, c):
    """The runs' flavour and vectors; the counters that follow from them."""
    mode, vmax, vslot = (np.asarray(x).astype(np.int64) for x in rtable)
    runs = np.zeros(len(first), RUN_DTYPE)
    runs["first"], runs["count"], runs["dst"], runs["cos"] = first, count, dst, cos
    count = np.asarray(count, np.int64)
    cos = np.asarray(cos, np.int64)
    vec = (count >= 2) & ((mode[cos] & VEC) != 0)
    nvec = np.where(vec, -(-count // np.maximum(vmax[cos], 1)), 0)
    runs["flags"] = np.where(vec, VEC, mode[cos] & AGGR)
    runs["nvec"] = nvec
    c["nruns"] = len(first)
    c["vectors"] = int(nvec.sum())
    c["vec_need"] = np.bincount(vslot[cos][vec], weights=nvec[vec], minlength=VSLOTS).astype(np.int64).tolist()
    return runs


def plan_runs(records, lens, table, rtable, burst=0):
    """(seq, runs, out): the per-record loop."""
    cos_nq, cos_q0, ent_dst, ndst = table
    nq, q0, dst = cos_nq.tolist(), cos_q0.tolist(), ent_dst.tolist()
    c = dict.fromkeys(M.FIELDS, 0)
    dlv, rest = [], []
    runs = []      # [first, count, id, cos]
    prev = None    # the (id, cos) of the run that is open
    rec = zip(records["err"].tolist(), records["outcome"].tolist(), records["cos"].tolist(),
              records["queue"].tolist(), np.asarray(lens).tolist())
    for i, (err, outcome, cos, queue, ln) in enumerate(rec):
        if burst and i % burst == 0:
            prev = None   # the burst before ended: its last run is enqueued
        if err != 0 or outcome == M.OUT_PARSE_DROP:
            c["in_errors"] += 1
        if outcome in (M.OUT_DISCARD, M.OUT_LOOP):
            c["in_discards"] += 1
        g = None
        if outcome == M.OUT_ENQ:
            e = q0[cos] + queue
            if queue < nq[cos] and e < M.ENT and dst[e] < ndst:
                g = dst[e]
                c["delivered"] += 1
                if err == 0:
                    c["packets"] += 1
                    c["octets"] += ln
            else:
                c["stale"] += 1
        if g is None:
            rest.append(i)   # ends no run
            continue
        if (g, cos) != prev:
            runs.append([len(dlv), 0, g, cos])
            prev = (g, cos)
        runs[-1][1] += 1
        dlv.append(i)
    seq = np.array(dlv + rest, dtype=np.uint32)
    cols = list(zip(*runs)) if runs else [[], [], [], []]
    return seq, _finish(*cols, rtable, c), c


def plan_runs_np(records, lens, table, rtable, burst=0):
    """plan_runs() without a loop per record."""
    ndst = table[3]
    n = records.shape[0]
    k, stale = M.keys(records, table)
    dlv = k < ndst
    good = dlv & (records["err"] == 0)
    c = {"in_errors": int(np.count_nonzero((records["err"] != 0) | (records["outcome"] == M.OUT_PARSE_DROP))),
         "in_discards": int(np.count_nonzero(np.isin(records["outcome"], (M.OUT_DISCARD, M.OUT_LOOP)))),
         "packets": int(np.count_nonzero(good)),
         "octets": int(np.asarray(lens).astype(np.int64)[good].sum()),
         "delivered": int(np.count_nonzero(dlv)), "stale": int(np.count_nonzero(stale))}
    idx = np.nonzero(dlv)[0]
    seq = np.concatenate([idx, np.nonzero(~dlv)[0]]).astype(np.uint32)
    ids = k[idx]
    cos = records["cos"][idx].astype(np.int64)
    b = idx // burst if burst else np.zeros(idx.shape[0], np.int64)
    head = np.ones(idx.shape[0], bool)
    head[1:] = (ids[1:] != ids[:-1]) | (cos[1:] != cos[:-1]) | (b[1:] != b[:-1])
    first = np.nonzero(head)[0]
    count = np.diff(np.concatenate([first, [idx.shape[0]]]))
    assert n == seq.shape[0]
    return seq, _finish(first, count, ids[first], cos[first], rtable, c), c


def events(runs, rtable, name_of):
    """Per queue name the deliveries of the runs, in order: ("P",) a packet of
    a plain run, ("V", k) a vector of k packets -- what
    rt_helpers.expected_vectors lists."""
    vmax = rtable[1]
    ev = {}
    for r in runs:
        q = ev.setdefault(name_of[int(r["dst"])], [])
        left = int(r["count"])
        if not r["flags"] & VEC:
            q.extend([("P",)] * left)
            continue
        for _ in range(int(r["nvec"])):
            k = min(left, int(vmax[int(r["cos"])]))
            q.append(("V", k))
            left -= k
        assert left == 0
    return ev


# ---- synthetic run tables ----------------------------------------------------
def make_rtable(rng, nslots=3, vmaxes=(1, 2, 3, 8, 64, 4096)):
    """Every mode among the 256 CoS, vector sizes from vmaxes, nslots slots."""
    mode = rng.integers(0, 4, 256).astype(np.uint8)
    vmax = np.asarray(vmaxes)[rng.integers(0, len(vmaxes), 256)].astype(np.uint16)
    vslot = rng.integers(0, nslots, 256).astype(np.uint8)
    return mode, vmax, vslot


def uniform_rtable(mode, vmax, vslot=0):
    return (np.full(256, mode, np.uint8), np.full(256, vmax, np.uint16), np.full(256, vslot, np.uint8))
