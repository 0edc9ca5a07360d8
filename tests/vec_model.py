"""CPU model of the vector fill (mi_cls_vec_fill, include/mi_cls.h).

fill() is the literal per-run loop of _odp_cos_enq / _odp_cos_vector_enq
(odp_classification_internal.h:83-167) over a run plan: a plain run's packets
become its events; a vector run allocates vectors one by one until its slot's
stock is gone, fills them, and the packets that found no vector are lost.
fill_np() states the same with numpy and no loop per packet or per run;
tests/test_vec_fill_cpu.py holds the two equal on random plans, and the GPU
tests use the numpy form.

Both return a dict:
  ev        uint64[ev_span]: packet handles, vector handles (their vgot value), 0
  evr       EVRUN_DTYPE[nruns]
  lost      uint64, sorted (the order inside lost[] is unspecified)
  vec_idx   the vgot indexes of the vectors written, ascending
  vec_size  their sizes
  vec_tbl   their tables, one behind the other in that order
  out       the counters of mi_cls_vec_out_t (vec_used: a list)
A run table is run_model's tuple (mode, vmax, vslot).  ok(v, size) -> bool
array says which vectors the device accepts (None: all of them).
"""
import numpy as np

from tests.run_model import VEC, VSLOTS

NONE = 0xFFFFFFFF
EVRUN_DTYPE = np.dtype([("ev_first", "<u4"), ("ev_count", "<u4"), ("pk_enq", "<u4"), ("vfirst", "<u4")])
FIELDS = ("events", "ev_span", "vectors", "in_vectors", "lost", "holes", "refused", "truncated", "vec_used")


def arena_ok(lo, nbytes, tbl_off):
    """The device's test of a vector: not 0, 8-byte aligned, [v, v + tbl_off +
    8 * size) inside [lo, lo + nbytes)."""
    def ok(v, size):
        v = np.asarray(v, np.uint64).astype(object)
        need = tbl_off + 8 * np.asarray(size, np.int64).astype(object)
        return np.array([x != 0 and x % 8 == 0 and x >= lo and x + n <= lo + nbytes
                         for x, n in zip(v.reshape(-1), need.reshape(-1))], bool)
    return ok


def truncated():
    """out of a fill over a truncated plan: nothing else is written."""
    out = dict.fromkeys(FIELDS[:8], 0)
    out["truncated"] = 1
    out["vec_used"] = [0] * VSLOTS
    return out


def _result(ev, evr, lost, vecs, c, need, vhave):
    idx = sorted(vecs)
    c["ev_span"], c["truncated"] = len(ev), 0
    c["events"] = int(sum(r[1] for r in evr))
    c["vec_used"] = [min(int(need[s]), int(vhave[s])) for s in range(VSLOTS)]
    return {"ev": np.array(ev, np.uint64), "evr": np.array(evr, EVRUN_DTYPE).reshape(-1),
            "lost": np.sort(np.array(lost, np.uint64)),
            "vec_idx": np.array(idx, np.int64), "vec_size": np.array([vecs[i][0] for i in idx], np.int64),
            "vec_tbl": np.array([h for i in idx for h in vecs[i][1]], np.uint64), "out": c}


def _pad(v):
    a = np.zeros(VSLOTS, np.int64)
    a[:len(v)] = np.asarray(v, np.int64)
    return a


def fill(seq, runs, ent, rtable, vgot, vbase, vhave, ent_to_handle=0, ok=None):
    """The per-run loop."""
    _, vmax, vslot = rtable
    vbase, vhave = _pad(vbase), _pad(vhave)
    stock = [list(range(int(vbase[s]), int(vbase[s] + vhave[s]))) for s in range(VSLOTS)]
    need = [0] * VSLOTS
    c = dict.fromkeys(FIELDS[:8], 0)
    ev, evr, lost, vecs = [], [], [], {}

    def hnd(i):
        e = int(ent[i])
        return e - ent_to_handle if e else 0

    for r in runs:
        first, count, cos = int(r["first"]), int(r["count"]), int(r["cos"])
        pk = [hnd(int(seq[first + o])) for o in range(count)]
        if not int(r["flags"]) & VEC:
            evr.append((len(ev), count, count, NONE))
            ev.extend(pk)
            c["holes"] += pk.count(0)
            continue
        s, vm, nvec = int(vslot[cos]), int(vmax[cos]), int(r["nvec"])
        need[s] += nvec
        got = []
        for _ in range(nvec):          # odp_packet_vector_alloc until it fails
            if not stock[s]:
                break
            got.append(stock[s].pop(0))
        ev_first, num_enq = len(ev), 0
        for vi in got:
            sz = min(vm, count - num_enq)
            tbl = pk[num_enq:num_enq + sz]
            v = int(vgot[vi])
            if ok is None or ok(np.array([v], np.uint64), np.array([sz]))[0]:
                vecs[vi] = (sz, tbl)
                ev.append(v)
                c["vectors"] += 1
                c["in_vectors"] += sz
                c["holes"] += tbl.count(0)
            else:                       # refused: nothing of it is written
                ev.append(0)
                c["refused"] += 1
            num_enq += sz
        ev.extend([0] * (nvec - len(got)))
        rest = pk[num_enq:]
        lost.extend(rest)
        c["holes"] += rest.count(0)
        c["lost"] += len(rest)
        evr.append((ev_first, len(got), num_enq, got[0] if got else NONE))
    return _result(ev, evr, lost, vecs, c, need, vhave)


def fill_np(seq, runs, ent, rtable, vgot, vbase, vhave, ent_to_handle=0, ok=None):
    """fill() without a loop per run or per packet."""
    _, vmax, vslot = (np.asarray(x).astype(np.int64) for x in rtable)
    vbase, vhave = _pad(vbase), _pad(vhave)
    vgot = np.asarray(vgot, np.uint64)
    nr = len(runs)
    first, count = runs["first"].astype(np.int64), runs["count"].astype(np.int64)
    cos = runs["cos"].astype(np.int64)
    isvec = (runs["flags"] & VEC) != 0
    slot, vm = vslot[cos], np.maximum(vmax[cos], 1)
    wv = np.where(isvec, runs["nvec"].astype(np.int64), 0)
    rank = np.zeros(nr, np.int64)
    need = np.zeros(VSLOTS, np.int64)
    for s in range(VSLOTS):
        m = isvec & (slot == s)
        cs = np.cumsum(wv[m])
        rank[m] = cs - wv[m]
        need[s] = cs[-1] if cs.size else 0
    g = np.where(isvec, np.clip(vhave[slot] - rank, 0, wv), 0)
    we = np.where(isvec, wv, count)
    ev_first = np.cumsum(we) - we
    evr = np.zeros(nr, EVRUN_DTYPE)
    evr["ev_first"] = ev_first
    evr["ev_count"] = np.where(isvec, g, count)
    evr["pk_enq"] = np.where(isvec, np.minimum(count, g * vm), count)
    evr["vfirst"] = np.where(isvec & (g > 0), vbase[slot] + rank, NONE)
    # every delivered place: its run, its offset in it, its handle
    dl = int(count.sum())
    run_of = np.repeat(np.arange(nr), count)
    o = np.arange(dl) - first[run_of]
    e = np.asarray(ent, np.uint64)[np.asarray(seq[:dl], np.int64)]
    h = np.where(e != 0, e - np.uint64(ent_to_handle), np.uint64(0)).astype(np.uint64)
    ev = np.zeros(int(we.sum()), np.uint64)
    pv = isvec[run_of]
    ev[ev_first[run_of[~pv]] + o[~pv]] = h[~pv]
    k = o // vm[run_of]
    j = o - k * vm[run_of]
    inv = pv & (k < g[run_of])
    vi = np.where(inv, vbase[slot[run_of]] + rank[run_of] + k, 0)
    size = np.minimum(vm[run_of], count[run_of] - k * vm[run_of])
    good = inv.copy()
    if ok is not None and inv.any():
        hd = inv & (j == 0)
        okv = np.zeros(int(vi.max()) + 1, bool)
        okv[vi[hd]] = ok(vgot[vi[hd]], size[hd])
        good &= okv[vi]
    hd = inv & (j == 0)
    ev[ev_first[run_of[hd]] + k[hd]] = np.where(good[hd], vgot[vi[hd]], np.uint64(0))
    lostp = pv & ~inv
    order = np.lexsort((j[good], vi[good]))
    heads = good & (j == 0)
    hs = np.argsort(vi[heads], kind="stable")
    c = {"events": int(evr["ev_count"].astype(np.int64).sum()), "ev_span": int(ev.shape[0]),
         "vectors": int(heads.sum()), "in_vectors": int(good.sum()), "lost": int(lostp.sum()),
         "holes": int(np.count_nonzero(h[~pv | good | lostp] == 0)), "refused": int((hd & ~good).sum()),
         "truncated": 0, "vec_used": np.minimum(need, vhave).tolist()}
    return {"ev": ev, "evr": evr, "lost": np.sort(h[lostp]), "vec_idx": vi[heads][hs],
            "vec_size": size[heads][hs], "vec_tbl": h[good][order], "out": c}


def same(a, b):
    for k in ("ev", "evr", "lost", "vec_idx", "vec_size", "vec_tbl"):
        assert np.array_equal(a[k], b[k]), k
    assert a["evr"].dtype == b["evr"].dtype == EVRUN_DTYPE
    assert a["out"] == b["out"], (a["out"], b["out"])


def events(runs, res, name_of):
    """Per queue name the deliveries a consumer of the fill makes, in order:
    ("P",) a packet of a plain run, ("V", k) a vector of k packets -- the form
    of rt_helpers.expected_vectors and of the receive path's event lists."""
    size_of = dict(zip(res["vec_idx"].tolist(), res["vec_size"].tolist()))
    ev = {}
    for r, x in zip(runs, res["evr"]):
        q = ev.setdefault(name_of[int(r["dst"])], [])
        if not int(r["flags"]) & VEC:
            q.extend([("P",)] * int(x["ev_count"]))
            continue
        for k in range(int(x["ev_count"])):
            q.append(("V", size_of[int(x["vfirst"]) + k]))
    return ev


def make_ent(rng, n, base=0x10000, stride=0x800, holes=0.0):
    """n distinct line addresses (64-byte aligned), a share of them 0."""
    ent = (base + stride * rng.permutation(n)).astype(np.uint64)
    if holes:
        ent[rng.random(n) < holes] = 0
    return ent
