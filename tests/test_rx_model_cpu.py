"""Pins tests/rx_model.py (the CPU model the receive-chain and delivery
kernels are compared with) to the reference-derived expectation of the
receive path, tests/rt_helpers.expected: the per-queue packet sequences
(order, pool, flags, offsets, mark, bytes) and the four pktio counters read
off the model's perm / gcnt / dq / metadata lines must be what the oracle's
records give under the reference's receive rules.  Also checks the harness's
struct layouts against include/mi_cls.h with a compiled probe.  No GPU."""
import os
import subprocess
from collections import defaultdict

import numpy as np
import pytest

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import rt_helpers as H
from tests import rx_harness as X
from tests import rx_model as M
from tests import zoo

INPUT = 0x1122334455667788


def _frames():
    return H.pcap_frames([f for _, f in zoo.all_frames()])


def _records(prog, frames):
    from oracle.oracle import Oracle
    o = Oracle()
    o.apply(prog)
    return o.classify(pg.batch_from_frames(frames))


def _reported(pool, line, frame):
    """A packet as rt_helpers.expected lists it (what tests/rt/rx_driver.c
    reads through the packet accessors)."""
    m = np.frombuffer(line, M.META_DTYPE)[0]
    fl, err = int(m["in_flags"]), int(m["err"])
    l3st = 0 if not (fl >> 30) & 1 else (1 if err & 4 else 2)
    l4st = 0 if not (fl >> 31) & 1 else (1 if err & 64 else 2)
    assert int(m["len"]) == len(frame) and int(m["input"]) == INPUT and int(m["l2"]) == 0
    return (pool, (fl & H.FLAG_MASK) | (l3st << 40) | (l4st << 42), int(err != 0), int(m["l3"]),
            int(m["l4"]), int(m["cls_mark"]) if fl & 1 else 0, len(frame), frame.hex())


def _programs():
    base = [f for _, f in zoo.all_frames()]
    return [("everything", zoo.prog_everything(), 0), ("deletes", zoo.prog_deletes(), 1),
            ("random7", zoo.random_program(np.random.default_rng(7), base), 1),
            ("random8", zoo.random_program(np.random.default_rng(8), base), 1)]


@pytest.mark.parametrize("burst", [37, 4096])
@pytest.mark.parametrize("case", range(4))
def test_decide_gives_the_reference_queues(built, case, burst):
    name, prog, cos_pools = _programs()[case]
    frames = _frames()
    recs = _records(prog, frames)
    tab, pools, qnames = M.prog_table(prog, cos_pools)
    got_q, stats = defaultdict(list), [0, 0, 0, 0]
    for b0 in range(0, len(frames), burst):
        r, fr = recs[b0: b0 + burst], frames[b0: b0 + burst]
        n = len(fr)
        lens = [len(f) for f in fr]
        # packet handle = (slot + 1) << 20 | index: plenty of every slot
        got_base = [k * n for k in range(M.RX_POOLS)]
        got = np.array([((k + 1) << 20) | j for k in range(M.RX_POOLS) for j in range(n)], np.uint64)
        d = M.decide(r, lens, tab, [n] * M.RX_POOLS, got_base, got)
        # perm is the stable sort of the delivered frames by their group
        g = (d.dec >> 8) & 0x7F
        idx = np.nonzero(g != M.NO_GROUP)[0]
        assert np.array_equal(d.perm, idx[np.argsort(g[idx], kind="stable")])
        assert np.array_equal(idx, np.nonzero(d.ent)[0]) and not d.out.short_pool
        for h, members in M.queues_of(d, n).items():
            for i in members:
                line = M.chain_meta(d, i, r[i], lens[i], X.HEADROOM, INPUT, None, None)
                pool = pools[(int(d.ent[i]) >> 20) - 1]
                assert (int(d.dec[i]) >> 2) & 31 == (int(d.ent[i]) >> 20) - 1
                got_q[qnames[h]].append(_reported(pool, line, fr[i]))
        stats[0] += d.out.packets
        stats[1] += d.out.in_errors
        stats[2] += d.out.in_discards
        stats[3] += d.out.octets
    exp_q, exp_stats, _ = H.expected(prog, frames, cos_pools=cos_pools)
    H.compare((dict(got_q), tuple(stats), {}), (exp_q, exp_stats, {}))


def test_decide_short_pool_leaves_out_the_slots_last_frame(built):
    prog = zoo.prog_deletes()
    frames = _frames()
    recs = _records(prog, frames)
    tab, pools, _ = M.prog_table(prog, 1)
    n = len(frames)
    lens = [len(f) for f in frames]
    got_base = [k * n for k in range(M.RX_POOLS)]
    got = np.arange(1, 1 + n * M.RX_POOLS, dtype=np.uint64)
    full = M.decide(recs, lens, tab, [n] * M.RX_POOLS, got_base, got)
    k = int(np.argmax(full.out.need))
    assert full.out.need[k] > 1 and sum(1 for x in full.out.need if x) > 1
    have = [n] * M.RX_POOLS
    have[k] = full.out.need[k] - 1
    d = M.decide(recs, lens, tab, have, got_base, got)
    assert d.out.short_pool == 1 and d.out.need == full.out.need and d.out.used[k] == have[k]
    of_k = [i for i in range(n) if int(d.dec[i]) & 3 == M.RXF_FRESH and (int(d.dec[i]) >> 2) & 31 == k]
    missing = [i for i in of_k if not d.ent[i]]
    assert missing == [of_k[-1]]
    assert (int(d.dec[missing[0]]) >> 8) & 0x7F == M.NO_GROUP
    others = [i for i in range(n) if i != missing[0]]
    assert np.array_equal(d.ent[others], full.ent[others])
    assert np.array_equal(d.dec[others], full.dec[others])


@pytest.mark.parametrize("layer", [1, 2, 3, 4])
def test_deliver_gives_the_parser_only_queue(built, layer):
    """mi_cls_deliver_submit's metadata at every parser layer of a pktio
    without the classifier: the host keeps every frame but a parse drop (below
    L4 only an IP-error drop at L3 is one: odp_parse.c:372-414)."""
    frames = _frames()
    recs = _records([], frames)
    keep = []
    for i, r in enumerate(recs):
        drop = int(r["outcome"]) == R.OUT_PARSE_DROP
        if layer < 3 and not (layer == 2 and int(r["err"]) & 2):
            drop = False
        if not drop:
            keep.append(i)
    dlv = np.zeros(len(keep), M.DLV_DTYPE)
    dlv["rec"], dlv["flags"], dlv["qid"] = keep, M.DLV_FRESH | M.DLV_COPY, 0
    dlv["len"] = [len(frames[i]) for i in keep]
    d = M.deliver(recs, dlv, layer, INPUT, X.HEADROOM, None)
    assert np.array_equal(d.perm, np.arange(len(keep))) and int(d.gcnt[0]) == len(keep)
    got = [_reported("pktio_pool", d.lines[j], frames[i]) for j, i in enumerate(keep)]
    for line in d.lines:
        m = np.frombuffer(line, M.META_DTYPE)[0]
        assert int(m["cos"]) == 0xFF and int(m["dst_queue"]) == 0 and int(m["cls_mark"]) == 0
    exp_q, _, _ = H.expected([], frames, cls=0, layer=layer)
    H.compare(({"odp-pktin-0-0": got}, None, {}), (exp_q, None, {}))


def test_stable_groups_is_argsort():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 80, 5000)
    q[q >= 64] = 0xFF
    perm, cnt = M.stable_groups(q)
    idx = np.nonzero(q < 64)[0]
    assert np.array_equal(perm, idx[np.argsort(q[idx], kind="stable")])
    assert np.array_equal(cnt, np.bincount(q[idx], minlength=64))


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "mi_cls.h"
#define S(t) printf(#t " = %zu\n", sizeof(t))
#define F(t, f) printf(#t " " #f " %zu\n", offsetof(t, f))
int main(void)
{
	printf("GROUP_MAX %d GROUPS %d POOLS %d QENT %d\n", MI_CLS_DLV_GROUP_MAX, MI_CLS_DLV_GROUPS,
	       MI_CLS_RX_POOLS, MI_CLS_RX_QENT);
FIELDS
	return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of every bound field, printed by a C probe compiled
    against include/mi_cls.h."""
    names = sorted(set(X.STRUCTS) | set(X.DTYPES))
    lines = []
    for t in names:
        lines.append(f"\tS({t});")
        for f in X.layout_of(t)[0]:
            if f:
                lines.append(f"\tF({t}, {f});")
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("FIELDS", "\n".join(lines)))
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I", os.path.join(H.ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.check_output([exe], text=True)
    c = defaultdict(dict)
    for ln in out.splitlines():
        if ln.startswith("GROUP_MAX"):
            assert ln.split() == ["GROUP_MAX", str(M.DLV_GROUP_MAX), "GROUPS", str(M.DLV_GROUPS),
                                  "POOLS", str(M.RX_POOLS), "QENT", str(M.RX_QENT)]
            continue
        w = ln.split()
        if w[1] == "=":
            c[w[0]][""] = int(w[2])
        else:
            c[w[0]][w[1]] = int(w[2])
    for t in names:
        for lay in X.layout_of(t):
            assert lay == c[t], (t, lay, c[t])
