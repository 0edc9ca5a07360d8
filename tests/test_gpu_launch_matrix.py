"""One row per compiled instantiation of mi_cls_kernel: the smallest program
and knobs that make the launcher (mi_cls_classify / pick_shape in
odp_amd/csrc/mi_cls.hip) choose it, the instantiation last_launch() must then
report, and every record bit-identical to the CPU oracle through the poisoned
result buffer of tests.helpers.gpu_run.

The CPU test parses the MI_LAUNCH lines of the kernel translation units and
requires that set to equal the matrix's, so an instantiation added without a
row fails here, and checks on the CPU (program_info) that every row's program
still has the hot-region size and engine that lead to its kernel.  The first
section below restates pick_shape and the dispatch: the LDS limits are
computed from the same formula, not copied from a run.

Beside the matrix: the dynamic tile dealing (tiles 2 NW + k of a block, dealt
by its LDS counter) on the 12-wave, 8-wave and 4-wave / HBM shapes and on a
DIV kernel, and the window predictor's state across the launches of one
context and across the tiles of one wave.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from odp_amd import cls
from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import chksum_frames as CK
from tests import zoo
from tests.helpers import assert_same, classify_poisoned, gpu_run, knobs, oracle_run
from tests.test_gpu_parity import _under_root

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "odp_amd", "csrc")

# ------------------------------------------------------- the launcher, restated
# mi_cls_dev.h: WAVE, RS, WROWS = WIN / 4 + 1, MAX_STATS_COS, CRC_WORDS,
# MIN_WAVES_PER_EU; mi_cls.hip pick_shape: LDS_CU, MI_CLS_LDS_HOT_MAX's default
WAVE, RS, WIN, MAX_STATS_COS, OCC = 64, 66, 96, 256, 4
WROWS = WIN // 4 + 1
CRC_WORDS = 3072 + 256 + 65 + 64
LDS_CU = 160 * 1024
HOT_MAX = 20 * 1024


def st_of(w, ck=False):
    """Static LDS bytes of a block of w waves: windows, stats histogram, L4
    table, tile counter (+ the CRC-32C tables of the pktin-option kernels)."""
    return 4 * (w * RS * WROWS + MAX_STATS_COS + 256 + 1 + (CRC_WORDS if ck else 0))


def hot_bytes(info):
    return ((info["hot_words"] + 3) & ~3) * 4


def pick_shape(hot, wpb=0, ck=False):
    """(waves per block, hot region in LDS, blocks per CU) as pick_shape
    chooses them (no batch hint, no MI_CLS_BLOCKS_PER_CU / MI_CLS_LDS_HOT_MAX)."""
    small = hot <= HOT_MAX
    full4 = small and 4 * (st_of(4, ck) + hot) <= LDS_CU
    nw, lt = 4, full4
    for w in (16, 12, 8):
        if st_of(w, ck) + hot <= LDS_CU:
            nw, lt = w, True
            break
    if nw == 8 and full4:
        nw, lt = 4, True
    if wpb in (4, 8, 12, 16):
        nw = wpb
        lt = (small if nw == 4 else True) and st_of(nw, ck) + hot <= LDS_CU
        if nw not in (4, 16) and not lt:
            nw = 16
    if ck and nw != 4:
        nw = 16
        lt = st_of(16, ck) + hot <= LDS_CU
        if not lt:
            nw = 4
    per_cu = max(1, min(LDS_CU // (st_of(nw, ck) + (hot if lt else 0)), OCC * 4 // nw))
    return nw, lt, per_cu


def generic_kernel(info, wpb=0, ck=False):
    """(LT, DIV, NW, FM, CK) of the generic kernel mi_cls_classify launches for a
    program with this program_info()."""
    nw, lt, _ = pick_shape(hot_bytes(info), wpb, ck)
    fm = info["flat_engine"]
    if not ck and fm >= 0 and fm != 1 and lt and nw in (4, 12, 16):
        return (True, False, nw, fm, False)
    return (lt, info["tree"], nw, -1, ck)


def spec_accepted(info, plan, wpb=0, ck=False):
    """Whether spec_setup requests a specialised kernel: flat programs need
    the hot region in LDS and 4, 12 or 16 waves (4 or 16 with pktin options),
    tree plans 4, 8, 12 or 16 waves (4 or 16 with pktin options)."""
    nw, lt, _ = pick_shape(hot_bytes(info), wpb, ck)
    flat = info["flat_engine"] >= 0
    if not flat and not plan:
        return False
    if ck:
        return not (flat and not lt) and nw in (4, 16)
    return (lt and nw in (4, 12, 16)) if flat else nw in (4, 8, 12, 16)


# ------------------------------------------------------------------- programs
# name -> maker of (batch, program) for n packets
def _c4(num_rules):
    return lambda n: R.config4(n, num_rules=num_rules)


def _rooted(make):
    def f(n):
        b, prog = make(n)
        return b, _under_root(prog)
    return f


PROGRAMS = {
    "c2": lambda n: R.config2(n),                       # flat, direct (engine 0)
    "c3_8": lambda n: R.config3(n, num_rules=8),        # flat, bitmap (engine 2)
    "c3_64": lambda n: R.config3(n, num_rules=64),      # flat, single candidate (4); wide (3)
    "c4_1400": _c4(1400),                               # 12-wave hot region
    "c4_2048": _c4(2048),                               # 8-wave hot region
    "c4_3072": _c4(3072),                               # hot region stays in HBM
    "c2_tree": lambda n: R.config2(n, tree=True),       # small tree with a plan
    "c5": lambda n: R.config5(n),                       # config 5's tree (plan), 52 KB hot
}
for _k in ("c3_64", "c4_1400", "c4_2048", "c4_3072"):
    PROGRAMS[_k + "_root"] = _rooted(PROGRAMS[_k])      # trees without a plan
HAS_PLAN = {"c2_tree", "c5"}   # trees whose levels are joint groups: they get a tree plan

N_ROW = 4501   # 71 tiles, the last of 21 packets; five 16-wave blocks


@functools.lru_cache(maxsize=None)
def row_case(name):
    """The program and its N_ROW packets, one frame of the parser zoo put into
    every tile (at a different lane each) so the general parser runs too."""
    b, prog = PROGRAMS[name](N_ROW)
    frames = [b.frame(i) for i in range(b.n)]
    z = [f for _, f in zoo.all_frames()]
    for t in range((b.n + WAVE - 1) // WAVE):
        i = min(t * WAVE + (t * 7) % WAVE, b.n - 1)
        frames[i] = z[t % len(z)]
    return pg.batch_from_frames(frames), prog


@functools.lru_cache(maxsize=None)
def row_expected(name, opt):
    b, prog = row_case(name)
    exp, _ = oracle_run(prog, b, pktin_opt=opt)
    exp.setflags(write=False)
    return exp


def cpu_info(prog, env):
    with knobs(env):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            return c.program_info()
        finally:
            c.close()


# --------------------------------------------------------------------- matrix
# kernel: (LT, DIV, NW, FM, CK) -- the generic instantiation launched, or for
# spec = True the shape and engine of the specialised kernel (last_launch()
# reports a tree plan's as DIV, FM -1).  spec: None = generic row
# (MI_CLS_JIT=0); True = the specialised kernel is waited for and launched;
# False = the program is flat but its shape has no specialised kernel.
Row = namedtuple("Row", "id prog env opt kernel spec")
OPT = CK.ALL_CK
NOJIT = {"MI_CLS_JIT": "0"}


def _g(id_, prog, kernel, env=None, opt=0):
    return Row(id_, prog, dict(NOJIT, **(env or {})), opt, kernel, None)


def _s(id_, prog, kernel, env=None, opt=0, spec=True):
    return Row(id_, prog, dict(env or {}), opt, kernel, spec)


def _wpb(w, **kw):
    return dict({"MI_CLS_WPB": str(w)}, **kw)


NOFLAT = {"MI_CLS_NO_FLAT": "1"}
FLAT_ENGINES = {0: ("c2", {}), 2: ("c3_8", {}), 3: ("c3_64", {"MI_CLS_NO_CAND1": "1"}),
                4: ("c3_64", {})}

ROWS = [
    # general kernels, no pktin options: mi_cls_k4 / k8 / k12 / k16.hip
    _g("k4_lds", "c3_64", (True, False, 4, -1, False), _wpb(4, **NOFLAT)),
    _g("k4_lds_div", "c3_64_root", (True, True, 4, -1, False), _wpb(4)),
    _g("k4_hbm_auto", "c4_3072", (False, False, 4, -1, False)),
    _g("k4_hbm_div_auto", "c4_3072_root", (False, True, 4, -1, False)),
    _g("k8_auto", "c4_2048", (True, False, 8, -1, False)),
    _g("k8_noflat", "c4_2048", (True, False, 8, -1, False), NOFLAT),
    _g("k8_div_auto", "c4_2048_root", (True, True, 8, -1, False)),
    _g("k12_noflat", "c4_1400", (True, False, 12, -1, False), NOFLAT),
    _g("k12_div_auto", "c4_1400_root", (True, True, 12, -1, False)),
    _g("k16_lds", "c3_64", (True, False, 16, -1, False), NOFLAT),
    _g("k16_lds_div", "c3_64_root", (True, True, 16, -1, False)),
    _g("k16_hbm", "c4_1400", (False, False, 16, -1, False), _wpb(16)),
    _g("k16_hbm_div", "c4_1400_root", (False, True, 16, -1, False), _wpb(16)),
    # flat kernels: mi_cls_kf.hip (4 waves), kf12, kf16
    _g("kf12_e4_auto", "c4_1400", (True, False, 12, 4, False)),
] + [
    _g(f"kf{w}_e{fm}", p, (True, False, w, fm, False), dict(e, **({} if w == 16 else _wpb(w))))
    for w in (4, 12, 16) for fm, (p, e) in sorted(FLAT_ENGINES.items())
] + [
    # pktin-option kernels: mi_cls_kc4.hip, kc16
    _g("kc4_lds", "c3_64", (True, False, 4, -1, True), _wpb(4), OPT),
    _g("kc4_lds_div", "c3_64_root", (True, True, 4, -1, True), _wpb(4), OPT),
    _g("kc4_hbm_auto", "c4_1400", (False, False, 4, -1, True), None, OPT),
    _g("kc4_hbm_div_auto", "c4_1400_root", (False, True, 4, -1, True), None, OPT),
    _g("kc16", "c3_64", (True, False, 16, -1, True), None, OPT),
    _g("kc16_div", "c3_64_root", (True, True, 16, -1, True), None, OPT),
    # specialised kernels: every shape spec_setup accepts
    _s("spec_flat16", "c3_64", (True, False, 16, 4, False)),
    _s("spec_flat12_auto", "c4_1400", (True, False, 12, 4, False)),
    _s("spec_flat12_e2", "c3_8", (True, False, 12, 2, False), _wpb(12)),
    _s("spec_flat4", "c3_64", (True, False, 4, 4, False), _wpb(4)),
    _s("spec_none_flat8_auto", "c4_2048", (True, False, 8, -1, False), spec=False),
    _s("spec_none_flat8", "c3_64", (True, False, 8, -1, False), _wpb(8), spec=False),
    _s("spec_plan16", "c5", (True, True, 16, -1, False)),
    _s("spec_plan12", "c5", (True, True, 12, -1, False), _wpb(12)),
    _s("spec_plan8", "c5", (True, True, 8, -1, False), _wpb(8)),
    _s("spec_plan4_hbm", "c5", (False, True, 4, -1, False), _wpb(4)),
    _s("spec_plan4_lds", "c2_tree", (True, True, 4, -1, False), _wpb(4)),
    _s("spec_ck_flat16", "c3_64", (True, False, 16, 4, True), None, OPT),
    _s("spec_ck_flat4", "c3_64", (True, False, 4, 4, True), _wpb(4), OPT),
    _s("spec_ck_plan16", "c2_tree", (True, True, 16, -1, True), None, OPT),
    _s("spec_ck_plan4_hbm", "c5", (False, True, 4, -1, True), None, OPT),
]

# compiled instantiations no program and knob can reach: (kernel, the line that
# excludes it).  None: 8- and 12-wave blocks fall back to 16 waves without LDS
# room, and the units compile exactly what that leaves.
UNREACHABLE = []


def compiled_instantiations():
    """(LT, DIV, NW, FM, CK) of every MI_LAUNCH((mi_cls_kernel<...>)) line of
    the kernel translation units; NW of the flat units is launch_fm's
    template argument."""
    out = set()
    tf = {"true": True, "false": False}
    for unit in ("k4", "k8", "k12", "k16", "kf", "kf12", "kf16", "kc4", "kc16"):
        with open(os.path.join(SRC, f"mi_cls_{unit}.hip")) as f:
            text = f.read()
        found = re.findall(r"MI_LAUNCH\(\(mi_cls_kernel<([^>]*)>\)", text)
        assert found, unit
        nws = re.findall(r"launch_fm<(\d+)>\(", text)
        for args in found:
            a = [x.strip() for x in args.split(",")]
            assert 3 <= len(a) <= 5, (unit, args)
            if a[2] == "NW":
                assert len(nws) == 1, (unit, nws)
                a[2] = nws[0]
            out.add((tf[a[0]], tf[a[1]], int(a[2]), int(a[3]) if len(a) > 3 else -1,
                     tf[a[4]] if len(a) > 4 else False))
    return out


def _define(text, name):
    return re.search(rf"^#define {name}\s+(.+?)\s*(?://.*)?$", text, re.M).group(1)


def test_constants_match_the_kernel_header():
    with open(os.path.join(SRC, "mi_cls_dev.h")) as f:
        h = f.read()
    assert int(_define(h, "WAVE")) == WAVE and int(_define(h, "RS")) == RS
    assert int(_define(h, "WIN")) == WIN and _define(h, "WROWS") == "(WIN / 4 + 1)"
    assert int(_define(h, "MAX_STATS_COS")) == MAX_STATS_COS
    assert int(_define(h, "MIN_WAVES_PER_EU")) == OCC
    assert _define(h, "CRC_WORDS") == "(CRC_Y1 + 64u)" and _define(h, "CRC_Y1") == "(CRC_YINV + 65u)"
    assert _define(h, "CRC_YINV") == "(CRC_Z + CRC_ZN)"
    assert int(_define(h, "CRC_Z").rstrip("u")) + int(_define(h, "CRC_ZN")) + 65 + 64 == CRC_WORDS
    with open(os.path.join(SRC, "mi_cls.hip")) as f:
        m = f.read()
    assert "LDS_CU = 160u * 1024u" in m and "atoi(e) : 20 * 1024" in m
    # the limits the shapes follow from
    assert [LDS_CU - st_of(w) for w in (16, 12, 8)] == [56188, 82588, 108988]


def test_matrix_lists_every_instantiation():
    compiled = compiled_instantiations()
    generic = {r.kernel for r in ROWS if r.spec is not True}
    unreachable = {k for k, _ in UNREACHABLE}
    assert not generic & unreachable
    assert compiled - generic - unreachable == set(), "compiled instantiations without a row"
    assert (generic | unreachable) - compiled == set(), "rows of kernels that are not compiled"
    assert len(compiled) == 30
    assert len({r.id for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_row_program_reaches_its_kernel_cpu(built, row):
    """program_info() on the CPU: the row's program under the row's knobs has
    the hot-region size, tree shape and engine from which pick_shape and the
    dispatch, restated above, arrive at the row's kernel."""
    _, prog = PROGRAMS[row.prog](64)
    info = cpu_info(prog, row.env)
    wpb = int(row.env.get("MI_CLS_WPB", 0))
    ck = row.opt != 0
    lt, div, nw, fm, kck = row.kernel
    assert kck == ck
    plan = row.prog in HAS_PLAN
    assert info["tree"] == (row.prog in HAS_PLAN or row.prog.endswith("_root"))
    if row.spec is True:
        assert spec_accepted(info, plan, wpb, ck), (info, pick_shape(hot_bytes(info), wpb, ck))
        assert pick_shape(hot_bytes(info), wpb, ck)[:2] == (nw, lt)
        assert (div, fm) == (info["tree"], info["flat_engine"])
    else:
        if row.spec is False:
            assert info["flat_engine"] >= 0 and not spec_accepted(info, plan, wpb, ck)
        assert generic_kernel(info, wpb, ck) == row.kernel, (info, hot_bytes(info))
    if "auto" in row.id:
        assert wpb == 0


def run_row(row):
    b, prog = row_case(row.prog)
    info = {}
    with knobs(row.env):
        if row.spec is False:
            # a flat program whose shape has no specialised kernel: gpu_run's
            # wait insists on one, so this row waits for itself
            c = cls.Classifier(gpu=0)
            try:
                c.apply(prog)
                if row.opt:
                    c.set_pktin_opt(row.opt)
                assert c.program_info()["flat_engine"] >= 0
                assert c.spec_wait() == 1
                got = classify_poisoned(c, b)
                info = c.last_launch()
            finally:
                c.close()
        else:
            got = gpu_run(prog, b, pktin_opt=row.opt, spec=row.spec is True, info=info)
    return b, got, info


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_row(built, gpu, row):
    b, got, ll = run_row(row)
    lt, div, nw, fm, ck = row.kernel
    seen = (ll["lds_hot"], ll["div"], ll["nw"], ll["flat_engine"], ll["ck"], ll["specialised"])
    assert seen == (lt, div, nw, fm, ck, row.spec is True), ll["name"]
    if nw == 16:
        assert ll["grid"] > 1
    assert_same(got, row_expected(row.prog, row.opt), b, f"{row.id}: {ll['name']}")


# ------------------------------------------------------- dynamic tile dealing
DEAL = [("w12", "c4_1400", 12, False), ("w8", "c4_2048", 8, False), ("w4_hbm", "c4_3072", 4, False),
        ("w12_div", "c4_1400_root", 12, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,prog_name,nw,div", DEAL, ids=[d[0] for d in DEAL])
def test_dynamic_tile_dealing(built, gpu, name, prog_name, nw, div):
    """A block deals its tiles 2 NW + k from its LDS counter once it owns more
    than 2 NW: a batch of (2 NW + 3) tiles per block of the largest grid, and
    37 packets, on the shapes the 1 M-packet cases (16 waves) never run."""
    import torch
    from oracle.oracle import Oracle
    _, prog0 = PROGRAMS[prog_name](64)
    info = cpu_info(prog0, NOJIT)
    s_nw, s_lt, per_cu = pick_shape(hot_bytes(info))
    assert s_nw == nw
    grid_max = torch.cuda.get_device_properties(0).multi_processor_count * per_cu
    n = (2 * nw + 3) * grid_max * WAVE + 37
    b, prog = PROGRAMS[prog_name](n)
    ll = {}
    with knobs(NOJIT):
        got = gpu_run(prog, b, info=ll)
    assert (ll["nw"], ll["lds_hot"], ll["div"], ll["specialised"]) == (nw, s_lt, div, False), ll["name"]
    assert ll["grid"] == grid_max
    assert (n + WAVE - 1) // WAVE > (2 * nw + 2) * ll["grid"]
    o = Oracle()
    o.apply(prog)
    assert_same(got, o.classify(b, threads=16), b, f"dealing {name}: {ll['name']}")


# --------------------------------------------- predictor state across launches
PRED_VALS = [bytes([0xC0 + k, 0x11 * (k + 1)]) for k in range(4)]


def _predictor_prog():
    """A flat program with a PMR_CUSTOM_FRAME term at byte 70 (so frames longer
    than 64 B need the far half of the window) and a dport rule."""
    prog = [R.cos("default", queue=1)] + [R.cos(f"c{k}", queue=10 + k) for k in range(5)]
    prog.append(("default", 0))
    for k, v in enumerate(PRED_VALS):
        prog.append(("pmr", [R.t_custom(R.PMR_CUSTOM_FRAME, 70, v, b"\xff\xff")], 0, 1 + k, 100 + k))
    prog.append(("pmr", [R.t_be16(R.PMR_UDP_DPORT, 4000)], 0, 5, 7))
    return prog


def _predictor_traffic(far, seed):
    """Config 5 style traffic (VLAN / QinQ, IPv4 / IPv6, UDP / TCP): 300-byte
    frames where far[i], four in five of them with one of the rules' values at
    bytes 70-71, and 60-byte IPv4 frames elsewhere."""
    n = far.shape[0]
    rng = np.random.default_rng(seed)
    b = pg.build_batch(np.where(far, 300, 60), ipver=np.where(far & (rng.random(n) < 0.2), 6, 4),
                       l4proto=np.where(rng.random(n) < 0.8, pg.IPPROTO_UDP, pg.IPPROTO_TCP),
                       sip4=rng.integers(0, 2 ** 32, n).astype(np.uint64),
                       dip4=rng.integers(0, 2 ** 32, n).astype(np.uint64),
                       sip6=rng.integers(0, 256, (n, 16)).astype(np.uint8),
                       dip6=rng.integers(0, 256, (n, 16)).astype(np.uint8),
                       sport=rng.integers(1024, 65535, n),
                       dport=np.where(rng.random(n) < 0.3, 4000, rng.integers(1024, 65535, n)),
                       ntags=np.where(rng.random(n) < 0.1, 2, 1), vid0=rng.integers(1, 4095, n),
                       vid1=rng.integers(1, 4095, n), seed=seed)
    pick = rng.integers(0, 5, n)
    at = np.nonzero(far & (pick < 4))[0]
    vals = np.frombuffer(b"".join(PRED_VALS), np.uint8).reshape(4, 2)
    o = b.off[at].astype(np.int64) + 70
    b.buf[o] = vals[pick[at], 0]
    b.buf[o + 1] = vals[pick[at], 1]
    return b


def _predictor_batches(n=2048):
    """Batch A of 60-byte frames, batch B of 300-byte frames whose bytes 70-71
    decide the CoS, batch C of A's and B's tiles in turn."""
    a = _predictor_traffic(np.zeros(n, bool), 61)
    bb = _predictor_traffic(np.ones(n, bool), 62)
    fc = [(a if (i // WAVE) % 2 == 0 else bb).frame(i) for i in range(n)]
    return {"A": a, "B": bb, "C": pg.batch_from_frames(fc)}


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False, True], ids=["generic", "spec"])
def test_predictor_state_across_launches(built, gpu, spec):
    """The window predictor's hint word and launch count live in the context:
    whether a launch's first tiles stage bytes 64.. depends on whether the
    launch before saw frames that needed them.  One Classifier, the orders
    far-after-near, far-after-far, near-after-far and both mixed."""
    prog, batches = _predictor_prog(), _predictor_batches()
    exp = {k: oracle_run(prog, b)[0] for k, b in batches.items()}
    assert len(np.unique(exp["B"]["cos"])) == 6 and len(np.unique(exp["A"]["cos"])) == 2
    with knobs({} if spec else NOJIT):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            info = c.program_info()
            assert not info["tree"] and info["flat_engine"] >= 0, info
            assert c.spec_wait() == (0 if spec else 1)
            for step, k in enumerate("ABBACAB"):
                got = classify_poisoned(c, batches[k])
                ll = c.last_launch()
                assert not ll["div"] and not ll["ck"] and ll["specialised"] == spec, ll["name"]
                assert_same(got, exp[k], batches[k], f"launch {step} ({k}) of ABBACAB: {ll['name']}")
        finally:
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False, True], ids=["generic", "spec"])
def test_predictor_turns_within_a_launch(built, gpu, spec):
    """A wave's predictor follows the tile it parsed last, so it only ever
    turns in a launch that gives a wave several tiles: the batch of the dealing
    cases, 2 NW + 3 tiles per block, each tile near or far at random (a wave's
    tiles lie a whole grid apart, so a regular pattern would hand every wave
    tiles of one kind)."""
    import torch
    from oracle.oracle import Oracle
    prog = _predictor_prog()
    nw, lt, per_cu = pick_shape(hot_bytes(cpu_info(prog, NOJIT)))
    grid_max = torch.cuda.get_device_properties(0).multi_processor_count * per_cu
    n = (2 * nw + 3) * grid_max * WAVE + 37
    rng = np.random.default_rng(64)
    far = np.repeat(rng.random((n + WAVE - 1) // WAVE) < 0.5, WAVE)[:n]
    b = _predictor_traffic(far, 65)
    ll = {}
    with knobs({} if spec else NOJIT):
        got = gpu_run(prog, b, spec=spec, info=ll)
    assert (ll["nw"], ll["lds_hot"], ll["div"], ll["ck"], ll["specialised"]) == (nw, lt, False, False, spec)
    assert ll["grid"] == grid_max
    o = Oracle()
    o.apply(prog)
    exp = o.classify(b, threads=16)
    assert len(np.unique(exp["cos"])) == 6
    assert_same(got, exp, b, f"near / far tiles: {ll['name']}")
