"""The block setup of mi_cls_kernel (odp_amd/csrc/mi_cls_dev.h): the hot
region, the CRC-32C tables and the L4 table are loaded as one bounded batch of
16-B pieces per thread ahead of the first window loads, every wave reaches
the barrier once, whether it has a tile or not.  The cases are those at which
a batched, bounded copy can go wrong; every record is compared bit for bit
with the CPU oracle through the poisoned result buffer of tests.helpers.

Pieces per thread: rule programs whose hot region has fewer 16-B pieces than
the block has threads, just under and just over 1x and 2x the thread count,
and the largest each block shape accepts (4 pieces per thread for 16 waves, 7
for 12, 14 for 8, 5 for the 20-KB cap of 4-wave blocks: the batch's bounds).
The rule counts are found on the CPU from program_info()["hot_words"] and the
piece counts asserted, so a change of the assembler cannot quietly empty a
case.  Past the bounds lies only a 4-wave block with MI_CLS_LDS_HOT_MAX raised
(the launcher reads it once per process): that case runs in a child process.

Specialised kernels: a process keeps a bounded number of them for its whole
life (mi_cls_spec.cpp, SPEC_CACHE_MAX), the suite runs in one process, and
its other modules have tests that insist on getting one.  So that this module
takes nothing from that budget, whatever the other modules need, it compiles
none in the suite's process: every case runs the generic kernel here
(MI_CLS_JIT=0, which requests no compilation, as does every probe of a
program's size), and its specialised variant in one of two child processes
with a cache of their own.  A child runs its cases once (specialised_child),
prints one line per case, and every test_specialised[...] case asserts its own
line, so the first case of a group carries the group's time.

hot_words that is not a multiple of 4: the joint groups' directory (one word
per group, mi_cls_asm.cpp emit_joints) is appended to the hot region behind
the last aligned block with nothing padded behind it, so a CoS tree whose
levels are joint groups can end on any word count.  odd_tree() builds one of
1 mod 4: the last 16-B piece then holds one word of the region and three of
what follows it in the program, and the dynamic LDS size is rounded up.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from odp_amd import cls
from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import chksum_frames as CK
from tests.helpers import assert_same, classify_poisoned, gpu_run, knobs, oracle_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64
NOJIT = {"MI_CLS_JIT": "0"}
# mi_cls.hip pick_shape: the CU's LDS less a block's static LDS (windows, stats
# histogram, L4 table, tile counter), and MI_CLS_LDS_HOT_MAX's default
LDS_CU = 160 * 1024
HOT_MAX = 20 * 1024
RS, WROWS = 66, 25
# Pieces per thread in the kernel's batch, by mi_cls_kernel's own formula
# (SETUP_HOT in mi_cls_dev.h, which this mirrors: a change there belongs here)
SETUP_HOT = {nw: 5 if nw == 4 else (LDS_CU - 4 * nw * RS * WROWS) // 16 // (nw * WAVE) + 1
             for nw in (4, 8, 12, 16)}
assert SETUP_HOT == {4: 5, 8: 14, 12: 7, 16: 4}


def st_of(w):
    return 4 * (w * RS * WROWS + 256 + 256 + 1)


def hot_limit(nw):
    """Most bytes of hot region a block of nw waves copies into LDS."""
    return HOT_MAX if nw == 4 else LDS_CU - st_of(nw)


GEN = {"c3": lambda n, k: R.config3(n, num_rules=k), "c4": lambda n, k: R.config4(n, num_rules=k)}


@functools.lru_cache(maxsize=None)
def pieces_of(gen, k):
    """16-B pieces of the hot region of generator gen's program with k rules."""
    with knobs(NOJIT):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(GEN[gen](WAVE, k)[1])
            info = c.program_info()
        finally:
            c.close()
    assert info["flat_engine"] >= 0 and not info["tree"]
    return (info["hot_words"] + 3) // 4


def rules_for(gen, target):
    """The largest rule count whose program has at most `target` pieces (the
    hot region grows with the rule count)."""
    lo, hi = 2, {"c3": 400, "c4": 3000}[gen]
    assert pieces_of(gen, lo) <= target < pieces_of(gen, hi), (gen, target)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pieces_of(gen, mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo


# id -> (waves per block, generator, target pieces, "under" | "over" | "max")
def _piece_cases():
    out = {}
    for nw, gen in ((4, "c3"), (16, "c4")):
        nt = nw * WAVE
        for mult in (1, 2):
            out[f"w{nw}_under{mult}x"] = (nw, gen, mult * nt, "under")
            out[f"w{nw}_over{mult}x"] = (nw, gen, mult * nt, "over")
    for nw in (4, 8, 12, 16):
        out[f"w{nw}_max"] = (nw, "c4", hot_limit(nw) // 16, "max")
    return out


PIECE_CASES = _piece_cases()
NEAR = 12   # pieces: a rule adds 2-3, so the nearest rule count lies within this


def piece_program(case):
    nw, gen, target, kind = PIECE_CASES[case]
    k = rules_for(gen, target)
    if kind == "over":
        k += 1
    p = pieces_of(gen, k)
    nt = nw * WAVE
    if kind == "over":
        assert target < p <= target + NEAR, (case, k, p)
    else:
        assert target - NEAR <= p <= target, (case, k, p)
    if kind == "max":
        # the last piece of the batch is used, and nothing lies past the batch
        assert (SETUP_HOT[nw] - 1) * nt < p <= SETUP_HOT[nw] * nt, (case, p)
        assert pieces_of(gen, k + 1) * 16 > hot_limit(nw)
    return nw, gen, k, p


def n_for(nw):
    return 2 * WAVE * nw + 3   # two tiles per wave of a block, and a tile of 3


@pytest.mark.parametrize("case", sorted(PIECE_CASES))
def test_piece_counts_cpu(built, case):
    """The rule counts the GPU cases use give the intended piece counts."""
    piece_program(case)


def odd_tree(n):
    """A CoS tree whose two levels are joint groups of two-term rules (VLAN id
    + protocol at the root, UDP dport + protocol below), and n frames of which
    most take a rule of each level."""
    nsub, nper = 7, 30
    prog = [R.cos("default", queue=1)]
    sub = [len(prog) + i for i in range(nsub)]
    prog += [R.cos(f"s{i}", queue=10 + i) for i in range(nsub)]
    leaf = [len(prog) + i for i in range(4)]
    prog += [R.cos(f"l{i}", queue=50 + i) for i in range(4)]
    prog.append(("default", 0))
    for i in range(nsub):
        prog.append(("pmr", [R.t_be16(R.PMR_VLAN_ID_0, 100 + 7 * i, 0x0FFF), R.t_u8(R.PMR_IPPROTO, 17)],
                     0, sub[i], 0))
    for i in range(nsub):
        for j in range(nper):
            prog.append(("pmr", [R.t_be16(R.PMR_UDP_DPORT, 4000 + 37 * j + i), R.t_u8(R.PMR_IPPROTO, 17)],
                         sub[i], leaf[(i + j) % 4], j + 1))
    rng = np.random.default_rng(301)
    i = rng.integers(0, nsub + 1, n)
    j = rng.integers(0, nper + 3, n)
    b = pg.build_batch(np.where(rng.random(n) < 0.5, 64, rng.integers(64, 400, n)), ipver=np.full(n, 4),
                       l4proto=np.where(rng.random(n) < 0.85, pg.IPPROTO_UDP, pg.IPPROTO_TCP),
                       sip4=rng.integers(0, 2 ** 32, n).astype(np.uint64),
                       dip4=rng.integers(0, 2 ** 32, n).astype(np.uint64),
                       sport=rng.integers(1024, 65535, n), dport=4000 + 37 * j + i,
                       ntags=np.full(n, 1), vid0=100 + 7 * i, vid1=np.full(n, 5), seed=302)
    return b, prog


def odd_tree_info():
    with knobs(NOJIT):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(odd_tree(WAVE)[1])
            return c.program_info()
        finally:
            c.close()


def test_odd_tree_is_not_whole_pieces(built):
    """The program of test_hot_words_not_a_multiple_of_4 ends inside a piece,
    has more pieces than a 4-wave block has threads, and is a tree of joint
    groups (the DIV kernels, which share the prologue)."""
    info = odd_tree_info()
    assert info["hot_words"] % 4 == 1 and info["hot_words"] > 4 * 4 * WAVE, info
    assert info["tree"] and info["joint_bitmap"] > 0, info


def _run(prog, b, env, spec, opt=0, want=None, what=""):
    """Generic (MI_CLS_JIT=0) or specialised run against the oracle; want:
    (waves per block, hot region in LDS) the launch must report."""
    ll = {}
    with knobs(dict(env) if spec else dict(NOJIT, **env)):
        got = gpu_run(prog, b, pktin_opt=opt, spec=spec, info=ll)
    assert ll["specialised"] == spec, ll["name"]
    if want is not None:
        assert (ll["nw"], ll["lds_hot"]) == want, ll["name"]
    exp, _ = oracle_run(prog, b, pktin_opt=opt)
    assert_same(got, exp, b, f"{what}: {ll['name']}")
    return got


# (the specialised variants run in child processes, see CHILD_CALLS)
PIECE_RUNS = [(c, False) for c in sorted(PIECE_CASES)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,spec", PIECE_RUNS, ids=[f"{c}-{'spec' if s else 'generic'}" for c, s in PIECE_RUNS])
def test_pieces_per_thread(built, gpu, case, spec):
    nw, gen, k, p = piece_program(case)
    b, prog = GEN[gen](n_for(nw), k)
    # 8 and 12 waves are what the launcher picks for these sizes; 4 and 16 are forced
    env = {} if nw in (8, 12) else {"MI_CLS_WPB": str(nw)}
    _run(prog, b, env, spec, want=(nw, True), what=f"{case}: {k} rules, {p} pieces")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False], ids=["generic"])   # specialised: CHILD_CALLS
@pytest.mark.parametrize("nw", [4, 16])
def test_few_pieces(built, gpu, nw, spec):
    """Config 2: 33 pieces, so most threads of a block copy nothing."""
    b, prog = R.config2(n_for(nw))
    with knobs(NOJIT):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            assert c.program_info()["hot_words"] == 132
        finally:
            c.close()
    _run(prog, b, {"MI_CLS_WPB": str(nw)}, spec, want=(nw, True), what=f"config 2, {nw} waves")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False], ids=["generic"])   # specialised: CHILD_CALLS
@pytest.mark.parametrize("nw", [4, 16])
def test_idle_waves(built, gpu, nw, spec):
    """Batches that leave waves of the block without a tile: they still copy
    their share of the hot region (two or three pieces per thread here: the
    programs of the "over" cases) and reach the barrier.  LDS is not cleared
    between launches, so before each size a launch of another program in the
    same block shape, with a larger hot region and a batch that fills every
    block slot of every CU, overwrites what the launch before left there: a
    piece a launch fails to copy cannot be made good by its predecessor's."""
    import torch
    _, gen, k, p = piece_program("w4_over2x" if nw == 4 else "w16_over1x")
    _, s_gen, s_k, s_p = piece_program(f"w{nw}_max")
    assert nw * WAVE < p < s_p
    sizes = (1, 63, 64, 65, WAVE * nw + 1, 2 * WAVE * nw + 3)
    b_all, prog = GEN[gen](max(sizes), k)
    # 16 waves of 64 lanes per CU, in either shape (mi_cls.hip pick_shape)
    n_scrub = torch.cuda.get_device_properties(0).multi_processor_count * 16 * WAVE
    s_b = R.config2(n_scrub)[0]
    dev = torch.device("cuda:0")
    s_t = [torch.from_numpy(np.ascontiguousarray(s_b.buf)).to(dev), torch.from_numpy(s_b.off.view(np.int32)).to(dev),
           torch.from_numpy(s_b.len.view(np.int16)).to(dev), torch.empty((n_scrub, 16), dtype=torch.uint8, device=dev)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    s_prog = GEN[s_gen](WAVE, s_k)[1]
    exp_all, _ = oracle_run(prog, b_all)
    # (a Classifier per launch: the process has one classification state, which a new Classifier starts afresh)
    for n in sizes:
        with knobs(dict(NOJIT, MI_CLS_WPB=str(nw))):
            c = cls.Classifier(gpu=0)
            try:
                c.apply(s_prog)
                assert c.classify_device(s_t[0].data_ptr(), s_t[1].data_ptr(), s_t[2].data_ptr(), n_scrub,
                                         s_t[3].data_ptr(), stream) == 0
                torch.cuda.synchronize(dev)
                sl = c.last_launch()
                assert (sl["nw"], sl["lds_hot"]) == (nw, True) and sl["grid"] * nw * WAVE == n_scrub // 16 * min(
                    16, LDS_CU // (st_of(nw) + s_p * 16) * nw), sl   # every block slot the shape has
            finally:
                c.close()
        with knobs({"MI_CLS_WPB": str(nw)} if spec else dict(NOJIT, MI_CLS_WPB=str(nw))):
            c = cls.Classifier(gpu=0)
            try:
                c.apply(prog)
                assert c.spec_wait() == (0 if spec else 1)
                b = b_all.slice(0, n)
                got = classify_poisoned(c, b)
                ll = c.last_launch()
                assert (ll["nw"], ll["lds_hot"], ll["specialised"]) == (nw, True, spec), ll["name"]
                assert_same(got, exp_all[:n], b, f"n {n}: {ll['name']}")
            finally:
                c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False], ids=["generic"])   # specialised: CHILD_CALLS
@pytest.mark.parametrize("nw", [4, 16])
def test_hot_words_not_a_multiple_of_4(built, gpu, nw, spec):
    """hot_words = 1 (mod 4): the last 16-B piece of the copy is partly past
    the region.  A CoS tree (DIV kernels; specialised: its tree plan)."""
    info = odd_tree_info()
    assert info["hot_words"] % 4 != 0
    b, prog = odd_tree(n_for(nw))
    got = _run(prog, b, {"MI_CLS_WPB": str(nw)}, spec, want=(nw, True),
               what=f"hot_words {info['hot_words']}, {nw} waves")
    assert len(np.unique(got["cos"])) >= 8   # default, sub-CoS and leaves were all reached


@pytest.mark.gpu
def test_hot_region_from_hbm(built, gpu):
    """A region over the 20-KB cap in 4-wave blocks is read from HBM: no copy."""
    k = rules_for("c4", HOT_MAX // 16) + 8
    assert pieces_of("c4", k) * 16 > HOT_MAX
    b, prog = R.config4(n_for(4), num_rules=k)
    _run(prog, b, {"MI_CLS_WPB": "4"}, False, want=(4, False), what="hot region in HBM")


_CHILD = """
import sys
sys.path.insert(0, {root!r})
from odp_amd import rules as R
from tests.helpers import assert_same, gpu_run, oracle_run
b, prog = R.config4({n}, num_rules={k})
ll = {{}}
got = gpu_run(prog, b, info=ll)
assert (ll["nw"], ll["lds_hot"], ll["specialised"]) == (4, True, False), ll["name"]
assert_same(got, oracle_run(prog, b)[0], b, ll["name"])
print("same", ll["name"])
"""


@pytest.mark.gpu
def test_region_past_the_batch(built, gpu):
    """MI_CLS_LDS_HOT_MAX raised (read once per process, hence the child): a
    4-wave block copies a region of more than 5 pieces per thread, so the loop
    behind the batch runs."""
    k = 1000
    p = pieces_of("c4", k)
    assert p > 2 * SETUP_HOT[4] * 4 * WAVE and p * 16 + st_of(4) <= LDS_CU
    env = dict(os.environ, MI_CLS_LDS_HOT_MAX=str(p * 16), MI_CLS_WPB="4", MI_CLS_JIT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, n=n_for(4), k=k)], env=env,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "same" in r.stdout, r.stdout[-3000:]


def _sctp_batch():
    """SCTP frames of every kind of length the CRC paths split differently
    (within the staged block, 64-B pieces with every tail, the cooperative
    path's 256 pieces, one lane per frame), valid and with a flipped byte."""
    rng = np.random.default_rng(132)
    lens = np.concatenate([np.arange(46, 46 + 200), rng.integers(246, 1515, 300),
                           [9001, 16400, 16417, 16418, 20000, 131]])
    n = lens.size
    b = pg.build_batch(lens, ipver=np.where((rng.random(n) < 0.3) & (lens >= 100), 6, 4),
                       l4proto=np.full(n, pg.IPPROTO_SCTP),
                       sip4=rng.integers(0, 2**32, n).astype(np.uint64),
                       dip4=rng.integers(0, 2**32, n).astype(np.uint64),
                       sip6=rng.integers(0, 256, (n, 16), dtype=np.uint8),
                       dip6=rng.integers(0, 256, (n, 16), dtype=np.uint8),
                       sport=rng.integers(1, 65535, n), dport=rng.integers(1, 65535, n), seed=13)
    pg.set_checksums(b)
    for i in range(0, n, 3):
        o, ln = int(b.off[i]), int(b.len[i])
        b.buf[o + ln - 1] ^= 0x81
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False], ids=["generic"])   # specialised: CHILD_CALLS
@pytest.mark.parametrize("nw", [4, 16])
def test_option_kernels(built, gpu, nw, spec):
    """pktin options 0x3C (every checksum): the CRC-32C tables arrive in the
    same batch, four pieces per thread in a 4-wave block and one in a 16-wave
    block, the last word on its own."""
    assert CK.ALL_CK == 0x3C
    b = _sctp_batch()
    _, prog = R.config3(WAVE, num_rules=64)
    got = _run(prog, b, {"MI_CLS_WPB": str(nw)}, spec, opt=CK.ALL_CK, want=(nw, True),
               what=f"options, {nw} waves")
    l4_bad = (got["err"] & CK.E_L4CK) != 0
    assert ((got["in_flags"] >> 31) & 1).any() and l4_bad.any() and not l4_bad.all()


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [4, 16])
def test_statistics(built, gpu, nw):
    """Per-CoS statistics on: the histogram is zeroed in the same setup."""
    from oracle.oracle import Oracle
    b, prog = R.config3(n_for(nw), num_rules=64)
    prog = [(op[0], op[1], dict(op[2], stats=1 if k % 3 == 0 else 0)) if op[0] == "cos" else op
            for k, op in enumerate(prog)]
    with knobs(dict(NOJIT, MI_CLS_WPB=str(nw))):
        c = cls.Classifier(gpu=0)
        o = Oracle()
        try:
            cos, _ = c.apply(prog)
            ocos, _ = o.apply(prog)
            exp = o.classify(b)
            for _ in range(2):
                got = classify_poisoned(c, b)
                assert_same(got, exp, b, f"stats, {nw} waves: {c.last_launch()['name']}")
            o.classify(b)
            assert c.last_launch()["nw"] == nw
            counted = [c.cos_stats_packets(h) for h in cos if h]
            assert counted == [o.stats_packets(oh) for h, oh in zip(cos, ocos) if h]
            assert sum(counted) > 0
        finally:
            c.close()


def _proto_frames():
    """One frame per IP protocol number 0..255, IPv4 and IPv6, each with 24
    bytes behind the IP header that read as a TCP, UDP and SCTP header."""
    l4 = pg.tcp(sport=4000, dport=5000) + bytes(4)
    frames = []
    for p in range(256):
        frames.append(pg.pad_to(pg.eth() + pg.ipv4(proto=p, payload_len=len(l4)) + l4, 60))
        frames.append(pg.eth(ethtype=pg.ETH_IPV6) + pg.ipv6(next_hdr=p, payload_len=len(l4)) + l4)
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False], ids=["generic"])   # specialised: CHILD_CALLS
@pytest.mark.parametrize("nw", [4, 16])
def test_l4_table_every_protocol(built, gpu, nw, spec):
    b = pg.batch_from_frames(_proto_frames())
    _, prog = R.config3(WAVE, num_rules=64)
    got = _run(prog, b, {"MI_CLS_WPB": str(nw)}, spec, want=(nw, True), what=f"protocols, {nw} waves")
    assert len(np.unique(got["in_flags"])) >= 8   # ICMP, IPIP, TCP, UDP, AH, ESP, SCTP, no-next, none


# The specialised variants: id -> (test, arguments after the fixtures), by
# block shape.  A child calls the test functions above directly.  (Flat
# programs have no specialised kernel in 8-wave blocks.)
def _child_calls(shapes):
    out = {f"pieces-{c}": ("test_pieces_per_thread", (c, True))
           for c in sorted(PIECE_CASES) if PIECE_CASES[c][0] in shapes}
    for name in ("test_few_pieces", "test_idle_waves", "test_hot_words_not_a_multiple_of_4", "test_option_kernels",
                 "test_l4_table_every_protocol"):
        for nw in (4, 16):
            if nw in shapes:
                out[f"{name[5:]}-w{nw}"] = (name, (nw, True))
    return out


CHILD_CALLS = {"w4": _child_calls((4,)), "w12_w16": _child_calls((12, 16))}
CHILD_IDS = [(g, i) for g in sorted(CHILD_CALLS) for i in CHILD_CALLS[g]]

_CHILD_SPEC = """
import sys, traceback
sys.path.insert(0, {root!r})
from tests import test_gpu_block_setup as m
for cid, (name, args) in m.CHILD_CALLS[{group!r}].items():
    try:
        getattr(m, name)(True, None, *args)
        print("CASE ok", cid, flush=True)
    except BaseException:
        print("CASE failed", cid, flush=True)
        traceback.print_exc(file=sys.stdout)
print("CHILD done", flush=True)
"""


@functools.lru_cache(maxsize=None)
def specialised_child(group):
    """Runs the group's cases in one child process, once: its output."""
    r = subprocess.run([sys.executable, "-c", _CHILD_SPEC.format(root=ROOT, group=group)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    return r.returncode, r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("group,cid", CHILD_IDS, ids=[i for _, i in CHILD_IDS])
def test_specialised(built, gpu, group, cid):
    rc, out = specialised_child(group)
    assert rc == 0 and "CHILD done" in out, out[-3000:]
    assert f"CASE ok {cid}\n" in out, out[out.find(f"CASE failed {cid}"):][:3000] or out[-3000:]
