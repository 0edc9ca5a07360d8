"""The result records of mi_cls_kernel (store_rec, odp_amd/csrc/mi_cls_dev.h)
are written through L2 with 16-B buffer stores over a descriptor of exactly
the launch's n records.  The cases are those at which such a store can go
wrong: a record never written or written past 16 n (batch sizes around a tile
and around a block, in every block shape), a result array that is 16-B but not
line aligned, every kernel family (flat, general, tree, pktin options, linear
engine, specialised), a result array written by two launches in a row, and a
kernel that reads the records on the same stream with no host synchronisation
in between (write-through lines leave L2: the next kernel must still see
them).  Every record is compared bit for bit with the CPU oracle; the result
buffers are filled with poison first (tests.helpers.classify_poisoned).

Specialised kernels run in one child process (as tests/test_gpu_block_setup.py
does, and for its reason: the suite's process keeps a bounded number of them).
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from odp_amd import cls
from odp_amd import rules as R
from tests import chksum_frames as CK
from tests import enq_model as EM
from tests.helpers import POISON, assert_same, classify_poisoned, gpu_run, knobs, oracle_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64
NOJIT = {"MI_CLS_JIT": "0"}
N_MAX = 4160   # 65 tiles: four 16-wave blocks and a tile


def sizes_for(nw):
    """A lane, a tile less one, a tile, a tile and a lane, and a block's waves
    with one tile each, one wave with a second and a third of one lane: a
    partial last tile, waves with no tile, and waves whose only records are
    stored after the loop."""
    return (1, 63, 64, 65, WAVE * (nw + 1) + 1)


@functools.lru_cache(maxsize=None)
def flat_case():
    """Config 3's traffic under 64 of its rules (a flat program), N_MAX packets,
    and the oracle's records."""
    b, prog = R.config3(N_MAX, num_rules=64)
    exp, _ = oracle_run(prog, b)
    exp.setflags(write=False)
    return b, prog, exp


def _upload(batch, dev):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(batch.buf)).to(dev),
            torch.from_numpy(batch.off.astype(np.int32, copy=False).view(np.int32)).to(dev),
            torch.from_numpy(batch.len.astype(np.int16, copy=False).view(np.int16)).to(dev))


def _records(raw):
    return np.ascontiguousarray(raw).reshape(-1).view(R.RESULT_DTYPE).copy()


def _batch_sizes(nw, spec):
    b_all, prog, exp_all = flat_case()
    with knobs({"MI_CLS_WPB": str(nw)} if spec else dict(NOJIT, MI_CLS_WPB=str(nw))):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            assert c.spec_wait() == (0 if spec else 1)
            for n in sizes_for(nw):
                b = b_all.slice(0, n)
                got = classify_poisoned(c, b)
                ll = c.last_launch()
                assert (ll["nw"], ll["specialised"]) == (nw, spec), ll["name"]
                assert_same(got, exp_all[:n], b, f"n {n}: {ll['name']}")
        finally:
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [4, 8, 12, 16])
def test_batch_sizes(built, gpu, nw):
    """Generic kernels, every block shape (8 waves: the general kernel)."""
    _batch_sizes(nw, False)


# ------------------------------------------------------ the specialised kernels
SPEC_SHAPES = (4, 12, 16)   # flat programs have no specialised kernel in 8-wave blocks

_CHILD = """
import sys, traceback
sys.path.insert(0, {root!r})
from tests import test_gpu_record_stores as m
calls = [(nw, m._batch_sizes, (nw, True)) for nw in m.SPEC_SHAPES]
for cid, f, args in calls:
    try:
        f(*args)
        print("CASE ok", cid, flush=True)
    except BaseException:
        print("CASE failed", cid, flush=True)
        traceback.print_exc(file=sys.stdout)
print("CHILD done", flush=True)
"""


@functools.lru_cache(maxsize=None)
def specialised_child():
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    return r.returncode, r.stdout


def _child_case(cid):
    rc, out = specialised_child()
    assert rc == 0 and "CHILD done" in out, out[-3000:]
    assert f"CASE ok {cid}\n" in out, out[out.find(f"CASE failed {cid}"):][:3000] or out[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nw", SPEC_SHAPES)
def test_batch_sizes_specialised(built, gpu, nw):
    _child_case(nw)


# ------------------------------------------------------- unaligned result array
@pytest.mark.gpu
@pytest.mark.parametrize("shift", [16, 48, 112])
def test_unaligned_result_array(built, gpu, shift):
    """The array starts `shift` bytes into an allocation: 16-B aligned, not
    line aligned, so a wave's 1 KB of records straddles lines at both ends.
    The bytes in front of it and 1 KB behind it stay poison."""
    import torch
    dev = torch.device("cuda:0")
    b_all, prog, exp_all = flat_case()
    n, back = WAVE * 17 + 1, 1024
    b = b_all.slice(0, n)
    with knobs(NOJIT):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            t = _upload(b, dev)
            t_out = torch.full((shift + 16 * n + back,), POISON, dtype=torch.uint8, device=dev)
            assert t_out.data_ptr() % 128 == 0
            stream = torch.cuda.current_stream(dev).cuda_stream
            assert c.classify_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n,
                                     t_out.data_ptr() + shift, stream) == 0
            torch.cuda.synchronize(dev)
            name = c.last_launch()["name"]
        finally:
            c.close()
    raw = t_out.cpu().numpy()
    assert (raw[:shift] == POISON).all(), f"bytes in front of the array were written: {name}"
    assert (raw[shift + 16 * n:] == POISON).all(), f"bytes behind the array were written: {name}"
    assert_same(_records(raw[shift:shift + 16 * n]), exp_all[:n], b, f"shift {shift}: {name}")


# --------------------------------------------------------------- kernel families
@pytest.mark.gpu
def test_pktin_option_kernel(built, gpu):
    """Every checksum option (0x3C): the option kernels."""
    assert CK.ALL_CK == 0x3C
    b_all, prog, _ = flat_case()
    b = b_all.slice(0, WAVE * 17 + 1)
    exp, _ = oracle_run(prog, b, pktin_opt=CK.ALL_CK)
    ll = {}
    with knobs(NOJIT):
        got = gpu_run(prog, b, pktin_opt=CK.ALL_CK, info=ll)
    assert ll["ck"] and not ll["specialised"], ll["name"]
    assert_same(got, exp, b, ll["name"])


@pytest.mark.gpu
def test_tree_kernel(built, gpu):
    """A small CoS tree (config 2's rules under two aggregates): the tree kernels."""
    b, prog = R.config2(WAVE * 17 + 1, tree=True)
    exp, _ = oracle_run(prog, b)
    ll = {}
    with knobs(NOJIT):
        got = gpu_run(prog, b, info=ll)
    assert ll["div"] and not ll["specialised"], ll["name"]
    assert_same(got, exp, b, ll["name"])


@pytest.mark.gpu
def test_linear_engine(built, gpu):
    """No bit-vector blocks (MI_CLS_NO_BV): the general kernel's linear scan."""
    b_all, prog, exp_all = flat_case()
    n = WAVE * 17 + 1
    b = b_all.slice(0, n)
    ll = {}
    with knobs(dict(NOJIT, MI_CLS_NO_BV="1")):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            info = c.program_info()
        finally:
            c.close()
        assert info["bitmap"] == 0 and info["candidate"] == 0 and info["direct"] == 0, info
        got = gpu_run(prog, b, info=ll)
    assert not ll["specialised"] and not ll["div"] and ll["flat_engine"] in (-1, 1), ll["name"]
    assert_same(got, exp_all[:n], b, ll["name"])


# ---------------------------------------------------------------- reused buffers
@pytest.mark.gpu
def test_result_array_written_twice(built, gpu):
    """Two batches back to back on one stream into one result array: 65 packets
    after 4 160.  The first 65 records are the second batch's, the rest still
    the first's."""
    import torch
    dev = torch.device("cuda:0")
    b1, prog, exp1 = flat_case()
    lo = 3000
    b2 = b1.slice(lo, lo + 65)
    exp2 = exp1[lo:lo + 65]
    assert np.count_nonzero(exp2 != exp1[:65]) > 32
    with knobs(NOJIT):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            t1, t2 = _upload(b1, dev), _upload(b2, dev)
            t_out = torch.full((16 * (b1.n + 64),), POISON, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            for t, n in ((t1, b1.n), (t2, b2.n)):
                assert c.classify_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n,
                                         t_out.data_ptr(), stream) == 0
            torch.cuda.synchronize(dev)
            name = c.last_launch()["name"]
        finally:
            c.close()
    raw = t_out.cpu().numpy()
    assert (raw[16 * b1.n:] == POISON).all(), name
    got = _records(raw[:16 * b1.n])
    assert_same(got[:65], exp2, b2, f"second batch: {name}")
    assert_same(got[65:], exp1[65:], None, f"first batch's records behind the second's: {name}")


# ------------------------------------------------------------ device-side reader
@pytest.mark.gpu
def test_enqueue_plan_reads_the_records_on_the_stream(built, gpu):
    """Classify, then the enqueue plan of the records (mi_cls_enq_plan) on the
    same stream, no host synchronisation between them: the plan is that of
    tests/enq_model.py over the oracle's records only if the records written
    through L2 are visible to the kernel after."""
    import torch
    dev = torch.device("cuda:0")
    b, prog, exp = flat_case()
    n = b.n
    poison = 0xA5A5A5A5
    with knobs(NOJIT):
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            tab, _, _ = c.enq_table()
            ng = int(tab.ndst) + 2
            t = _upload(b, dev)
            t_res = torch.full((16 * n,), POISON, dtype=torch.uint8, device=dev)
            t_perm = torch.from_numpy(np.full(n + 1, poison, np.uint32).view(np.int32)).to(dev)
            t_gbeg = torch.from_numpy(np.full(ng + 1, poison, np.uint32).view(np.int32)).to(dev)
            t_ctr = torch.from_numpy(np.full(2 * (len(cls.ENQ_OUT_FIELDS) + 1), poison, np.uint32).view(np.int32)).to(dev)
            torch.cuda.synchronize(dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            assert c.classify_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n,
                                     t_res.data_ptr(), stream) == 0
            assert c.L.odp_amd_cls_enq_plan(c.pktio, t_res.data_ptr(), t[2].data_ptr(), n, C.byref(tab),
                                            t_perm.data_ptr(), t_gbeg.data_ptr(), t_ctr.data_ptr(),
                                            stream or None) == 0
            torch.cuda.synchronize(dev)
            name = c.last_launch()["name"]
        finally:
            c.close()
    assert_same(_records(t_res.cpu().numpy()), exp, b, name)
    perm = t_perm.cpu().numpy().view(np.uint32)
    gbeg = t_gbeg.cpu().numpy().view(np.uint32)
    out = t_ctr.cpu().numpy().view(np.uint32)
    assert perm[n] == poison and gbeg[ng] == poison and out[-1] == poison and out[-2] == poison
    ctr = {k: int(v) for k, v in zip(cls.ENQ_OUT_FIELDS, out[:-2].view(np.uint64))}
    eperm, egbeg, ectr = EM.plan(exp, b.len, EM.table_of(tab))
    assert ectr["delivered"] > n // 2
    assert ctr == ectr, (ctr, ectr)
    assert np.array_equal(gbeg[:ng], egbeg) and np.array_equal(perm[:n], eperm), name
