"""Shared test helpers: run one rule program + batch through the HIP path and
the CPU oracle and compare every result record bit for bit."""
import contextlib
import os

import numpy as np

from odp_amd import rules as R


KNOBS = ("MI_CLS_NO_BV", "MI_CLS_DIV", "MI_CLS_WPB", "MI_CLS_NO_WIDE", "MI_CLS_NO_CAND1",
         "MI_CLS_NO_PORTMERGE", "MI_CLS_NO_FLAT", "MI_CLS_JIT", "MI_CLS_NO_JOINT", "MI_CLS_NO_PLAN")


@contextlib.contextmanager
def knobs(env):
    """The assembler's and launcher's environment knobs set to exactly env
    (every other knob unset) inside the block, the caller's values after it."""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def oracle_run(prog, batch, limits=(255, 8192, 4096), pktin_opt=0):
    from oracle.oracle import Oracle
    o = Oracle(limits=limits, pktin_opt=pktin_opt)
    o.apply(prog)
    return o.classify(batch), o


POISON = 0xA5   # fills the result buffer before a launch: outcome 0xA5 is no outcome
GUARD = 64      # records past the batch's that must stay poison


def classify_poisoned(c, batch, device="cuda:0"):
    """Classify a batch on Classifier c as c.classify uploads it, into a buffer
    of batch.n + GUARD records filled with POISON bytes: a record the kernel
    never stores stays poison (torch.empty would hand back the block an earlier
    launch filled with the right records) and a store past the batch shows in
    the guard.  Returns the batch's records."""
    import torch
    dev = torch.device(device)
    n = batch.n
    t_buf = torch.from_numpy(np.ascontiguousarray(batch.buf)).to(dev)
    t_off = torch.from_numpy(batch.off.astype(np.int32, copy=False).view(np.int32)).to(dev)
    t_len = torch.from_numpy(batch.len.astype(np.int16, copy=False).view(np.int16)).to(dev)
    t_out = torch.full((n + GUARD, 16), POISON, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = c.classify_device(t_buf.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n,
                           t_out.data_ptr(), stream)
    if rc != 0:
        raise RuntimeError(f"odp_amd_cls_classify: {rc} ({c.L.mi_cls_strerror(rc).decode()})")
    torch.cuda.synchronize(dev)
    raw = t_out.cpu().numpy()
    over = np.nonzero((raw[n:] != POISON).any(axis=1))[0]
    assert over.size == 0, (f"{over.size} records stored past the batch's {n}; first at "
                            f"{n + int(over[0])}: {raw[n + int(over[0])].tobytes().hex()}")
    unwritten = np.nonzero((raw[:n] == POISON).all(axis=1))[0]
    assert unwritten.size == 0, (f"{unwritten.size} of {n} records never written (still 0xA5 "
                                 f"poison); first at {int(unwritten[0])}, last at "
                                 f"{int(unwritten[-1])}; launch {c.last_launch()['name']}")
    return raw[:n].reshape(-1).view(R.RESULT_DTYPE).copy()


def gpu_run(prog, batch, limits=(255, 8192, 4096), pktin_opt=0, spec=False, info=None):
    """spec: wait for the program-specialised kernel before classifying (a
    flat program must get one); otherwise whichever kernel is ready.  info: a
    dict that receives the launch's last_launch()."""
    from odp_amd.cls import Classifier
    c = Classifier(gpu=0, limits=limits)
    try:
        c.apply(prog)
        if pktin_opt:
            c.set_pktin_opt(pktin_opt)
        if spec:
            rc = c.spec_wait()
            # a flat program always has one (trees: when the default CoS has a block)
            assert rc == 0 or (rc == 1 and c.program_info()["flat_engine"] < 0), rc
        got = classify_poisoned(c, batch)
        if info is not None:
            info.update(c.last_launch())
        return got
    finally:
        c.close()


def assert_same(got, exp, batch=None, what=""):
    assert got.shape == exp.shape, (got.shape, exp.shape)
    if np.array_equal(got, exp):
        return
    bad = np.nonzero(got != exp)[0]
    i = int(bad[0])
    msg = [f"{what}: {bad.size} of {got.size} records differ; first at {i}:",
           f"  gpu    {got[i]}", f"  oracle {exp[i]}"]
    if batch is not None:
        msg.append(f"  frame  {batch.frame(i).hex()}")
    raise AssertionError("\n".join(msg))


def summary(res):
    out = np.bincount(res["outcome"], minlength=5)
    return {"enq": int(out[R.OUT_ENQ]), "cos_drop": int(out[R.OUT_COS_DROP]),
            "discard": int(out[R.OUT_DISCARD]), "parse_drop": int(out[R.OUT_PARSE_DROP]),
            "loop": int(out[R.OUT_LOOP])}
