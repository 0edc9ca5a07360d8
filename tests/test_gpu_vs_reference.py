"""The kernels against the reference's OWN compiled parser, checksum and
classifier code (oracle/_ref/libodp_ref.so, oracle/reflib.py), with no oracle
in between: a misreading of the reference that the oracle and a kernel share
shows here.  The corpora, the comparison and its one masked field (`cos` of a
COS_DROP record) are those of tests/test_oracle_vs_reference.py
(tests/ref_cases.py); the classifier runs at the reference's compile-time
limits (64 CoS, 256 PMRs, 8 PMRs per CoS) into poisoned result buffers.

The library is built where the reference tree is present and travels with the
working tree: nothing here reads the reference tree.
"""
import functools

import numpy as np
import pytest

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import parse_model as PM
from tests import ref_cases as RC
from tests.helpers import gpu_run, knobs
from tests.ref_cases import assert_same_ref
from tests.test_gpu_parity import ENGINE_ENV

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=8)
def _reference(key, opt=0):
    """The reference's records for one corpus, computed once for all the
    engines and left unchanged."""
    from oracle.reflib import Reference
    prog, frames = _corpus(key)
    r = Reference(pktin_opt=opt)
    r.apply(prog)
    exp = r.classify(pg.batch_from_frames(frames))
    exp.flags.writeable = False
    return exp


def _corpus(key):
    from tests import zoo
    if key == "edge":
        return RC.edge_program(), list(RC.edge_frames())
    if key == "chksum":
        return zoo.prog_everything(), RC.chksum_corpus()
    return RC.fuzz_case(key)


@pytest.mark.parametrize("engine", ["auto", "spec", "nojit", "linear", "wpb4"])
@pytest.mark.parametrize("seed", RC.GPU_FUZZ_SEEDS)
def test_classify_fuzz(built, gpu, seed, engine):
    prog, frames = _corpus(seed)
    b = pg.batch_from_frames(frames)
    with knobs(ENGINE_ENV[engine]):
        got = gpu_run(prog, b, limits=RC.LIMITS, spec=engine == "spec")
    assert_same_ref(got, _reference(seed), b, f"fuzz seed {seed} [{engine}]", who="gpu")


@pytest.mark.parametrize("engine", ["auto", "spec", "nojit", "linear", "wpb4"])
def test_classify_edge_frames(built, gpu, engine):
    prog, frames = _corpus("edge")
    b = pg.batch_from_frames(frames)
    with knobs(ENGINE_ENV[engine]):
        got = gpu_run(prog, b, limits=RC.LIMITS, spec=engine == "spec")
    assert_same_ref(got, _reference("edge"), b, f"edge frames [{engine}]", who="gpu")


@pytest.mark.parametrize("name", ["all_ck", "all_ck_drop"])
def test_checksum_options(built, gpu, name):
    """The plain (not specialised) option kernel on the checksum corpus."""
    prog, frames = _corpus("chksum")
    b = pg.batch_from_frames(frames)
    info = {}
    with knobs(ENGINE_ENV["nojit"]):
        got = gpu_run(prog, b, limits=RC.LIMITS, pktin_opt=RC.OPTS[name], info=info)
    assert info["ck"] and not info["specialised"], info
    exp = _reference("chksum", RC.OPTS[name])
    assert_same_ref(got, exp, b, f"checksum corpus / {name}", who="gpu")
    assert (exp["in_flags"] >> 30).any() and (exp["err"] & (RC.CK.E_L3CK | RC.CK.E_L4CK)).any()


@pytest.fixture(scope="module")
def ctx(built, gpu):
    from odp_amd.cls import ParseContext
    c = ParseContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("off", [0, 2, 19])
def test_parse_kernel(ctx, off):
    """mi_cls_parse against odp_packet_parse: the zoo, 500 mutations and the
    edge frames behind `off` filler bytes, from every start protocol, at
    layers L3 and ALL, checksums off and all on."""
    frames = [PM.shifted(f, off) for f in RC.parse_frames(500)]
    offs = [off] * len(frames)
    batch = PM.batch_at(frames, offs)
    for proto in (PM.PROTO_ETH, PM.PROTO_IPV4, PM.PROTO_IPV6):
        for layer, sel in ((PM.ALL, 0), (PM.ALL, 0xF), (PM.L3, 0xF)):
            got = ctx.parse(batch, proto, layer, sel)
            exp = RC.ref_parse_records(frames, offs, proto, layer, sel)
            assert_same_ref(got, exp, batch, f"offset {off} proto {proto} layer {layer} chksums {sel:#x}",
                            who="gpu")
