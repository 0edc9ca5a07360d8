"""Growth of a context's staging buffers under the pageable host forms of
checksum insertion, parse and LSO (the staging step they share): a small
batch, one past both capacities the buffers start with (4096 entries, 1 MiB
of frames), the small one again -- each equal to the device entry's result for
the same input, whole buffer included.  Then the same with the large batch
submitted while the small one's ticket is still unwaited: the growth that
first waits for the context's stream.
"""
import ctypes as C

import numpy as np
import pytest

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import lso_model as M
from tests import parse_model as PM
from tests import tx_model as TX

pytestmark = pytest.mark.gpu

SMALL, BIG = 8, 4097          # frames of 300 B: 4097 * 320 B of slots > 1 MiB
LSO_SMALL, LSO_BIG = 65, 830  # sources of 3 segments: 2n + nsegs = 5n > 4096 at 830
LSO_PROFILES = [(M.PROTO_CUSTOM, [(M.ADD_SEGMENT_NUM, 16, 2)])]


def _udp_batch(n):
    rng = np.random.default_rng(n)
    return pg.build_batch(np.full(n, 300), ipver=np.full(n, 4), l4proto=np.full(n, pg.IPPROTO_UDP),
                          sip4=rng.integers(0, 2**32, n).astype(np.uint64),
                          dip4=rng.integers(0, 2**32, n).astype(np.uint64),
                          sport=rng.integers(1, 65535, n), dport=rng.integers(1, 65535, n), seed=n)


class _Tx:
    """Each feature: its context class, an input of a size, the device
    entry's result, a pageable host call (submit: without the wait; returns
    the ticket and the arrays the call writes), the wait."""
    sizes = (SMALL, BIG)

    @staticmethod
    def context():
        from odp_amd.cls import TxContext
        return TxContext(0)

    @staticmethod
    def make(n):
        b = _udp_batch(n)
        return b, TX.make_desc(np.full(n, 14), np.full(n, 34), 0)

    @staticmethod
    def device(c, inp):
        return c.insert(inp[0], inp[1], TX.ALL_TX)

    @staticmethod
    def host(c, inp, submit):
        b, desc = inp
        buf, off, ln = b.buf.copy(), b.off.astype(np.uint32), b.len.astype(np.uint16)
        desc, done = desc.copy(), np.zeros(b.n, np.uint8)
        args = (c.ctx, buf.ctypes.data, buf.nbytes, off.ctypes.data, ln.ctypes.data, desc.ctypes.data, b.n,
                TX.ALL_TX, done.ctypes.data)
        t = C.c_uint64()
        rc = c.L.mi_cls_chksum_insert_host_submit(*args, C.byref(t)) if submit else c.L.mi_cls_chksum_insert_host(*args)
        assert rc == 0
        return t.value, (buf, done), (off, ln, desc)

    @staticmethod
    def wait(c, t):
        assert c.L.mi_cls_chksum_insert_host_wait(c.ctx, t) == 0


class _Parse(_Tx):
    @staticmethod
    def context():
        from odp_amd.cls import ParseContext
        return ParseContext(0)

    @staticmethod
    def make(n):
        return _udp_batch(n)

    @staticmethod
    def device(c, b):
        return (c.parse(b, PM.PROTO_ETH, PM.ALL, 0xF),)

    @staticmethod
    def host(c, b, submit):
        buf, off, ln = b.buf.copy(), b.off.astype(np.uint32), b.len.astype(np.uint16)
        out = np.zeros(b.n, R.RESULT_DTYPE)
        t = 0
        if submit:
            t = c.submit_host(buf, off, ln, out, PM.PROTO_ETH, PM.ALL, 0xF)
        else:
            c.parse_host(buf, off, ln, out, PM.PROTO_ETH, PM.ALL, 0xF)
        return t, (out,), (buf, off, ln)

    @staticmethod
    def wait(c, t):
        c.wait(t)


class _Lso(_Tx):
    sizes = (LSO_SMALL, LSO_BIG)

    @staticmethod
    def context():
        from odp_amd.cls import LsoContext
        return LsoContext(0)

    @staticmethod
    def make(n):
        rng = np.random.default_rng(n)
        # 22 B of headers + 578 B in segments of 200: three segments each
        lay = M.Layout([(bytes(rng.integers(0, 256, 600).astype(np.uint8)), 22, 200, 0, M.L3_INVALID)
                        for _ in range(n)], LSO_PROFILES)
        assert len(lay.seg) == 3 * n
        return lay

    @staticmethod
    def device(c, lay):
        from odp_amd.cls import lso_profiles
        return c.segment(lay.buf, lay.off, lay.len, lay.desc, lay.seg, lso_profiles(LSO_PROFILES))

    @staticmethod
    def host(c, lay, submit):
        from odp_amd.cls import lso_profiles
        prof = lso_profiles(LSO_PROFILES)
        buf, st = lay.buf.copy(), np.full(len(lay.desc), 0xEE, np.uint8)
        args = (c.ctx, buf.ctypes.data, buf.nbytes, lay.off.ctypes.data, lay.len.ctypes.data,
                lay.desc.ctypes.data, len(lay.desc), buf.ctypes.data, buf.nbytes, lay.seg.ctypes.data,
                len(lay.seg), C.cast(prof, C.c_void_p), len(prof), st.ctypes.data)
        t = C.c_uint64()
        rc = c.L.mi_cls_lso_segment_host_submit(*args, C.byref(t)) if submit else c.L.mi_cls_lso_segment_host(*args)
        assert rc == 0
        return t.value, (buf, st), (prof,)

    @staticmethod
    def wait(c, t):
        assert c.L.mi_cls_lso_segment_host_wait(c.ctx, t) == 0


_reference = {}


def _inputs(feature):
    """The feature's two inputs and the device entry's result for each,
    computed once (on a context of their own) and left unchanged."""
    if feature not in _reference:
        c = feature.context()
        try:
            inputs = [feature.make(n) for n in feature.sizes]
            _reference[feature] = [(inp, feature.device(c, inp)) for inp in inputs]
        finally:
            c.close()
    return _reference[feature]


def _same(got, exp, what):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and np.array_equal(g, e), what


@pytest.mark.parametrize("unwaited", [False, True], ids=["sync", "submit_over_unwaited"])
@pytest.mark.parametrize("feature", [_Tx, _Parse, _Lso], ids=["chksum", "parse", "lso"])
def test_staging_buffers_grow(built, gpu, feature, unwaited):
    (small, small_exp), (big, big_exp) = _inputs(feature)
    c = feature.context()
    try:
        t1, got1, keep1 = feature.host(c, small, submit=unwaited)
        t2, got2, keep2 = feature.host(c, big, submit=unwaited)   # grows both buffers
        if unwaited:
            assert (t1, t2) == (1, 2)
            feature.wait(c, t2)
            feature.wait(c, t1)
        _same(got1, small_exp, "small batch before the growth")
        _same(got2, big_exp, "large batch")
        _, got3, _ = feature.host(c, small, submit=False)
        _same(got3, small_exp, "small batch after the growth")
    finally:
        c.close()
