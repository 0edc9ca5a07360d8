"""The transmit kernels against the reference's OWN compiled transmit code
(oracle/_ref/libodp_ref.so: loopback_fix_checksums and get_dest_queue of
pktio/loop.c, oracle/ref_loop_shim.c), with no model in between: a misreading
of the reference that tests/tx_model.py or tests/txq_model.py shares with
mi_cls_tx_kernel shows here.  The corpus, the comparison and its documented
deviations are those of tests/test_tx_vs_reference.py (tests/tx_ref_cases.py,
DESIGN.md (c)).

The reference's answers are computed once per module on the CPU and cached.
The library is built where the reference tree is present and travels with the
working tree: nothing here reads the reference tree.
"""
import functools

import numpy as np
import pytest

from tests import tx_model as TX
from tests import tx_ref_cases as TC

pytestmark = pytest.mark.gpu

POISON = 0xA5A5A5A5


@pytest.fixture(scope="module")
def tx(built, gpu):
    from odp_amd.cls import TxContext
    c = TxContext(0)
    yield c
    c.close()


def _cases(key):
    """"all": the corpus; "slice": 300 cases spread over every group."""
    cs = TC.cases()
    return cs if key == "all" else cs[::len(cs) // 300][:300]


@functools.lru_cache(maxsize=None)
def _reference(key, opt):
    """Per case of one option row: what the kernel must leave (expected() of
    the reference's output frame) and the masked deviation, computed once."""
    cs = _cases(key)
    return tuple(TC.expected(c, r) for c, r in zip(cs, TC.ref_fix(cs, opt)))


@functools.lru_cache(maxsize=None)
def _ref_queues(key, hp):
    q = TC.ref_queues(_cases(key), hp)
    q.flags.writeable = False
    return q


def check_frames(buf, b, cs, opt, ref, who, tally=None):
    """The whole buffer -- so a stray store shows -- against the reference's
    frames laid out as the batch is; a difference is reported by
    assert_same_tx for its case."""
    exp = b.buf.copy()
    for o, (e, kind), c in zip(b.off, ref, cs):
        exp[int(o):int(o) + len(e)] = np.frombuffer(e, np.uint8)
        if tally is not None:
            tally.compared += 1
            if kind is not None and TC.l4_wanted(c, opt):
                tally.masked[kind] += 1
    bad = np.nonzero(buf != exp)[0]
    if bad.size:
        i = int(np.searchsorted(b.off, int(bad[0]), side="right")) - 1
        o, n = int(b.off[i]), int(b.len[i])
        assert int(bad[0]) < o + n, f"{who}: byte {int(bad[0])} outside every frame was written (behind frame {i})"
        # the reference's own output for the message: expected() masks it again
        TC.assert_same_tx(bytes(buf[o:o + n]), cs[i], opt, who, TC.ref_fix([cs[i]], opt)[0])
        raise AssertionError(f"{who}: frame {i} differs")


def check_hash(h, cs, hp, ref, who):
    """All 32 bits through the six residues (see
    test_tx_vs_reference.test_flow_hash_vs_reference: six pairwise coprime
    moduli whose product exceeds 2^32)."""
    got = TC.residues(h)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, (who, hp, bad[:8], cs[int(bad[0])], hex(int(h[bad[0]])), got[bad[0]], ref[bad[0]])


def test_insert_whole_corpus(tx):
    """mi_cls_chksum_insert in device form over the whole corpus, one packed
    batch per option row; the masked share and the three deviations."""
    cs = TC.cases()
    b, desc = TC.batch_of(cs)
    tally = TC.Tally()
    for opt in TC.OPT_ROWS:
        buf, _ = tx.insert(b, desc, opt)
        check_frames(buf, b, cs, opt, _reference("all", opt), f"gpu insert opt {opt:#x}", tally)
    print(f"{tally.compared} comparisons, masked {dict(tally.masked)}")
    assert tally.compared == len(cs) * len(TC.OPT_ROWS)
    tally.check()


def test_insert_unaligned(tx):
    """The same corpus at arbitrary byte offsets of the batch."""
    cs = TC.cases()
    b, desc = TC.batch_of(cs, unaligned_seed=8)
    assert (b.off % 4 != 0).sum() > len(cs) // 2
    for opt in TC.OPT_ROWS:
        buf, _ = tx.insert(b, desc, opt)
        check_frames(buf, b, cs, opt, _reference("all", opt), f"gpu insert unaligned opt {opt:#x}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(tx, n):
    cs = _cases("slice")[:n]
    ref = _reference("slice", TX.ALL_TX)[:n]
    b, desc = TC.batch_of(cs)
    buf, _ = tx.insert(b, desc, TX.ALL_TX)
    check_frames(buf, b, cs, TX.ALL_TX, ref, f"gpu insert n={n}")
    buf, done, h = tx.hash(b, desc, 63, opt=TX.ALL_TX, chksum=True, poison=POISON)
    check_frames(buf, b, cs, TX.ALL_TX, ref, f"gpu hash + insert n={n}")
    check_hash(h, cs, 63, TC.ref_queues(cs, 63, frames=TC.frames_of(b, buf)), f"n={n}")
    buf, done, h = tx.hash(b, desc, 63, poison=POISON)
    assert np.array_equal(buf, b.buf)
    check_hash(h, cs, 63, _ref_queues("slice", 63)[:n], f"alone n={n}")


def test_hash_alone(tx):
    """mi_cls_tx_hash alone: every hash against get_dest_queue, the hash
    buffer poisoned before every launch, no frame byte written, done bytes
    zero.  hash_proto 63 and each single bit over the whole corpus packed and
    at arbitrary offsets, all 63 non-zero values over a 200-case slice."""
    cs = TC.cases()
    for b, desc in (TC.batch_of(cs), TC.batch_of(cs, unaligned_seed=9)):
        for hp in TC.HP_ROWS[1:]:
            buf, done, h = tx.hash(b, desc, hp, poison=POISON)
            check_hash(h, cs, hp, _ref_queues("all", hp), "gpu hash alone")
            assert np.array_equal(buf, b.buf), "the hash alone wrote a frame byte"
            assert not done.any()
    sl = TC.hash_slice()
    b, desc = TC.batch_of(sl)
    for hp in range(1, 64):
        buf, done, h = tx.hash(b, desc, hp, poison=POISON)
        check_hash(h, sl, hp, TC.ref_queues(sl, hp), "gpu hash alone, slice")
        assert np.array_equal(buf, b.buf) and not done.any()


@pytest.mark.parametrize("hp,opt", [(63, TX.ALL_TX), (32, TX.ALL_TX), (63, TX.CK_UDP | TX.CK_IPV4), (5, 0xFF),
                                    (36, 0)])
def test_hash_with_checksums(tx, hp, opt):
    """mi_cls_tx_hash with checksums: the frames are the reference's, and the
    hash is get_dest_queue's over the frames as the launch left them (the
    reference fixes the checksums, then picks the queue: loop.c:581-582)."""
    cs = TC.cases()
    ref = _reference("all", opt)
    for b, desc in (TC.batch_of(cs), TC.batch_of(cs, unaligned_seed=10)):
        buf, done, h = tx.hash(b, desc, hp, opt=opt, chksum=True, poison=POISON)
        check_frames(buf, b, cs, opt, ref, f"gpu hash + insert hp {hp} opt {opt:#x}")
        check_hash(h, cs, hp, TC.ref_queues(cs, hp, frames=[e for e, _ in ref]), "gpu hash + insert")
        ibuf, idone = tx.insert(b, desc, opt)
        assert np.array_equal(done, idone)


@pytest.mark.parametrize("submit", [False, True])
def test_host_entries(tx, submit):
    """mi_cls_chksum_insert_host and mi_cls_tx_hash_host (staged from pageable
    memory), the plain call and the submit / wait pair, on a 300-case slice."""
    cs = _cases("slice")
    ref = _reference("slice", TX.ALL_TX)
    b, desc = TC.batch_of(cs)
    n = b.n
    off, ln = b.off.astype(np.uint32), b.len.astype(np.uint16)
    buf, d, done = b.buf.copy(), desc.copy(), np.zeros(n, np.uint8)
    tx.insert_host(buf, off, ln, d, TX.ALL_TX, done, submit=submit)
    check_frames(buf, b, cs, TX.ALL_TX, ref, "insert_host")
    for ck in (False, True):
        buf, d = b.buf.copy(), desc.copy()
        h, done = np.full(n, POISON, np.uint32), np.full(n, 0xEE, np.uint8)
        tx.hash_host(buf, off, ln, d, 63, h, opt=TX.ALL_TX, chksum=ck, done=done, submit=submit)
        if ck:
            check_frames(buf, b, cs, TX.ALL_TX, ref, "hash_host with checksums")
            check_hash(h, cs, 63, TC.ref_queues(cs, 63, frames=[e for e, _ in ref]), "hash_host with checksums")
        else:
            assert np.array_equal(buf, b.buf) and not done.any()
            check_hash(h, cs, 63, _ref_queues("slice", 63), "hash_host")
