"""The transmit models against the reference's OWN compiled transmit code
(oracle/_ref/libodp_ref.so: loopback_fix_checksums / check_proto and
get_dest_queue of pktio/loop.c behind oracle/ref_loop_shim.c, with
odp_packet.c's _odp_packet_*_chksum_insert): tests/tx_model.py (checksum
insertion) and tests/txq_model.py (the pktin flow hash) over the transmit
corpus of tests/tx_ref_cases.py, which also states the comparison and its
documented deviations.  A misreading of the reference that a
model and a kernel share shows here; the kernels themselves are held to the
same library in tests/test_gpu_tx_vs_reference.py.

The library is built where the reference tree is present and travels with the
working tree; a recorded fixture (tests/golden/tx_reference.json, written by
tools/make_tx_golden.py) holds the models to the same answers without it.
Not covered here, pinned by fixtures only: LSO.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import tx_model as TX
from tests import tx_ref_cases as TC
from tests import txq_model as TQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tx_reference.json")
DONE_OF = {TC.UDP: TX.DONE_UDP, TC.TCP: TX.DONE_TCP, TC.SCTP: TX.DONE_SCTP}


def test_corpus():
    """The corpus builds (its floors are asserted where it is built), is a
    few thousand cases, and never asks the reference for what it cannot do."""
    cs = TC.cases()
    assert 3000 <= len(cs) <= 6000
    assert len(TC.hash_slice()) == TC.HASH_SLICE
    assert {c.group for c in TC.hash_slice()} >= {"valid", "lengths", "padded", "overrides", "meta16"}
    assert all(TC.ref_defined(c) for c in cs)


def check_done(c, opt, got, done):
    """The done bits have no counterpart in the reference: they must name
    what the insertion computed -- a bit is set exactly where the decision
    (protocol, configuration, contract) leads to a store, and the bytes of
    every field whose bit is clear are unchanged."""
    info = TC.ip_info(c.frame, c.l3)
    changed = [i for i in range(len(got)) if got[i] != c.frame[i]]
    allowed = set()
    if done & TX.DONE_IPV4:
        assert info is not None and info[0]
        allowed |= {c.l3 + 10, c.l3 + 11}
    l4 = done & (TX.DONE_UDP | TX.DONE_TCP | TX.DONE_SCTP)
    if l4:
        assert info is not None and l4 == DONE_OF.get(info[1]) and TC.l4_wanted(c, opt), (c, done)
        assert TC.deviation(c) is None
        at, size = {TX.DONE_UDP: (6, 2), TX.DONE_TCP: (16, 2), TX.DONE_SCTP: (8, 4)}[l4]
        allowed |= set(range(c.l4 + at, c.l4 + at + size))
    elif info is not None and TC.l4_wanted(c, opt) and TC.deviation(c) is None and c.l4 != TC.INVALID:
        raise AssertionError(f"no L4 done bit for {c}")
    assert set(changed) <= allowed, (c, done, changed)


def test_insert_vs_reference(built):
    """TX.insert against ref_tx_fix_checksums over the whole corpus and all
    option rows, by assert_same_tx; the done bits against what the model
    changed; the masked share and the three deviations' counts."""
    cs = TC.cases()
    tally = TC.Tally()
    wrote = 0
    for opt in TC.OPT_ROWS:
        ref = TC.ref_fix(cs, opt)
        for c, r in zip(cs, ref):
            got, done = TX.insert(c.frame, c.l3, c.l4, c.flags & 0xF, opt)
            TC.assert_same_tx(got, c, opt, "tx_model", r, tally)
            check_done(c, opt, got, done)
            wrote += r != c.frame
    print(f"corpus {len(cs)} cases x {len(TC.OPT_ROWS)} option rows: {tally.compared} comparisons, "
          f"{sum(tally.masked.values())} masked {dict(tally.masked)}, reference wrote {wrote} frames")
    assert tally.compared == len(cs) * len(TC.OPT_ROWS) and wrote > tally.compared // 4
    tally.check()


def test_udp_zero_stored_as_ffff(built):
    """The computed-zero frames, with the reference alone: the stored field
    comes out 0xFFFF."""
    cs = [c for c in TC.cases() if c.group == "udp_zero"]
    assert sum(1 for c in cs if c.frame[c.l3] >> 4 == 4) >= 4 and sum(1 for c in cs if c.frame[c.l3] >> 4 == 6) >= 4
    for c, r in zip(cs, TC.ref_fix(cs, TX.CK_UDP)):
        assert r[c.l4 + 6:c.l4 + 8] == b"\xff\xff", c
        assert r[:c.l4 + 6] == c.frame[:c.l4 + 6] and r[c.l4 + 8:] == c.frame[c.l4 + 8:]


def _model_hashes(cs, hp, frames=None):
    frames = [c.frame for c in cs] if frames is None else frames
    return np.array([TQ.flow_hash(f, c.l3, c.l4, c.flags, hp)[0] for c, f in zip(cs, frames)], np.uint64)


def test_flow_hash_vs_reference(built):
    """TQ.flow_hash and TQ.dest_queue against ref_tx_dest_queue.

    The reference exposes only hash % num_qs.  The 32-bit hash is compared
    through six calls per packet with num_qs in {64, 63, 61, 59, 55, 53}:
    these are pairwise coprime, none exceeds the loop pktio's 64 queues, and
    their product 42 300 054 720 exceeds 2^32, so by the Chinese remainder
    theorem agreement on all six residues is agreement on all 32 bits.
    hash_proto 0, 63 and each single bit over the whole corpus, all 64 values
    over a 200-case slice, and the frames as the insertion leaves them; no
    case is masked."""
    prod = 1
    for m in TC.MODULI:
        assert m <= 64 and all(np.gcd(m, k) == 1 for k in TC.MODULI if k != m)
        prod *= m
    assert prod == 42300054720 > 2 ** 32
    cs = TC.cases()
    seen = set()
    for hp in TC.HP_ROWS:
        ref = TC.ref_queues(cs, hp, index=5)
        if hp == 0:
            exp = np.array([[TQ.dest_queue(0, m, 0, 5) for m in TC.MODULI]] * len(cs), np.uint8)
        else:
            h = _model_hashes(cs, hp)
            exp = TC.residues(h)
            seen |= {TQ.flow_hash(c.frame, c.l3, c.l4, c.flags, hp)[1] for c in cs}
            assert all(TQ.dest_queue(int(x), 64, hp, 5) == int(r[0]) for x, r in zip(h[:200], ref[:200]))
        bad = np.nonzero((exp != ref).any(axis=1))[0]
        assert bad.size == 0, (hp, bad[:8], cs[int(bad[0])], exp[bad[0]], ref[bad[0]])
    assert seen == {0, 4, 8, 12, 32, 36}
    sl = TC.hash_slice()
    for hp in range(64):
        ref = TC.ref_queues(sl, hp, index=3)
        exp = TC.residues(_model_hashes(sl, hp)) if hp else \
            np.array([[3 % m for m in TC.MODULI]] * len(sl), np.uint8)
        assert np.array_equal(exp, ref), (hp, np.nonzero((exp != ref).any(axis=1))[0][:8])
    # after the insertion (the reference fixes the checksums, then picks the queue)
    after = [TX.insert(c.frame, c.l3, c.l4, c.flags & 0xF, TX.ALL_TX)[0] for c in cs]
    for hp in (63, 32):
        assert np.array_equal(TC.residues(_model_hashes(cs, hp, after)), TC.ref_queues(cs, hp, frames=after))


# ------------------------------------------- the shim under host sanitizers
def test_tx_shim_sanitised(built, tmp_path):
    """The transmit entries of the shim as a stand-alone executable under
    AddressSanitizer and UBSan (oracle/Makefile ref-shim-main; no preloaded
    runtime): clean over the transmit corpus held in exact-size heap blocks,
    and the answers the library gives.

    One kind of case is kept out of this run only: the 12 IPv4 headers
    whose IHL nibble is 0.  packet_ipv4_chksum (odp_packet.c:1893-1898)
    declares a variable-length array of IHL x 2 elements before it checks
    IHL, and UBSan's bound check fires on the zero-length array ("variable
    length array bound evaluates to non-positive value 0"); the library runs
    above cover them."""
    from oracle import reflib
    from odp_amd._build import REF_SHIM_MAIN
    if not os.path.exists(REF_SHIM_MAIN):
        r = subprocess.run(["make", "-s", "-C", reflib.HERE, "ref-shim-main"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0 and "cannot find" in r.stdout:
            pytest.skip("no sanitiser runtime to link against")
    assert os.path.exists(REF_SHIM_MAIN), "oracle/_ref/ref_shim_main is missing: build() makes it"
    cs = [c for c in TC.cases() if not (TC.ip_info(c.frame, c.l3) is not None and c.frame[c.l3] == 0x40)]
    assert len(TC.cases()) - len(cs) == 12
    opts, hps = (TX.ALL_TX, TX.CK_UDP | TX.CK_IPV4, 0), (63, 0, 36)
    corpus, out = str(tmp_path / "tx_corpus.bin"), str(tmp_path / "tx_out.bin")
    given = [TC.ref_input(c) for c in cs]
    reflib.write_tx_corpus(corpus, [(f, c.l3, c.l4, c.flags) for f, c in zip(given, cs)],
                           [TX.all_bits(o) for o in opts], hps)
    r = subprocess.run([REF_SHIM_MAIN, corpus, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    with open(out, "rb") as f:
        raw = f.read()
    at = 0
    for opt in opts:
        for c, exp in zip(cs, TC.ref_fix(cs, opt)):
            got = TC.ref_output(c, raw[at:at + len(c.frame)])
            assert got == exp, (hex(opt), c)
            at += len(c.frame)
    for hp in hps:
        exp = TC.ref_queues(cs, hp, frames=given, index=5)
        got = np.frombuffer(raw[at:at + exp.size], np.uint8).reshape(exp.shape)
        assert np.array_equal(got, exp), hp
        at += exp.size
    assert at == len(raw)


# ------------------------------------------------------ the recorded fixture
def _golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["moduli"] == list(TC.MODULI) and 250 <= len(doc["cases"]) <= 400
    assert os.path.getsize(GOLDEN) < 1 << 20
    all_cases = TC.cases()
    cs, outs, queues = [], [], []
    for d in doc["cases"]:
        c = TC.Case(bytes.fromhex(d["frame"]), d["l3"], d["l4"], d["flags"], d["group"])
        assert all_cases[d["i"]] == c, "the corpus changed: run tools/make_tx_golden.py"
        cs.append(c)
        outs.append([c.frame if o is None else bytes.fromhex(o) for o in d["out"]])
        queues.append(d["queues"])
    assert {c.group for c in cs} == set(TC.FLOORS)
    return doc, cs, outs, np.array(queues, np.uint8)


def test_models_vs_recorded_reference():
    """The models against answers recorded from the reference's code: holds
    where libodp_ref.so was not built."""
    doc, cs, outs, queues = _golden()
    tally = TC.Tally()
    for k, opt in enumerate(doc["opts"]):
        for c, o in zip(cs, outs):
            got, done = TX.insert(c.frame, c.l3, c.l4, c.flags & 0xF, opt)
            TC.assert_same_tx(got, c, opt, "tx_model", o[k], tally)
            check_done(c, opt, got, done)
    assert sum(tally.masked.values()) * 10 <= tally.compared and len(tally.masked) == 3
    for k, hp in enumerate(doc["hash_protos"]):
        exp = TC.residues(_model_hashes(cs, hp)) if hp else \
            np.array([[doc["index"] % m for m in TC.MODULI]] * len(cs), np.uint8)
        assert np.array_equal(exp, queues[:, k, :]), hp


def test_recorded_reference_is_current(built):
    """The fixture is what the library gives today."""
    doc, cs, outs, queues = _golden()
    for k, opt in enumerate(doc["opts"]):
        assert TC.ref_fix(cs, opt) == [o[k] for o in outs], hex(opt)
    for k, hp in enumerate(doc["hash_protos"]):
        assert np.array_equal(TC.ref_queues(cs, hp, index=doc["index"]), queues[:, k, :]), hp
