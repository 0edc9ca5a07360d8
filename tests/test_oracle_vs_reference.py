"""The CPU oracle against the reference's OWN compiled parser, checksum and
classifier code (oracle/_ref/libodp_ref.so: odp_parse.c, odp_packet.c,
odp_chksum.c, odp_hash_crc_gen.c, odp_classification.c and
arch/default/odp_hash_crc32.c, compiled unchanged; oracle/ref_shim.c).

Every GPU parity test compares a kernel with the oracle; this module is what
ties the oracle to the reference on the inputs where parsers and matchers go
wrong: mutated and truncated headers, masked terms on odd frames, first-match
order after pmr_destroy, checksum verdicts on malformed L4, error-CoS routing.

Every comparison is bit-exact on in_flags, err, outcome, cos, queue, mark,
l3_offset and l4_offset, with the oracle at the reference's compile-time
limits (64 CoS, 256 PMRs, 8 PMRs per CoS).

Field masking, by outcome only (tests/ref_cases.py): `cos` of a COS_DROP
record -- _odp_cls_classify_packet returns 1 for a drop CoS
(odp_classification.c:1754-1755) before it stores pkt_hdr->cos (:1761), so
the reference does not say which CoS dropped.  Nothing else is masked.

Not covered here, pinned by fixtures only: CoS cycles (the reference never
returns from one; the binding refuses them), limits above the stock ones, LSO.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import parse_model as PM
from tests import ref_cases as RC
from tests import refcases
from tests import zoo
from tests.ref_cases import assert_same_ref


def both(prog, batch, opt=0, what=""):
    """Oracle and reference over one program and batch: records, and which
    creates each side refused."""
    from oracle.oracle import Oracle
    from oracle.reflib import Reference
    o = Oracle(limits=RC.LIMITS, pktin_opt=opt)
    oc, op = o.apply(prog)
    r = Reference(pktin_opt=opt)
    rc, rp = r.apply(prog)
    assert [h != 0 for h in oc] == [h != 0 for h in rc], f"{what}: CoS creates refused differently"
    assert [h != 0 for h in op] == [h != 0 for h in rp], f"{what}: PMR creates refused differently"
    exp = r.classify(batch)
    assert_same_ref(o.classify(batch), exp, batch, what)
    return o, r, exp


def zoo_batch():
    return pg.batch_from_frames(list(RC.zoo_frames()))


# ------------------------------------------------------------- fixture rows
def test_binding_refuses_a_cos_cycle(built):
    """The reference never returns from a CoS cycle, so zoo.prog_loop stays
    pinned by the oracle alone: the binding must refuse it, not hang."""
    from oracle.reflib import Reference
    r = Reference()
    r.apply(zoo.prog_loop())
    with pytest.raises(ValueError, match="cycle"):
        r.classify(zoo_batch())


def test_golden_parser_frames(built):
    b = pg.batch_from_frames([f for _, f in zoo.golden_frames()])
    _, _, exp = both([R.cos("d", queue=1), ("default", 0)], b, what="golden parser frames")
    assert (exp["outcome"] == R.OUT_ENQ).all()


def test_zoo_no_rules(built):
    both([R.cos("d", queue=1), R.cos("e", queue=2), ("default", 0), ("error", 1)], zoo_batch(),
         what="zoo / no rules")


@pytest.mark.parametrize("name,term", zoo.term_examples(), ids=[n for n, _ in zoo.term_examples()])
def test_zoo_each_term(built, name, term):
    both(zoo.prog_single(term, mark=0x77), zoo_batch(), what=f"zoo / {name}")


@pytest.mark.parametrize("prog", ["prog_everything", "prog_deletes", "prog_no_default"])
def test_zoo_programs(built, prog):
    _, _, exp = both(getattr(zoo, prog)(), zoo_batch(), what=f"zoo / {prog}")
    if prog == "prog_everything":
        # (the default CoS takes 8 of its PMRs at these limits: both sides
        # must refuse the same rest, which both() asserts)
        out = np.bincount(exp["outcome"], minlength=4)
        assert out[R.OUT_COS_DROP] and out[R.OUT_PARSE_DROP] and len(np.unique(exp["cos"])) > 5
        assert (exp["queue"] > 0).any() and (exp["mark"] > 0).any()


@pytest.mark.parametrize("case", refcases.term_cases() + refcases.chain_cases(), ids=lambda c: c[0])
def test_refcases(built, case):
    name, prog, pkts = case
    b = pg.batch_from_frames([f for f, _ in pkts])
    _, _, exp = both(prog, b, what=name)
    # the reference test's own assertion (the reference names no CoS for a dropped packet)
    enq = exp["outcome"] != R.OUT_COS_DROP
    assert list(exp["cos"][enq]) == [e for (_, e), k in zip(pkts, enq) if k], name


@pytest.mark.parametrize("opt", [0, RC.OPTS["all_ck"], RC.OPTS["all_ck_drop"]], ids=["plain", "all_ck", "all_ck_drop"])
def test_edge_frames(built, opt):
    """Swept header fields (fragment words, tag words, IHL, data offset, UDP
    and IPv6 payload lengths) under rules on what they move."""
    b = pg.batch_from_frames(list(RC.edge_frames()))
    _, _, exp = both(RC.edge_program(), b, opt, "edge frames")
    if opt == 0:
        assert set(np.unique(exp["cos"])) >= {0, 1, 2, 3, 4, 5, 6, 7}
        assert (exp["queue"] > 0).any() and len(np.unique(exp["mark"])) >= 8


def _quirk_cases():
    """The Appendix-A quirk programs and frames of tests/test_oracle_golden.py,
    with the swap-on-delete and destroyed-default-CoS programs."""
    E = pg.eth()
    err = [R.cos("d", queue=1), R.cos("e", queue=2), ("default", 0), ("error", 1)]
    q1 = pg.udp4_frame(tags=(0x123,), tpids=[pg.ETH_QINQ], size=64)
    base = pg.udp4_frame(size=60)
    swap = [R.cos("d", queue=1), R.cos("a", queue=2), R.cos("b", queue=3), R.cos("c", queue=4),
            ("default", 0), ("pmr", [R.t_u8(R.PMR_IPPROTO, 99)], 0, 1, 0),
            ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 2048)], 0, 2, 0),
            ("pmr", [R.t_be16(R.PMR_UDP_SPORT, 1024)], 0, 3, 0)]
    hbh = [pg.pad_to(pg.eth(ethtype=pg.ETH_IPV6) + pg.ipv6(next_hdr=0, payload_len=plen) +
                     pg.ipv6_ext(pg.IPPROTO_UDP) + pg.udp(5, 6, 8), 120) for plen in (16, 64)]
    return [
        ("a6_tot_len_20", zoo.prog_single(R.t_be16(R.PMR_UDP_DPORT, 2048)),
         [pg.pad_to(E + pg.ipv4(tot_len=20) + pg.udp(1234, 2048), 60)], [1]),
        ("a7_nonfirst_frag", zoo.prog_single(R.t_be16(R.PMR_UDP_DPORT, 2048)),
         [pg.pad_to(E + pg.ipv4(frag=10, payload_len=26) + struct.pack("!HH", 7, 0x0800) + bytes(22), 60)],
         [1]),
        ("a15_qinq_one_tag_ipv4", zoo.prog_single(R.t_be16(R.PMR_ETHTYPE_X, pg.ETH_IPV4)), [q1], [0]),
        ("a15_qinq_one_tag_bytes", zoo.prog_single(R.t_be16(R.PMR_ETHTYPE_X,
                                                           struct.unpack("!H", q1[20:22])[0])), [q1], [1]),
        ("a16_custom_frame_gate", zoo.prog_single(R.t_custom(R.PMR_CUSTOM_FRAME, 58, base[58:60], b"\xff\xff")),
         [base, base + b"\x00"], [0, 1]),
        ("a9_ipv6_hbh_plen", err, hbh, [1, 0]),
        ("a10_truncated", err, [(E + pg.ipv4(tot_len=26) + bytes(6))[:40],
                                pg.pad_to(E + pg.ipv4(tot_len=200) + pg.udp(), 60)], [0xFF, 1]),
        ("a12_marked_match", [R.cos("d", queue=1), R.cos("m", queue=2), ("default", 0),
                              ("pmr", [R.t_u8(R.PMR_IPPROTO, 17)], 0, 1, 5)], [pg.udp4_frame()], [1]),
        ("swap_on_delete_before", swap, [pg.udp4_frame(sport=1024, dport=2048)], [2]),
        ("swap_on_delete_after", swap + [("pmr_destroy", 0)], [pg.udp4_frame(sport=1024, dport=2048)], [3]),
        ("destroyed_default_cos", [R.cos("d", queue=1), R.cos("x", queue=2), ("default", 0),
                                   ("pmr", [R.t_u8(R.PMR_IPPROTO, 17)], 0, 1, 0), ("cos_destroy", 0)],
         [pg.udp4_frame()], [0]),
    ]


@pytest.mark.parametrize("case", _quirk_cases(), ids=lambda c: c[0])
def test_appendix_a_quirks(built, case):
    """The quirks the oracle's own golden test asserts, asked of the reference
    itself (the expected CoS are those of tests/test_oracle_golden.py)."""
    name, prog, frames, want = case
    b = pg.batch_from_frames(frames)
    _, _, exp = both(prog, b, what=name)
    assert list(exp["cos"]) == want, name
    if name == "a12_marked_match":
        assert exp["in_flags"][0] == 0x402079 and exp["mark"][0] == 5


# ---------------------------------------------------------------- fuzz rows
def _fuzz(seed, dense):
    prog, frames = RC.fuzz_case(seed, dense)
    b = pg.batch_from_frames(frames)
    what = f"{'dense ' if dense else ''}fuzz seed {seed}"
    o, r, exp = both(prog, b, what=what)
    assert_same_ref(o.classify(b), r.classify(b), b, what + ", second pass")
    for i, (ho, hr) in enumerate(zip(o.cos, r.cos)):
        if hr:
            assert o.stats_packets(ho) == r.stats_packets(hr), f"{what}: packets of CoS {i}"
    return r, exp


@pytest.mark.parametrize("seed", RC.FUZZ_SEEDS)
def test_fuzz(built, seed):
    """A random CoS graph with deletes over the zoo and 3000 mutated frames:
    the same records, the same creates refused, the same per-CoS packet
    counters after two passes."""
    r, exp = _fuzz(seed, False)
    accepted = sum(h != 0 for h in r.pmr) / len(r.pmr)
    assert accepted >= RC.MIN_ACCEPTED, f"seed {seed}: the reference took {accepted:.0%} of the PMRs"
    assert len(np.unique(exp["cos"][exp["outcome"] == R.OUT_ENQ])) >= RC.MIN_COS


@pytest.mark.parametrize("seed", RC.DENSE_SEEDS)
def test_fuzz_dense(built, seed):
    """The same with 4..9 CoS: full rule lists on the CoS that packets reach
    (refused creates beyond 8 included), deeper chains."""
    _fuzz(seed, True)


def test_fuzz_dense_reaches_chains(built):
    """What the dense rows are for: PMR creates past a CoS's 8th are refused,
    and packets still arrive on several CoS of one program."""
    from oracle.reflib import Reference
    most, refused = 0, 0
    for seed in RC.DENSE_SEEDS:
        prog, frames = RC.fuzz_case(seed, True)
        r = Reference()
        r.apply(prog)
        exp = r.classify(pg.batch_from_frames(frames))
        most = max(most, len(np.unique(exp["cos"][exp["outcome"] == R.OUT_ENQ])))
        refused += sum(h == 0 for h in r.pmr)
    assert most >= RC.MIN_COS and refused > 0, (most, refused)


# -------------------------------------------------------- pktin option rows
@pytest.mark.parametrize("name", sorted(RC.OPTS))
def test_pktin_options_corpus(built, name):
    b = pg.batch_from_frames(RC.chksum_corpus())
    _, _, exp = both(zoo.prog_everything(), b, RC.OPTS[name], f"checksum corpus / {name}")
    if RC.OPTS[name] & RC.CK.ALL_CK:
        assert (exp["in_flags"] >> 30).any() and (exp["err"] & (RC.CK.E_L3CK | RC.CK.E_L4CK)).any()
    if RC.OPTS[name] & RC.CK.ALL_DROP:
        assert (exp["outcome"] == R.OUT_PARSE_DROP).sum() > 30


@pytest.mark.parametrize("proto", [pg.IPPROTO_UDP, pg.IPPROTO_TCP, pg.IPPROTO_SCTP], ids=["udp", "tcp", "sctp"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_pktin_options_valid_lengths(built, ipver, proto):
    """Valid checksums at every L4 length 12..395, a byte flipped in every
    third frame, under each option row."""
    b = RC.valid_chksum_batch(ipver, proto)
    prog = [R.cos("d", queue=1), R.cos("e", queue=2), ("default", 0), ("error", 1)]
    for name, opt in sorted(RC.OPTS.items()):
        _, _, exp = both(prog, b, opt, f"valid ipv{ipver} proto {proto} / {name}")
        if name == "all_ck":
            ok = np.ones(b.n, bool)
            ok[::3] = False
            assert ((exp["in_flags"][ok] >> 31) & 1).all() and (exp["err"][ok] == 0).all()
            assert (exp["err"][~ok] != 0).sum() > b.n // 6


# ------------------------------------------------------- odp_packet_parse rows
@pytest.mark.parametrize("layer", [PM.L2, PM.L3, PM.L4, PM.ALL])
@pytest.mark.parametrize("proto", [PM.PROTO_ETH, PM.PROTO_IPV4, PM.PROTO_IPV6])
def test_packet_parse(built, proto, layer):
    """tests/parse_model.parse (the model the parse kernel is compared with)
    against the reference's odp_packet_parse + odp_packet_parse_result: the
    zoo and 1000 mutations behind every offset of the reference's own
    l2_offset[] list, checksums off and all on."""
    from oracle import reflib
    frames = RC.parse_frames(1000)
    for off in sorted(set(PM.REF_OFFSETS)):
        for f in frames:
            sf = PM.shifted(f, off)
            for ck in (0, 0xF):
                ret, fl, err, l2, l3, l4 = PM.parse(sf, off, proto, layer, ck)
                p = reflib.packet_parse(sf, off, proto, layer, ck)
                got = (p.ret, p.in_flags, p.err, p.l2, p.l3, p.l4)
                assert (ret, fl, err, l2, l3, l4) == got, (
                    f"offset {off} chksums {ck:#x}: model {(ret, hex(fl), err, l2, l3, l4)} reference "
                    f"{(p.ret, hex(p.in_flags), p.err, p.l2, p.l3, p.l4)} frame {f.hex()}")
                assert p.result_flags == PM.result_word(fl, err), (off, ck, f.hex())
                assert (p.res_len, p.res_l2, p.res_l3, p.res_l4) == (len(sf), l2, l3, l4)
                assert (p.l2_type, p.l3_type, p.l4_type) == PM.types_of(fl), (off, ck, f.hex())


def test_packet_parse_offset_past_the_end(built):
    """odp_packet_parse refuses an offset at or past the packet's end (the
    model does not take one)."""
    from oracle import reflib
    f = pg.udp4_frame()
    for off in (len(f), len(f) + 1, 9000):
        assert reflib.packet_parse(f, off, PM.PROTO_ETH, PM.ALL, 0).ret == -1


# ------------------------------------------- the shim under host sanitizers
def test_shim_sanitised(built, tmp_path):
    """oracle/ref_shim.c's fake packet headers and zero tail are what could be
    read out of bounds: the same sources as a stand-alone executable under
    AddressSanitizer and UBSan (oracle/Makefile ref-shim-main) run clean over
    a fuzz corpus held in exact-size heap blocks, and give the records and
    parse results the library gives."""
    from oracle import reflib
    from odp_amd._build import REF_SHIM_MAIN
    if not os.path.exists(REF_SHIM_MAIN):
        r = subprocess.run(["make", "-s", "-C", reflib.HERE, "ref-shim-main"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0 and "cannot find" in r.stdout:
            pytest.skip("no sanitiser runtime to link against")
    assert os.path.exists(REF_SHIM_MAIN), "oracle/_ref/ref_shim_main is missing: build() makes it"
    opt = RC.OPTS["all_ck_drop"]
    prog = RC.fuzz_case(0)[0]
    frames = RC.fuzz_case(0)[1][:1200] + RC.chksum_corpus()[:400]
    corpus, out = str(tmp_path / "corpus.bin"), str(tmp_path / "out.bin")
    reflib.write_corpus(corpus, prog, frames, opt)
    r = subprocess.run([REF_SHIM_MAIN, corpus, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    with open(out, "rb") as f:
        raw = f.read()
    n = len(frames)
    ref = reflib.Reference(pktin_opt=opt)
    ref.apply(prog)
    assert np.array_equal(np.frombuffer(raw[:16 * n], reflib.RESULT_DTYPE),
                          ref.classify(pg.batch_from_frames(frames)))
    parsed = np.frombuffer(raw[16 * n:], reflib.PARSE_OUT_DTYPE)
    i = 0
    for f in frames:
        for off in (0, 2, 19):
            if off >= len(f):
                continue
            for proto in (PM.PROTO_ETH, PM.PROTO_IPV4, PM.PROTO_IPV6):
                p = reflib.packet_parse(f, off, proto, PM.ALL, 0xF)
                assert parsed[i].tobytes() == bytes(p), (i, off, proto, f.hex())
                i += 1
    assert i == parsed.size
