"""odp_packet_parse without a GPU: the CPU model (tests/parse_model.py)
against the reference's own expectations, the new symbols, the error returns
of the device ABI, the no-GPU stance of the ODP calls, and the host-only
odp_packet_parse_result / odp_packet_l2/l3/l4_type.

Reference: test/validation/api/packet/packet.c:3718-4541 (the fixture
tests/golden/parse_frames.json holds its frames and has_*() expectations),
platform/linux-generic/odp_packet.c:2140-2290.
"""
import ctypes as C
import json
import os
import subprocess

import pytest

from tests import parse_model as PM
from tests import rt_helpers as H
from tests.parse_model import FLAG_BITS, result_word, types_of

PARSE_DRIVER = os.path.join(H.ROOT, "tests", "_bin", "parse_driver")


def _golden():
    with open(os.path.join(H.ROOT, "tests", "golden", "parse_frames.json")) as f:
        return json.load(f)["frames"]


@pytest.mark.parametrize("name", sorted(_golden()))
def test_model_reference_cases(built, name):
    """Every golden frame behind the reference's ten L2 offsets, ETH / ALL /
    all checksums: the fixture's flags and return value, l2 at the offset."""
    d = _golden()[name]
    frame = bytes.fromhex(d["frame"])
    for o in PM.REF_OFFSETS:
        ret, fl, err, l2, l3, l4 = PM.parse(PM.shifted(frame, o), o, PM.PROTO_ETH, PM.ALL, 0xF)
        assert ret == d["ret"] and err == 0 and l2 == o and l3 >= o + 14
        for flag, want in d["expect"].items():
            assert (fl >> FLAG_BITS[flag]) & 1 == want, (name, o, flag)


@pytest.mark.parametrize("name,proto,flag,hdr", [("test_packet_ipv4_udp", PM.PROTO_IPV4, "ipv4", 20),
                                                 ("test_packet_ipv6_udp", PM.PROTO_IPV6, "ipv6", 40)])
def test_model_ip_start(built, name, proto, flag, hdr):
    """parse_ipv4_udp (packet.c:3827): the parse starts at the IP header."""
    frame = bytes.fromhex(_golden()[name]["frame"])
    for o in PM.REF_OFFSETS:
        for layer in (PM.L4, PM.ALL):
            ret, fl, err, l2, l3, l4 = PM.parse(PM.shifted(frame, o), o + 14, proto, layer, 0xF)
            assert (ret, err, l2, l3, l4) == (0, 0, PM.INVALID, o + 14, o + 14 + hdr)
            assert fl & (1 << FLAG_BITS[flag]) and fl & (1 << FLAG_BITS["udp"])
            assert not fl & (1 << FLAG_BITS["l2"] | 1 << FLAG_BITS["eth"])
        ret, fl, err, l2, l3, l4 = PM.parse(PM.shifted(frame, o), o + 14, proto, PM.L3, 0xF)
        assert (ret, l3, l4) == (0, o + 14, o + 14 + hdr) and not fl & (1 << FLAG_BITS["udp"] | 1 << 5)
        ret, fl, err, l2, l3, l4 = PM.parse(PM.shifted(frame, o), o + 14, proto, PM.L2, 0xF)
        assert (ret, fl, l3, l4) == (0, 0, o + 14, PM.INVALID)
    # the wrong start protocol: the version check fails at every layer from L3
    other = PM.PROTO_IPV6 if proto == PM.PROTO_IPV4 else PM.PROTO_IPV4
    assert PM.parse(frame, 14, other, PM.ALL, 0)[0] == -1
    assert PM.parse(frame, 14, other, PM.L2, 0)[0] == 0


def test_symbols(built):
    """The new entries exist in the libraries."""
    from odp_amd import cls
    mi = C.CDLL(cls.LIB_MI, mode=C.RTLD_GLOBAL)
    odp = C.CDLL(cls.LIB_ODP)
    for name in ("mi_cls_parse", "mi_cls_parse_host", "mi_cls_parse_host_submit", "mi_cls_parse_host_wait"):
        assert hasattr(mi, name), name
    for name in ("odp_packet_parse", "odp_packet_parse_multi", "odp_packet_parse_result",
                 "odp_packet_parse_result_multi", "odp_packet_l2_type", "odp_packet_l3_type",
                 "odp_packet_l4_type", "odp_amd_cls_parse_host", "odp_amd_cls_parse_term"):
        assert hasattr(odp, name), name


def test_device_abi_errors(built):
    """Bad parameters are -EINVAL with or without a device; without one a
    well-formed call is -ENODEV (no context can exist)."""
    from odp_amd import cls
    L = cls.lib()
    t = C.c_uint64(7)
    for proto, layer in ((0, 4), (4, 4), (1, 0), (1, 5)):
        pp = cls.ParseParam(proto, layer, 0)
        assert L.mi_cls_parse(None, None, None, None, 0, C.byref(pp), None, None) == -22
        assert L.mi_cls_parse_host(None, None, 0, None, None, 0, C.byref(pp), None) == -22
        assert L.mi_cls_parse_host_submit(None, None, 0, None, None, 0, C.byref(pp), None, C.byref(t)) == -22
    pp = cls.ParseParam(cls.PROTO_ETH, cls.LAYER_ALL, 0xF)
    assert L.mi_cls_parse(None, None, None, None, 0, None, None, None) == -22
    assert L.mi_cls_parse_host_submit(None, None, 0, None, None, 0, C.byref(pp), None, None) == -22
    if L.mi_cls_device_count() == 0:
        assert L.mi_cls_parse(None, None, None, None, 1, C.byref(pp), None, None) == -19
        assert L.mi_cls_parse_host(None, None, 0, None, None, 1, C.byref(pp), None) == -19
        assert L.mi_cls_parse_host_submit(None, None, 0, None, None, 1, C.byref(pp), None, C.byref(t)) == -19
        assert t.value == 0
        assert L.mi_cls_parse_host_wait(None, 1) == -19
        assert L.odp_amd_cls_parse_host(None, 0, None, None, 1, 1, 4, 0, None) == -19


@pytest.fixture(scope="module")
def surface(built):
    r = subprocess.run([PARSE_DRIVER, "surface"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()], r.stderr


def test_none_and_offset_return_without_a_call(surface):
    assert ["N", "-1", "-1", "-1", "0", "0", "0"] in surface[0]


def test_no_gpu_no_fallback(surface):
    """Without a GPU odp_packet_parse returns -1 (_multi: 0) and says so
    once; there is no CPU parser behind the call."""
    from odp_amd import cls
    lines, err = surface
    if cls.lib().mi_cls_device_count() == 0:
        assert ["G", "-1", "0"] in lines
        assert err.count("GPU parse unavailable") == 1
    else:
        assert ["G", "0", "2"] in lines


def test_parse_result_and_types(surface):
    """odp_packet_parse_result(_multi) and the type accessors on metadata
    set by hand: one word per input flag, mixed words, with and without an
    error bit."""
    xs = [[int(v, 0) for v in p[1:]] for p in surface[0] if p[0] == "X"]
    assert len(xs) == 2 * 28
    seen = set()
    for flags, err, l2, l3, l4, t2, t3, t4, s3, s4, word, plen in xs:
        assert (l2, l3, l4, plen) == (1, 15, 35, 60)
        assert (t2, t3, t4) == types_of(flags), hex(flags)
        assert word == result_word(flags, err), (hex(flags), err)
        assert s3 == (0 if not flags >> 30 & 1 else 1 if err & 0x04 else 2)
        assert s4 == (0 if not flags >> 31 & 1 else 1 if err & 0x40 else 2)
        seen.add((t2, t3, t4))
    assert {t[2] for t in seen} == {255, 6, 17, 132, 51, 50, 1, 58, 59}
    assert {t[1] for t in seen} == {0xFFFF, 0x0800, 0x86DD, 0x0806}
