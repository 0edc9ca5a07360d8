"""The capture file reader and dump writer (odp_amd/csrc/odp_pcap.c) on their
own: tests/rt/pcap_unit.c, a stand-alone program built with
-fsanitize=address,undefined, parses valid files of every kind, every proper
prefix of a small file of each kind, and hand-made malformed files, each from
a heap block of exactly the input's size -- none of it needs a GPU, and
nothing is loaded into Python."""
import json
import os
import struct
import subprocess

import pytest

from tests import rt_helpers as H
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UDP64 = os.path.join(ROOT, "tests", "golden", "udp64.pcap")
E_FORMAT, E_LINKTYPE = -3, -4   # PCAP_E_FORMAT, PCAP_E_LINKTYPE (odp_pcap.h)
SNAP = 100   # the simple-packet files' interface snap length: shorter than most frames

# the kinds of file: name -> (writer, what a frame becomes)
KINDS = {
    "pcap_le": (lambda p, fr: H.write_pcap(p, fr, "<"), None),
    "pcap_be": (lambda p, fr: H.write_pcap(p, fr, ">"), None),
    "pcap_ns": (lambda p, fr: H.write_pcap(p, fr, "<", nsec=True), None),
    "pcapng_le": (lambda p, fr: H.write_pcapng(p, fr, "<"), None),
    "pcapng_be": (lambda p, fr: H.write_pcapng(p, fr, ">"), None),
    "pcapng_spb": (lambda p, fr: H.write_pcapng(p, fr, "<", kind="spb", snaplen=SNAP), SNAP),
    "pcapng_pb": (lambda p, fr: H.write_pcapng(p, fr, ">", kind="pb"), None),
}


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pcap_unit") / "pcap_unit")
    csrc = os.path.join(ROOT, "odp_amd", "csrc")
    c = subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "rt", "pcap_unit.c"),
                        os.path.join(csrc, "odp_pcap.c")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert c.returncode == 0, c.stdout[-3000:]
    return exe


def _frames_file(path, frames):
    with open(path, "wb") as f:
        f.write(struct.pack("=I", len(frames)))
        for fr in frames:
            f.write(struct.pack("=I", len(fr)) + fr)
    return path


def _run(exe, tmp_path, lines):
    manifest = tmp_path / "manifest"
    manifest.write_text("".join(ln + "\n" for ln in lines))
    r = subprocess.run([exe, str(manifest)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"OK {len(lines)}", \
        (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def _file(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _received(frames, snap=None):
    """What the reader keeps of the written frames: none of length 0 or above
    65535 (judged after the snap length's cut), the others in order."""
    cut = [fr[:snap] if snap else fr for fr in frames]
    return [fr for fr in cut if 0 < len(fr) <= 65535]


def test_valid_files(unit, tmp_path):
    """Every kind of file over the zoo's frames, with an empty and a 70000 B
    frame among them: the frames' bytes and order, the 64 B aligned offsets,
    the zero padding and the 64 owned zero bytes behind the last frame (read
    byte by byte by the program).  The golden capture through the file entry."""
    zf = H.pcap_frames([f for _, f in zoo.all_frames()])
    assert len(zf) > 20 and any(len(f) > SNAP for f in zf) and any(len(f) < SNAP for f in zf)
    frames = zf[:5] + [b""] + zf[5:9] + [bytes(range(256)) * 273 + b"x" * 112] + zf[9:]
    assert len(frames[10]) == 70000
    lines = []
    for kind, (write, snap) in KINDS.items():
        p = str(tmp_path / f"{kind}.cap")
        write(p, frames)
        exp = _received(frames, snap)
        assert len(exp) == len(zf) + (1 if snap else 0) and exp[-1] == (zf[-1][:snap] if snap else zf[-1])
        lines.append(f"check {p} {_frames_file(str(tmp_path / (kind + '.frames')), exp)}")
    with open(os.path.join(ROOT, "tests", "golden", "udp64.json")) as f:
        golden = [bytes.fromhex(h) for h in json.load(f)["frames"]]
    exp = _frames_file(str(tmp_path / "udp64.frames"), golden)
    lines += [f"check {UDP64} {exp}", f"load {UDP64} {exp}"]
    _run(unit, tmp_path, lines)


def test_exact_capacity_and_dump(unit, tmp_path):
    """16384 frames of 64 B pad to exactly the store's first capacity, 1 MiB:
    the store reports 1 MiB + 64 and owns its last byte.  The dump writer's
    file reads back; the MAC filter; a missing file's code."""
    _run(unit, tmp_path, ["exact", f"self {tmp_path}"])


def test_truncations(unit, tmp_path):
    """Every proper prefix of a 3-frame file of each kind, in one process:
    an error code, or a prefix of the whole file's frames."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])[:3]
    lines = []
    for kind, (write, _) in KINDS.items():
        p = str(tmp_path / f"{kind}.cap")
        write(p, frames)
        assert os.path.getsize(p) < 1000
        lines.append(f"trunc {p}")
    _run(unit, tmp_path, lines)


def test_malformed(unit, tmp_path):
    """Hand-made files: each parses without a sanitizer report and gives the
    frames, or the code, stated with it."""
    a, b, c = (bytes([k]) * n for k, n in ((0xa1, 60), (0xb2, 77), (0xc3, 64)))
    ng = H.pcapng_shb() + H.pcapng_idb()
    lines = []

    def keeps(name, data, frames):
        lines.append(f"check {_file(tmp_path, name, data)} {_frames_file(str(tmp_path / (name + '.frames')), frames)}")

    def code(name, data, rc):
        lines.append(f"code {_file(tmp_path, name, data)} {rc}")

    # the file ends in a 12-byte interface block: nothing is read from it
    keeps("idb12", ng + H.pcapng_packet(0, a) + H.pcapng_packet(1, b) + struct.pack("<III", 1, 12, 12), [a, b])
    # an interface block shorter than its fixed fields ends the read
    keeps("idb16", ng + H.pcapng_packet(0, a) + struct.pack("<IIII", 1, 16, 1, 16) + H.pcapng_packet(1, b), [a])
    # a captured length of 0xFFFFFFF0: the frame is skipped, the next ones kept
    for kind in ("epb", "spb", "pb"):
        keeps(f"caplen_{kind}", ng + H.pcapng_packet(0, a, kind=kind) +
              H.pcapng_packet(1, b, kind=kind, caplen=0xFFFFFFF0) + H.pcapng_packet(2, c, kind=kind), [a, c])
    # a block length below 12, and one that is no multiple of 4 (it is taken
    # as it stands: the next block is read where it says)
    keeps("blen8", ng + H.pcapng_packet(0, a) + struct.pack("<III", 6, 8, 8) + H.pcapng_packet(1, b), [a])
    odd = struct.pack("<II", 0x0BAD, 13) + bytes(5)
    keeps("blen13", ng + H.pcapng_packet(0, a) + odd + H.pcapng_packet(1, b), [a, b])
    keeps("blen13_end", ng + H.pcapng_packet(0, a) + odd, [a])
    # a classic record that runs past the file
    hdr = struct.pack("<IHHiIII", 0xa1b2c3d4, 2, 4, 0, 0, 65535, 1)

    def rec(fr, incl=None):
        return struct.pack("<IIII", 0, 0, len(fr) if incl is None else incl, len(fr)) + fr

    keeps("incl_past", hdr + rec(a) + rec(b, incl=len(b) + 1), [a])
    keeps("incl_huge", hdr + rec(a) + rec(b, incl=0xFFFFFFF0) + rec(c), [a])
    # link types other than Ethernet
    code("link_classic", struct.pack("<IHHiIII", 0xa1b2c3d4, 2, 4, 0, 0, 65535, 101) + rec(a), E_LINKTYPE)
    for kind in ("epb", "spb", "pb"):
        code(f"link_{kind}", H.pcapng_shb() + H.pcapng_idb(link=101) + H.pcapng_packet(0, a, kind=kind), E_LINKTYPE)
    # an interface nobody refers to may be anything
    keeps("link_unused", ng + H.pcapng_idb(link=101) + H.pcapng_packet(0, a), [a])
    # 65 interfaces, a packet on the last: the table holds 64, the packet's
    # interface is unknown and its frame is taken
    keeps("if65", H.pcapng_shb() + H.pcapng_idb() * 64 + H.pcapng_idb(link=101) + H.pcapng_packet(0, a, ifc=64) +
          H.pcapng_packet(1, b, kind="pb", ifc=64), [a, b])
    # a second section in the other byte order
    keeps("two_sections", ng + H.pcapng_packet(0, a) + H.pcapng_shb(">") + H.pcapng_idb(">") +
          H.pcapng_packet(1, b, ">") + H.pcapng_packet(2, c, ">", kind="pb"), [a, b, c])
    # the new section forgets the first one's interfaces
    keeps("section_resets", H.pcapng_shb() + H.pcapng_idb(link=101) + H.pcapng_shb(">") + H.pcapng_idb(">") +
          H.pcapng_packet(0, a, ">"), [a])
    # not captures
    code("empty", b"", E_FORMAT)
    code("short23", hdr[:23], E_FORMAT)
    code("text", b"this is not a capture file at all\n", E_FORMAT)
    _run(unit, tmp_path, lines)
