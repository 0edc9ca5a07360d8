"""The rule-program assembler (odp_amd/csrc/mi_cls_asm.cpp) under
AddressSanitizer and UBSan, on the CPU: tests/rt/asm_check.cpp is compiled
together with it into an ordinary executable and run as a child process
over table blobs of every engine, under every assembler knob, and over
malformed tables."""
import os
import subprocess

import pytest

from odp_amd import cls
from odp_amd import rules as R
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "odp_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "_bin", "asm_check")


def programs():
    """name -> rule program: the smallest sizes that reach each engine."""
    c5 = R.config5(100)[1]
    ncos = sum(1 for op in c5 if op[0] == "cos")
    # config 5 with a fourth level no joint group covers (no tree plan)
    open5 = c5 + [R.cos("deep", queue=900),
                  ("pmr", [R.t_be16(R.PMR_UDP_SPORT, 7)], 17, ncos, 0),
                  ("pmr", [R.t_u8(R.PMR_IPPROTO, 17)], ncos, 161, 0)]
    return {
        "config3": R.config3(100)[1],          # first: the hostile cases corrupt it
        "everything": zoo.prog_everything(),
        "deletes": zoo.prog_deletes(),
        "loop": zoo.prog_loop(),
        "no_default": zoo.prog_no_default(),
        "config2": R.config2(100)[1],
        "config4": R.config4(100)[1],
        "config5": c5,
        "classes": R.config3_classes(100)[1],
        "nested1024": R.config3_nested(100, scale=4)[1],
        "5open": open5,
        "empty": [],
    }


def write_blobs(dirname):
    """Compile every program's table blob into dirname; name -> (path, program_info)."""
    out = {}
    for name, prog in programs().items():
        c = cls.Classifier(gpu=0)
        try:
            c.apply(prog)
            path = os.path.join(str(dirname), name)
            with open(path, "wb") as f:
                f.write(c.compile())
            out[name] = (path, c.program_info())
        finally:
            c.close()
    return out


@pytest.fixture(scope="module")
def asm_check(built):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    # (the sanitiser runtimes are linked into the executable, so it runs the
    # same whatever else the environment loads into a process)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", SRC, "-o", EXE,
                        os.path.join(ROOT, "tests", "rt", "asm_check.cpp"),
                        os.path.join(SRC, "mi_cls_asm.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and ("asan" in r.stdout or "ubsan" in r.stdout) and \
            "cannot find" in r.stdout:
        pytest.skip("no sanitiser runtime to link against")
    assert r.returncode == 0, r.stdout
    return EXE


def test_assembler_sanitised(asm_check, tmp_path):
    """Every program assembles under every knob with no sanitiser report,
    every key of every cuckoo table is found again by the shared hash
    functions, malformed tables are refused, and the default-knob facts are
    those the shipped library reports (mi_cls_program_info)."""
    blobs = write_blobs(tmp_path)
    r = subprocess.run([asm_check, "--hostile"] + [p for p, _ in blobs.values()],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert "hostile ok" in lines
    facts = {}
    for ln in lines:
        f = ln.split()
        if len(f) > 2:
            facts[(f[0], f[1])] = dict(x.split("=", 1) for x in f[2:])
    knobs = {k for _, k in facts}
    assert knobs == {"default", "no_bv", "div0", "div1", "no_wide", "no_cand1", "no_portmerge",
                     "no_flat", "no_joint", "no_plan"}
    assert len(facts) == len(blobs) * len(knobs)
    for name, (_, info) in blobs.items():
        f = facts[(name, "default")]
        got = (int(f["words"]), int(f["hot"]), bool(int(f["tree"])), int(f["flat"]))
        assert got == (info["words"], info["hot_words"], info["tree"], info["flat_engine"]), name
    # the knobs reach the assembler: a few effects that must show
    assert facts[("config3", "no_portmerge")]["fnv"] != facts[("config3", "default")]["fnv"]
    assert facts[("config5", "default")]["plan"] and not facts[("config5", "no_plan")]["plan"]
    assert facts[("5open", "default")]["plan"] == "" and facts[("5open", "default")]["spec"] == "-1"
    assert facts[("config3", "no_flat")]["flat"] == "-1" != facts[("config3", "default")]["flat"]
    assert int(facts[("config3", "default")]["keys"]) > 0
    assert facts[("classes", "default")]["spec"] == "5"    # FM_CHAIN
