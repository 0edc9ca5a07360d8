"""Native build of the MI355X classification path (in-tree, no JIT cache).

  odp_amd/libmi_cls.so   hipcc --offload-arch=gfx950: HIP kernels + mi_cls.h C ABI
                         (mi_cls.hip, one unit per block shape), linked with
                         two g++ units: the rule-program assembler
                         (mi_cls_asm.cpp, host-only C++17, no HIP) and the
                         specialised kernels' compile manager (mi_cls_spec.cpp,
                         host C++ over the HIP module API)
  odp_amd/mi_cls_jitc    g++ over hipRTC: compiles program-specialised kernels,
                         started by libmi_cls.so as a child process
  odp_amd/libodp_cls.so  gcc: the ODP library of this build -- classification
                         control plane (odp_cls_api.h) + runtime subset and
                         packet I/O (odp_rt.h), linked against libmi_cls.so
  odp_amd/libodph.so     gcc: the ODP helper subset (odp/helper/odph_api.h)
  oracle/_ref/odp_classifier
                         the reference's example/classifier/odp_classifier.c,
                         compiled UNCHANGED against these headers and libraries
                         by oracle/Makefile (only where the reference tree is
                         present; the binary travels, it is never committed)
  oracle/_ref/libodp_ref.so, oracle/_ref/ref_shim_main
                         test infrastructure: the reference's parser, checksum
                         and classifier sources, compiled UNCHANGED, with
                         oracle/ref_shim.c and ref_loop_shim.c (the loop
                         pktio's transmit code), as a library (oracle/reflib.py) and
                         as a sanitised stand-alone program; same rule
"""
from __future__ import annotations

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "odp_amd")
SRC = os.path.join(PKG, "csrc")
INC = os.path.join(ROOT, "include")

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950").split(";")[0] or "gfx950"


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"build failed: {' '.join(cmd)}\n{r.stdout}")
    return r.stdout


def build(force: bool = False, out_dir: str = PKG, defines=(), src_dir: str = SRC) -> list[str]:
    """Build both libraries into out_dir (default: in-tree).  ``defines``
    (e.g. ["WIN=64"]) and ``src_dir`` (a patched copy of odp_amd/csrc,
    tools/variant.py) build a kernel variant for A/B measurement."""
    SRC = src_dir   # noqa: N806 (shadows the module default for this build)
    hdrs = [os.path.join(INC, h) for h in ("mi_cls.h", "odp_cls_api.h")]
    mi_src = os.path.join(SRC, "mi_cls.hip")
    os.makedirs(out_dir, exist_ok=True)
    mi_so = os.path.join(out_dir, "libmi_cls.so")
    odp_srcs = [os.path.join(SRC, f) for f in ("odp_cls.c", "odp_rt.c", "odp_pktio.c", "odp_pktin.c",
                                                "odp_pktout.c", "odp_pcap.c")]
    odp_so = os.path.join(out_dir, "libodp_cls.so")
    odph_src = os.path.join(SRC, "odph.c")
    odph_so = os.path.join(out_dir, "libodph.so")
    rt_hdrs = hdrs + [os.path.join(INC, "odp_rt.h"), os.path.join(INC, "odp_api.h"),
                      os.path.join(INC, "odp", "helper", "odph_api.h"),
                      os.path.join(SRC, "odp_rt_internal.h"), os.path.join(SRC, "odp_txq.h"),
                      os.path.join(SRC, "odp_pktio_internal.h"), os.path.join(SRC, "odp_pcap.h")]
    built = []
    mi_hdr = os.path.join(SRC, "mi_cls_dev.h")
    prog_hdr = os.path.join(SRC, "mi_cls_prog.h")
    # host-only units of libmi_cls.so (g++): the assembler, the compile manager
    asm_src = os.path.join(SRC, "mi_cls_asm.cpp")
    spec_src = os.path.join(SRC, "mi_cls_spec.cpp")
    host_deps = [asm_src, spec_src, prog_hdr, os.path.join(SRC, "mi_cls_asm.h"),
                 os.path.join(SRC, "mi_cls_spec.h")]
    k_srcs = [os.path.join(SRC, f"mi_cls_k{w}.hip") for w in (4, 8, 12, 16, "f", "f12", "f16", "c4",
                                                              "c16", "d", "t", "h", "p", "l", "q", "r", "a", "m", "v")]
    tx_hdr = os.path.join(SRC, "mi_cls_tx_dev.h")
    parse_hdr = os.path.join(SRC, "mi_cls_parse_dev.h")
    lso_hdr = os.path.join(SRC, "mi_cls_lso_dev.h")
    enq_hdrs = [os.path.join(SRC, "mi_cls_enq_dev.h"), os.path.join(SRC, "mi_cls_rank_dev.h"),
                os.path.join(SRC, "mi_cls_run_dev.h"), os.path.join(SRC, "mi_cls_pool_dev.h"),
                os.path.join(SRC, "mi_cls_move_dev.h"), os.path.join(SRC, "mi_cls_vec_dev.h")]
    variant = bool(defines) or src_dir != globals()["SRC"]
    if force or variant or _stale(mi_so, [mi_src, mi_hdr, tx_hdr, parse_hdr, lso_hdr] + enq_hdrs + host_deps + k_srcs + hdrs + [__file__]):
        # one translation unit per block shape + the host code, compiled in
        # parallel (the kernel instantiations dominate the build time)
        import concurrent.futures as cf
        import tempfile
        tmp = tempfile.mkdtemp(prefix="mi_cls_obj_")
        flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-I", INC,
                 "-I", SRC, "-I", tmp] + [f"-D{d}" for d in defines]
        write_src_inc(os.path.join(tmp, "mi_cls_src.inc"), defines, SRC)
        objs = []
        jobs = []
        # MI_CLS_ONLY=kf,k4 (variant builds only): compile just those kernel
        # translation units; the others become -ENOSYS stubs (mi_cls_dev.h)
        only = os.environ.get("MI_CLS_ONLY", "") if variant else ""
        keep = {f"mi_cls_{k}.hip" for k in only.split(",") if k}
        for src in [mi_src] + k_srcs:
            obj = os.path.join(tmp, os.path.basename(src) + ".o")
            objs.append(obj)
            stub = ["-DMI_CLS_STUB"] if keep and src != mi_src and \
                os.path.basename(src) not in keep else []
            jobs.append([HIPCC] + flags + stub + ["-c", "-o", obj, src])
        host = ["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-I", INC, "-I", SRC, "-I", tmp]
        for src, extra in ((asm_src, []), (spec_src, ["-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"])):
            obj = os.path.join(tmp, os.path.basename(src) + ".o")
            objs.append(obj)
            jobs.append(host + extra + ["-c", "-o", obj, src])
        with cf.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
            list(ex.map(_run, jobs))
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", mi_so] + objs)
        shutil.rmtree(tmp, ignore_errors=True)
        built.append(mi_so)
    # the program-specialised kernels' compiler, run as a child process of
    # libmi_cls.so (mi_cls_spec.cpp spec_compile): host code over hipRTC
    jitc_src = os.path.join(SRC, "mi_cls_jitc.cpp")
    jitc = os.path.join(out_dir, "mi_cls_jitc")
    if force or _stale(jitc, [jitc_src]):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
              "-o", jitc, jitc_src, "-L", "/opt/rocm/lib", "-lhiprtc", "-Wl,-rpath,/opt/rocm/lib"])
        built.append(jitc)
    if force or _stale(odp_so, odp_srcs + [mi_so] + rt_hdrs):
        _run(["gcc", "-O2", "-std=gnu11", "-Wall", "-Wextra", "-fPIC", "-ftls-model=initial-exec",
              "-shared", "-I", INC, "-o", odp_so] + odp_srcs + ["-L", out_dir, "-lmi_cls", "-Wl,-rpath,$ORIGIN",
                                          "-lpthread"])
        built.append(odp_so)
    if force or _stale(odph_so, [odph_src, odp_so] + rt_hdrs):
        _run(["gcc", "-O2", "-std=gnu11", "-Wall", "-Wextra", "-fPIC", "-shared", "-I", INC,
              "-o", odph_so, odph_src, "-L", out_dir, "-lodp_cls", "-Wl,-rpath,$ORIGIN",
              "-lpthread"])
        built.append(odph_so)
    if out_dir == PKG:
        for b in (build_example(force), build_reflib(force), build_test_drivers(force)):
            if b:
                built.append(b)
    return built


def write_src_inc(path, defines=(), src_dir=SRC):
    """The kernel sources as C string literals for hipRTC (program-specialised
    kernels, mi_cls_spec.cpp): mi_cls.h, mi_cls_prog.h, mi_cls_dev.h and the build's -D options,
    so a specialised kernel is compiled from exactly the code of this build."""
    def lit(name, text):
        assert ")MICLS\"" not in text
        return f'static const char {name}[] = R"MICLS({text})MICLS";\n'
    with open(os.path.join(INC, "mi_cls.h")) as f:
        h = f.read()
    with open(os.path.join(src_dir, "mi_cls_prog.h")) as f:
        prog = f.read()
    with open(os.path.join(src_dir, "mi_cls_dev.h")) as f:
        dev = f.read()
    defs = ", ".join(f'"-D{d}"' for d in defines)
    with open(path, "w") as f:
        f.write(lit("mi_cls_src_h", h) + lit("mi_cls_src_prog", prog) + lit("mi_cls_src_dev", dev) +
                f"static const char *const mi_cls_src_defs[] = {{ {defs}{', ' if defs else ''}nullptr }};\n"
                f'static const char mi_cls_src_arch[] = "{ARCH}";\n')


TEST_BIN = os.path.join(ROOT, "tests", "_bin")


def build_test_drivers(force: bool = False):
    """Test-only C drivers of the runtime (tests/rt/*.c -> tests/_bin/)."""
    built = None
    deps = [os.path.join(PKG, "libodp_cls.so"), os.path.join(PKG, "libodph.so"),
            os.path.join(INC, "odp_rt.h"), os.path.join(INC, "odp", "helper", "odph_api.h")]
    for name in ("rx_driver", "rt_unit", "tx_driver", "parse_driver", "lso_driver", "mq_driver",
                 "runtab_driver", "pooltab_driver", "vecenq_unit", "vecfill_driver"):
        src = os.path.join(ROOT, "tests", "rt", name + ".c")
        if not os.path.exists(src):
            continue
        os.makedirs(TEST_BIN, exist_ok=True)
        out = os.path.join(TEST_BIN, name)
        # vecfill_driver includes rx_driver.c (its control plane and printing)
        more = [os.path.join(ROOT, "tests", "rt", "rx_driver.c")] if name == "vecfill_driver" else []
        if not force and not _stale(out, [src] + more + deps):
            continue
        # vecenq_unit alone calls the kernel library's own entries (mi_cls_vec_fill)
        mi = ["-lmi_cls"] if name == "vecenq_unit" else []
        _run(["gcc", "-O2", "-std=gnu11", "-Wall", "-I", INC, "-o", out, src, "-L", PKG,
              "-lodph", "-lodp_cls"] + mi + ["-Wl,-rpath,$ORIGIN/" + os.path.relpath(PKG, TEST_BIN),
              "-lpthread"])
        built = out
    return built


def build_vecenq_sanitized(out_dir: str):
    """tests/rt/vecenq_unit.c together with the runtime's C sources under
    -fsanitize=address,undefined, as a stand-alone program in out_dir (never
    in-tree): the memory-safety run of the vector fill's host side.  Needs no
    device.  Run it with ASAN_OPTIONS=detect_leaks=0 (the HIP runtime that
    libmi_cls.so loads keeps allocations of its own); it prints "ok".
      python -c 'from odp_amd import _build as b; print(b.build_vecenq_sanitized("DIR"))'
    """
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "vecenq_unit_san")
    srcs = [os.path.join(SRC, f) for f in ("odp_cls.c", "odp_rt.c", "odp_pktio.c", "odp_pktin.c", "odp_pktout.c",
                                           "odp_pcap.c", "odph.c")]
    _run(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
          "-I", INC, "-I", SRC, "-o", out, os.path.join(ROOT, "tests", "rt", "vecenq_unit.c")] + srcs +
         ["-L", PKG, "-lmi_cls", "-Wl,-rpath," + PKG, "-lpthread"])
    return out


EXAMPLE = os.path.join(ROOT, "oracle", "_ref", "odp_classifier")


def build_example(force: bool = False):
    """Compile the reference's example/classifier source, unchanged, against
    this build's odp_api.h / odph_api.h and link it with libodp_cls.so +
    libodph.so (north-star acceptance: the example links and runs unchanged).
    The recipe is oracle/Makefile's ref-example target, the binary
    oracle/_ref/odp_classifier (never committed).  Nothing is built where the
    reference tree is absent: the binary built where it is present travels."""
    before = os.path.getmtime(EXAMPLE) if os.path.exists(EXAMPLE) else None
    _run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref-example"] +
         (["-B"] if force else []))
    after = os.path.getmtime(EXAMPLE) if os.path.exists(EXAMPLE) else None
    return EXAMPLE if after != before else None


REFLIB = os.path.join(ROOT, "oracle", "_ref", "libodp_ref.so")
REF_SHIM_MAIN = os.path.join(ROOT, "oracle", "_ref", "ref_shim_main")


def build_reflib(force: bool = False):
    """Compile the reference's parser, checksum and classifier sources,
    unchanged, with oracle/ref_shim.c into oracle/_ref/libodp_ref.so (the
    library oracle/reflib.py binds; recipe: oracle/Makefile ref-lib), and the
    same sources as the stand-alone, sanitised oracle/_ref/ref_shim_main
    (ref-shim-main; left out where the compiler has no static sanitiser
    runtimes).  Test infrastructure, never committed; nothing is built where
    the reference tree is absent: what was built where it is present travels.
    The recipe and the shim come with oracle/: an oracle/ directory from
    before them (an older checker beside this build) builds nothing either,
    and oracle/reflib.py, which is then absent too, is what names build()."""
    oracle_dir = os.path.join(ROOT, "oracle")
    with open(os.path.join(oracle_dir, "Makefile")) as f:
        has_recipe = any(ln.startswith("ref-lib") for ln in f)
    if not has_recipe or not os.path.exists(os.path.join(oracle_dir, "ref_shim.c")):
        return None
    before = os.path.getmtime(REFLIB) if os.path.exists(REFLIB) else None
    mk = ["make", "-s", "-C", oracle_dir]
    _run(mk + ["ref-lib"] + (["-B"] if force else []))
    try:
        _run(mk + ["ref-shim-main"])
    except RuntimeError as e:
        if "cannot find" not in str(e):
            raise
    after = os.path.getmtime(REFLIB) if os.path.exists(REFLIB) else None
    return REFLIB if after != before else None


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 2:   # python -m odp_amd._build OUT_DIR DEF=1 ...
        print(build(force=True, out_dir=sys.argv[1], defines=sys.argv[2:]))
    else:
        print(build(force=True))
