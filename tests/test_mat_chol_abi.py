"""CPU-only checks of cholesky / cholesky_solve (Hermitian positive-definite systems on the device): the header declares
the four entry points and names their codes, the built library exports them with the stated prototypes, the two Python
functions are module-level while DspVec and DspMat gained no name, mat_chol.hip has no atomic operation and no environment
variable, its kernels are exactly the k_la_ set, it builds without a warning and is in the Makefile with its core header,
every k_la_ kernel of the shipped library is there without scratch, and the dispatch rule, launch plan, LDS maps and
per-thread arithmetic of mat_chol_core.h hold on the host for every shape of tests/mat_chol_shapes.txt, which the GPU
test reads too (tests/host_sim/sim_mat_chol.cpp, built plainly and with the address and undefined-behaviour sanitizers)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
NAMES = ("bdsp_hip_mat_cholesky32", "bdsp_hip_mat_cholesky64", "bdsp_hip_mat_cholesky_solve32", "bdsp_hip_mat_cholesky_solve64")


def test_header_declares_and_library_exports_the_4_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    declared = set(declared_functions())
    assert not [n for n in NAMES if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in NAMES if not hasattr(lib, n)]
    for sfx in ("32", "64"):
        fn = getattr(L.lib, "bdsp_hip_mat_cholesky" + sfx)
        assert fn.restype is C.c_int32 and fn.argtypes == [C.c_void_p, C.c_double, C.POINTER(C.c_void_p)], sfx
        fn = getattr(L.lib, "bdsp_hip_mat_cholesky_solve" + sfx)
        assert fn.restype is C.c_int32 and fn.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)], sfx
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for sfx in ("32", "64"):
        for proto in ("int32_t bdsp_hip_mat_cholesky%s(const MatBuf%s *a, double loading, MatBuf%s **out);" % (sfx, sfx, sfx),
                      "int32_t bdsp_hip_mat_cholesky_solve%s(const MatBuf%s *l, const MatBuf%s *b, int32_t part, MatBuf%s **out);"
                      % (sfx, sfx, sfx, sfx)):
            assert proto in hdr, proto
    assert hdr.index("int32_t bdsp_hip_mat_matmul32(") < hdr.index("/* cholesky / cholesky_solve:")  # after the matmul block
    comment = hdr[hdr.index("/* cholesky / cholesky_solve:"):hdr.index("int32_t bdsp_hip_mat_cholesky32(")]
    comment = re.sub(r"\s*\n \*\s*", " ", comment)  # (one line: a phrase may be wrapped)
    for word in ("-1 for a poisoned", "2 for a real and a complex", "7 unless", "8 when a pivot", "*out = NULL", "BDSP_ERR_HIP",
                 "BDSP_ERR_UNSUPPORTED", "N == 0", "P == 0", "lower triangle", "loading", "0 both", "1 forward", "2 backward",
                 "Deterministic", "CU count", "c(N) = 2 N + 4", "3 c(N)", "captured", "does not synchronise", "No atomics"):
        assert word in comment, word


def test_the_functions_are_module_level_and_the_classes_gained_no_name():
    import inspect
    import numpy as np
    import basic_dsp_amd as b
    from basic_dsp_amd import linalg
    assert b.cholesky is linalg.cholesky and b.cholesky_solve is linalg.cholesky_solve
    assert "cholesky" in b.__all__ and "cholesky_solve" in b.__all__
    assert str(inspect.signature(b.cholesky)) == "(a, loading=0.0)"
    assert str(inspect.signature(b.cholesky_solve)) == "(l, b, part='both')"
    for fn in (b.cholesky, b.cholesky_solve):
        for word in ("Graph", "Deterministic", "(2 N + 4) eps", "TypeError"):
            assert word in fn.__doc__, (fn.__name__, word)
    for cls in (b.DspVec, b.DspMat):
        assert not [n for n in dir(cls) if "chol" in n.lower() or "solve" in n.lower()], cls
    for bad in ([1.0, 2.0], np.ones((2, 2), dtype=np.float32), None):  # (no device is touched before the type check)
        with pytest.raises(TypeError):
            b.cholesky(bad)
        with pytest.raises(TypeError):
            b.cholesky_solve(bad, bad)


def test_the_unit_has_no_atomic_and_is_in_the_makefile():
    with open(os.path.join(CSRC, "mat_chol.hip")) as f:
        unit = f.read()
    with open(os.path.join(CSRC, "mat_chol_core.h")) as f:
        core = f.read()
    assert "atomic" not in unit.lower() and "atomic" not in core.lower()
    assert "getenv" not in unit and "getenv" not in core  # no new environment variable
    kernels = set(re.findall(r"\bvoid (k_\w+)\(", unit))
    assert kernels == {"k_la_panel", "k_la_update", "k_la_trsolve"}
    assert '#include "mat_chol_core.h"' in unit and "__builtin_amdgcn_mfma_f32_32x32x2f32" in unit
    assert '#include "mat_mul_core.h"' in core
    # the attribute for more than 64 KB of dynamic LDS is set before every launch, not once behind a static
    # (through kernel_lds of runtime.cpp, the one place that names the attribute)
    with open(os.path.join(CSRC, "runtime.cpp")) as f:
        runtime = f.read()
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in runtime.split("int kernel_lds(")[1].split("\n}\n")[0]
    assert "BDSP_TRY(kernel_lds(kern, lds));\n    hipLaunchKernelGGL(kern," in unit and not re.search(r"\bstatic\s+(bool|int)\b[^;(]*;", unit)
    # every dispatch threshold is a named constant that cites its line of the profile or says that nobody measured it
    for name in ("LA_SMALL_MAX_N", "LA_SOLVE_MAX_BLOCKS"):
        m = re.search(r"^(.*\n)?.*constexpr size_t %s = \d+;.*$" % name, core, re.M)
        assert m and ("not measured" in m.group(0) or "profiles/mat_chol.txt" in m.group(0)), name
    assert re.search(r"constexpr int LA_BLOCK = 64;", core)
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/mat_chol.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "mat_chol_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    assert os.path.exists(os.path.join(ROOT, "profiles", "mat_chol.txt")) and os.path.exists(os.path.join(ROOT, "tools", "mat_chol_bench.py"))


def test_mat_chol_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_chol.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_mat_chol_kernels_use_no_scratch(tmp_path):
    """Every k_la_ kernel of the shipped library: present, .private_segment_fixed_size 0."""
    import basic_dsp_amd._lib as L
    llvm = "/opt/rocm/lib/llvm/bin"
    objcopy, readelf = os.path.join(llvm, "llvm-objcopy"), os.path.join(llvm, "llvm-readelf")
    if not (os.path.exists(objcopy) and os.path.exists(readelf)):
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    fat = tmp_path / "fat.bin"
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=%s" % fat, L.LIB_PATH, str(tmp_path / "copy.so")],
                   check=True)
    blob = fat.read_bytes()
    found = {}
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob):
        p = m.start()
        count = struct.unpack_from("<Q", blob, p + 24)[0]
        off = p + 32
        for _ in range(count):
            o, size, tl = struct.unpack_from("<QQQ", blob, off)
            off += 24
            triple = blob[off:off + tl].decode()
            off += tl
            if "gfx950" not in triple or size == 0:
                continue
            co = tmp_path / "co.elf"
            co.write_bytes(blob[p + o:p + o + size])
            notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"\n\s*- \.", notes):
                nm = re.search(r"\.name:\s+(_Z\S*k_la_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # per precision: the panel kernel for real / complex; the update kernel for real / complex x three forms; the
    # diagonal solve for real / complex x 8, 16, 32, 64 unknowns x forward / backward
    per_kernel = {"k_la_panel": 4, "k_la_update": 12, "k_la_trsolve": 32}
    for k, want in per_kernel.items():
        assert len([n for n in found if k + "I" in n]) == want, (k, sorted(found))
    assert len(found) == sum(per_kernel.values()), sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_core_templates_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_chol.cpp, a stand-alone program, built with the host compiler once plainly and once with
    -fsanitize=address,undefined and run on tests/mat_chol_shapes.txt: the dispatch rule gives the path every line names;
    every element of L and X is written exactly once, nothing is read out of bounds, from the upper triangle or in the
    launch that wrote it; the launch counts obey the caps; both paths pass the derived bounds against long double; the
    LDS maps stay inside the allocation and the bank-conflict count is printed."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_mat_chol.cpp")
    shapes_file = os.path.join(ROOT, "tests", "mat_chol_shapes.txt")
    shapes = [l for l in open(shapes_file) if l.strip() and not l.startswith("#")]
    want_n = {0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 191, 200}
    want_p = {0, 1, 63, 64, 65, 255, 256, 257, 1000}
    assert {int(l.split()[1]) for l in shapes} == want_n
    for n in (17, 64, 65, 130):
        assert {int(l.split()[2]) for l in shapes if int(l.split()[1]) == n} == want_p, n
    for n in want_n:
        assert len([l for l in shapes if int(l.split()[1]) == n]) >= 2, n
    for flags, name in (([], "sim_mat_chol"), (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], "sim_mat_chol_san")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + flags + ["-o", exe, src])
        r = subprocess.run([exe, shapes_file], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        assert "%d shapes (x 4 number kinds), 0 failures" % len(shapes) in r.stdout
        for path in ("small", "blocked"):
            assert re.search(r"^%s\s+worst residual / bound: cholesky 0\.\d+, forward 0\.\d+, backward 0\.\d+, both 0\.\d+" % path,
                             r.stdout, re.M), path
        assert re.search(r"LDS \(panel update.*\): real f32 \d+ accesses, \d+ extra bank cycles; complex f64 \d+ accesses, \d+ extra", r.stdout)
