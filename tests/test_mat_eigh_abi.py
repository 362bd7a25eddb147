"""CPU-only checks of eigh (the Hermitian eigendecomposition of a DspMat on the device): the header declares the two entry
points and names their codes, the built library exports them with the stated prototypes, the Python function is
module-level while DspVec and DspMat gained no name, mat_eigh.hip has no atomic operation and no environment variable,
its kernels are exactly the k_je_ set, it builds without a warning and is in the Makefile with its core header, every
k_je_ kernel of the shipped library is there without scratch, and the dispatch rule, pair schedule, launch plan, LDS
maps, per-thread arithmetic and derived bounds of mat_eigh_core.h hold on the host for every shape of
tests/mat_eigh_shapes.txt, which the GPU test reads too (tests/host_sim/sim_mat_eigh.cpp, a stand-alone program built
plainly and with the address and undefined-behaviour sanitizers)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
NAMES = ("bdsp_hip_mat_eigh32", "bdsp_hip_mat_eigh64")
KERNELS = {"k_je_small", "k_je_complete", "k_je_norm", "k_je_pivot", "k_je_rows", "k_je_cols", "k_je_sorted"}


def test_header_declares_and_library_exports_the_2_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    declared = set(declared_functions())
    assert not [n for n in NAMES if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in NAMES if not hasattr(lib, n)]
    for sfx in ("32", "64"):
        fn = getattr(L.lib, "bdsp_hip_mat_eigh" + sfx)
        assert fn.restype is C.c_int32, sfx
        assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)], sfx
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for sfx in ("32", "64"):
        proto = "int32_t bdsp_hip_mat_eigh%s(const MatBuf%s *a, MatBuf%s **w, MatBuf%s **v, int32_t *sweeps);" % (sfx, sfx, sfx, sfx)
        assert proto in hdr, proto
    assert hdr.index("int32_t bdsp_hip_mat_cholesky_solve32(") < hdr.index("/* eigh:")  # after the cholesky block
    comment = hdr[hdr.index("/* eigh:"):hdr.index("int32_t bdsp_hip_mat_eigh32(")]
    comment = re.sub(r"\s*\n \*\s*", " ", comment)  # (one line: a phrase may be wrapped)
    for word in ("-1 for a poisoned", "7 unless", "8 when the Frobenius norm", "not converged after 30 sweeps", "*w = *v = NULL",
                 "BDSP_ERR_HIP", "BDSP_ERR_UNSUPPORTED", "N == 0", "sweeps may be NULL", "lower triangle", "ascending", "Row k",
                 "Deterministic", "CU count", "No atomics", "captured", "one 4-byte read-back", "synchronises once per sweep",
                 "c_res(N, S)", "c_orth(N, S)", "3 launches per block step"):
        assert word in comment, word


def test_the_function_is_module_level_and_the_classes_gained_no_name():
    import inspect
    import numpy as np
    import basic_dsp_amd as b
    from basic_dsp_amd import linalg
    assert b.eigh is linalg.eigh
    assert "eigh" in b.__all__
    assert str(inspect.signature(b.eigh)) == "(a, return_sweeps=False)"
    for word in ("Graph", "Deterministic", "TypeError", "lower triangle", "ascending", "Row k", "c_res(N, sweeps)", "c_orth(N, sweeps)",
                 "30 sweeps"):
        assert word in b.eigh.__doc__, word
    for cls in (b.DspVec, b.DspMat):
        assert not [n for n in dir(cls) if "eig" in n.lower()], cls
    for bad in ([1.0, 2.0], np.ones((2, 2), dtype=np.float32), None):  # (no device is touched before the type check)
        with pytest.raises(TypeError):
            b.eigh(bad)
        with pytest.raises(TypeError):
            b.eigh(bad, return_sweeps=True)


def test_the_unit_has_no_atomic_and_is_in_the_makefile():
    with open(os.path.join(CSRC, "mat_eigh.hip")) as f:
        unit = f.read()
    with open(os.path.join(CSRC, "mat_eigh_core.h")) as f:
        core = f.read()
    assert "atomic" not in unit.lower() and "atomic" not in core.lower()
    assert "getenv" not in unit and "getenv" not in core  # no new environment variable
    assert set(re.findall(r"\bvoid (k_\w+)\(", unit)) == KERNELS
    assert '#include "mat_eigh_core.h"' in unit and '#include "mat_chol_core.h"' in core
    # the attribute for more than 64 KB of dynamic LDS is set before every launch, not once behind a static
    # (through kernel_lds of runtime.cpp, the one place that names the attribute)
    with open(os.path.join(CSRC, "runtime.cpp")) as f:
        runtime = f.read()
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in runtime.split("int kernel_lds(")[1].split("\n}\n")[0]
    assert not re.search(r"\bstatic\s+(bool|int)\b[^;(]*;", unit)
    launches = len(re.findall(r"hipLaunchKernelGGL\((pivot|rows|cols|kern),", unit))
    assert launches == 4 and len(re.findall(r"BDSP_TRY\(kernel_lds\(", unit)) == launches
    for m in re.finditer(r"hipLaunchKernelGGL\((pivot|rows|cols|kern),", unit):  # the line before the launch sets it
        before = unit[:m.start()].rstrip().splitlines()[-1]
        assert "kernel_lds(%s," % m.group(1) in before, before
    # every dispatch constant is named, and its line cites the profile or says that nobody measured it
    for name, typ in (("JE_SMALL_MAX_N", "size_t"), ("JE_BLOCK", "int"), ("JE_INNER_SWEEPS", "int"), ("JE_MAX_SWEEPS", "int")):
        m = re.search(r"^constexpr %s %s = \d+;.*$" % (typ, name), core, re.M)
        assert m and ("not measured" in m.group(0) or "profiles/mat_eigh.txt" in m.group(0)), name
    assert re.search(r"constexpr int JE_MAX_SWEEPS = 30;", core) and re.search(r"constexpr int JE_BLOCK = 32;", core)
    assert re.search(r"constexpr size_t JE_SMALL_MAX_N = 64;", core) and re.search(r"constexpr int JE_INNER_SWEEPS = 2;", core)
    assert "THE LOWER TRIANGLE GOVERNS" in core
    for fn in ("je_dispatch", "je_launches_per_sweep", "je_bound_res", "je_bound_orth", "je_pair"):
        assert re.search(r"\b%s\(" % fn, core), fn
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/mat_eigh.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "mat_eigh_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    rule = mk[:mk.index("$(BUILD)/mat_eigh.o: mat_eigh.hip")].rstrip().splitlines()
    assert "no $(EXACT) is needed" in rule[-1] and rule[-1].startswith("#")
    assert "$(EXACT)" not in mk[mk.index("$(BUILD)/mat_eigh.o: mat_eigh.hip"):].split("\n")[1]
    assert os.path.exists(os.path.join(ROOT, "profiles", "mat_eigh.txt")) and os.path.exists(os.path.join(ROOT, "tools", "mat_eigh_bench.py"))


def test_mat_eigh_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_eigh.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_mat_eigh_kernels_use_no_scratch(tmp_path):
    """Every k_je_ kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_je_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # every kernel for f32 / f64 x real / complex
    for k in KERNELS:
        assert len([n for n in found if k + "I" in n]) == 4, (k, sorted(found))
    assert len(found) == 4 * len(KERNELS), sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_core_templates_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_eigh.cpp, a stand-alone program with its own main, built with the host compiler once plainly
    and once with -fsanitize=address,undefined and run on tests/mat_eigh_shapes.txt: the schedule's steps hold disjoint
    pairs and a sweep every pair once; the dispatch rule gives the path every line names; every element of w and v is
    written exactly once, nothing is read out of bounds, from the upper triangle or from another workgroup of the same
    launch; both paths pass both derived bounds against long double within the sweep cap; diagonal matrices take one
    sweep and give a permutation matrix; the LDS maps stay inside the allocation and the bank-conflict count is printed."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_mat_eigh.cpp")
    with open(src) as f:
        text = f.read()
    assert re.search(r"^int main\(int argc, char\*\* argv\)", text, re.M) and '#include "../../basic_dsp_amd/csrc/mat_eigh_core.h"' in text
    shapes_file = os.path.join(ROOT, "tests", "mat_eigh_shapes.txt")
    shapes = [l.split() for l in open(shapes_file) if l.strip() and not l.startswith("#")]
    assert [int(s[1]) for s in shapes if s[0] == "empty"] == [0]
    assert [int(s[1]) for s in shapes if s[0] == "small"] == [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64]
    assert [int(s[1]) for s in shapes if s[0] == "blocked"] == [65, 95, 96, 97, 127, 128, 129, 130, 200]
    assert len(shapes) == 21
    for flags, name in (([], "sim_mat_eigh"), (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], "sim_mat_eigh_san")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread"] + flags + ["-o", exe, src])
        r = subprocess.run([exe, shapes_file], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        assert "%d shapes (x 4 number kinds), 0 failures" % len(shapes) in r.stdout
        for path in ("small", "blocked"):
            m = re.search(r"^%s\s+worst error / bound: residual (0\.\d+), orthogonality (0\.\d+); most sweeps (\d+) of 30" % path, r.stdout, re.M)
            assert m and float(m.group(1)) <= 1.0 and float(m.group(2)) <= 1.0 and 1 <= int(m.group(3)) <= 30, path
        assert re.search(r"LDS \(row pass, column pass.*\): f32 \d+ accesses, 0 extra bank cycles; f64 \d+ accesses, 0 extra", r.stdout)
