"""CPU-only checks of matmul (the product of two DspMat, a . b and a . b^H): the header declares the two entry points
and names their codes, the built library exports them with the stated prototypes, basic_dsp_amd.matmul is a module-level
function while DspVec and DspMat gained no public name, mat_mul.hip has no atomic operation, builds without a warning and
is in the Makefile with its core header, every k_mm_ kernel of the shipped library is there without scratch, and the
dispatch rule, index maps, LDS maps, lane maps and chunking of mat_mul_core.h hold on the host for every shape of
tests/mat_mul_shapes.txt, which the GPU test reads too (tests/host_sim/sim_mat_mul.cpp)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
NAMES = ("bdsp_hip_mat_matmul32", "bdsp_hip_mat_matmul64")


def test_header_declares_and_library_exports_the_2_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    declared = set(declared_functions())
    assert not [n for n in NAMES if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in NAMES if not hasattr(lib, n)]
    for n in NAMES:  # the prototypes the Python layer calls through
        fn = getattr(L.lib, n)
        assert fn.restype is C.c_int32, n
        assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)], n
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for sfx in ("32", "64"):
        proto = ("int32_t bdsp_hip_mat_matmul%s(const MatBuf%s *a, const MatBuf%s *b, int32_t b_conj_transposed, MatBuf%s **out);"
                 % (sfx, sfx, sfx, sfx))
        assert proto in hdr, proto
    comment = hdr[hdr.index("/* matmul:"):hdr.index("int32_t bdsp_hip_mat_matmul32(")]
    for word in ("-1 for a poisoned", "2 for a real and a complex", "else 7", "*out = NULL", "BDSP_ERR_HIP", "BDSP_ERR_UNSUPPORTED",
                 "K == 0", "M == 0", "N == 0", "conj(b[j][k])", "Deterministic", "CU count", "(2 K + 4) eps", "captured"):
        assert word in comment, word


def test_matmul_is_a_module_level_function_and_the_classes_gained_no_name():
    import inspect
    import numpy as np
    import basic_dsp_amd as b
    from basic_dsp_amd import linalg
    assert b.matmul is linalg.matmul and "matmul" in b.__all__
    assert str(inspect.signature(b.matmul)) == "(a, b, conj_transpose=False)"
    for word in ("a.row_points() == b.rows()", "a.row_points() == b.row_points()", "to_complex()", "Deterministic", "(2 K + 4) eps"):
        assert word in b.matmul.__doc__, word
    for cls in (b.DspVec, b.DspMat):
        assert not [n for n in dir(cls) if "matmul" in n.lower() or "mul_mat" in n.lower() or "gram" in n.lower()], cls
    for bad in ([1.0, 2.0], np.ones((2, 2), dtype=np.float32), None):  # (no device is touched before the type check)
        with pytest.raises(TypeError):
            b.matmul(bad, bad)


def test_the_unit_has_no_atomic_and_is_in_the_makefile():
    with open(os.path.join(CSRC, "mat_mul.hip")) as f:
        unit = f.read()
    with open(os.path.join(CSRC, "mat_mul_core.h")) as f:
        core = f.read()
    assert "atomic" not in unit.lower() and "atomic" not in core.lower()
    kernels = set(re.findall(r"\bvoid (k_\w+)\(", unit))
    assert kernels == {"k_mm_stream", "k_mm_tiled", "k_mm_split_sum"}
    assert '#include "mat_mul_core.h"' in unit and "__builtin_amdgcn_mfma_f32_32x32x2f32" in unit
    assert "getenv" not in unit and "getenv" not in core  # no new environment variable
    # every dispatch threshold is a named constant that cites its line of the profile or says that nobody measured it
    for name in ("MM_STREAM_MAX_M", "MM_STREAM_MAX_K", "MM_SPLIT_MAX_TILES", "MM_SPLIT_MIN_K", "MM_SPLIT_MIN_CHUNK",
                 "MM_SPLIT_TARGET_BLOCKS"):
        assert re.search(r"constexpr size_t %s = \d+;" % name, core), name
    assert core.count("not measured") >= 2 and "profiles/mat_mul.txt" in core
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/mat_mul.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "mat_mul_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    assert os.path.exists(os.path.join(ROOT, "profiles", "mat_mul.txt")) and os.path.exists(os.path.join(ROOT, "tools", "mat_mul_bench.py"))


def test_mat_mul_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_mul.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_mat_mul_kernels_use_no_scratch(tmp_path):
    """Every k_mm_ kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_mm_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # per precision: the streaming kernel for real / complex x 4, 8, 16 accumulator rows, the tiled kernel for real /
    # complex x plain / transposed, the sum of the partials
    per_kernel = {"k_mm_stream": 12, "k_mm_tiled": 8, "k_mm_split_sum": 2}
    for k, want in per_kernel.items():
        assert len([n for n in found if k + "I" in n]) == want, (k, sorted(found))
    assert len(found) == sum(per_kernel.values()), sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_core_templates_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_mul.cpp, built with the host compiler and run as a stand-alone program on
    tests/mat_mul_shapes.txt: the dispatch rule gives the path every line names; each path's maps write every output
    (every partial) exactly once and read nothing out of bounds; the result equals a plain triple loop bit for bit with
    the matrix instruction modelled as a k-ordered fmaf chain; the LDS maps stay inside the planes with 0 bank conflicts;
    the chunks cover K exactly once."""
    exe = str(tmp_path / "sim_mat_mul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "sim_mat_mul.cpp")])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "mat_mul_shapes.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:]
    assert "FAIL" not in r.stdout
    shapes = [l for l in open(os.path.join(ROOT, "tests", "mat_mul_shapes.txt")) if l.strip() and not l.startswith("#")]
    assert "%d shapes (" % len(shapes) in r.stdout and ", 0 failures" in r.stdout
    for path in ("stream", "tiled", "split"):
        assert re.search(r"^%s\s+\d+ shapes, worst error / bound" % path, r.stdout, re.M), path
    assert re.search(r"LDS: \d+ wave accesses counted, 0 bank conflicts at pitch 65 \([1-9]\d* at pitch 64\)", r.stdout)
    assert "512 x 8200 x 512 -> 16 chunks of 544" in r.stdout
