"""CPU-only checks of the matrix's math family, reverse, mixer, wrap-around binary operations and part getters /
setters (bdsp_hip_mat_sqrt .. bdsp_hip_mat_set_mag_phase): the header declares the 94 entry points, the built library
exports them, DspMat binds every method with the DspVec method's signature, the host functions hold no row loop and no
synchronisation, elementwise.hip and mat_ew.hip compile one definition of the arithmetic without FMA contraction,
mat_ew.hip builds without a warning, none of its kernels uses scratch, and the index maps of the kernels hold on the
host."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
MATH0 = ("sqrt", "square", "ln", "exp", "sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh", "asinh",
         "acosh", "atanh", "abs", "ln_approx", "exp_approx", "sin_approx", "cos_approx")
MATH1 = ("root", "powf", "log", "expf", "log_approx", "expf_approx", "powf_approx")
SMALLER = ("add_smaller", "sub_smaller", "mul_smaller", "div_smaller")
ROW_AWARE = ("reverse", "multiply_complex_exponential") + SMALLER + tuple(n + "_vector" for n in SMALLER)
PARTS = ("get_real", "get_imag", "get_magnitude", "get_magnitude_squared", "get_phase", "get_real_imag", "get_mag_phase",
         "set_real_imag", "set_mag_phase")
ENTRIES = MATH0 + MATH1 + ROW_AWARE + PARTS
METHODS = MATH0 + MATH1 + ("reverse", "multiply_complex_exponential") + SMALLER + PARTS
ROW_HOST_FUNCTIONS = ("op_reverse",)  # one body for vectors and matrices (rows = 1 by default)
HOST_FUNCTIONS = ("mat_mul_cexp", "mat_smaller", "mat_get_part", "mat_get_pair", "mat_set_pair")


def expected_names():
    return ["bdsp_hip_mat_%s%s" % (b, s) for b in ENTRIES for s in ("32", "64")]


def test_header_declares_and_library_exports_the_94_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    assert (len(MATH0) + len(MATH1), len(ROW_AWARE), len(PARTS)) == (28, 10, 9)
    names = expected_names()
    assert len(set(names)) == 94
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]
    for n in names:  # the prototypes the Python layer calls through: int32 codes
        assert getattr(L.lib, n).restype is C.c_int32, n
        assert getattr(L.lib, n).argtypes, n
    # the block sits after mat_interpolate_hermite, in the 32 and again in the 64 section, under a comment that names
    # the reference
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for s in ("32", "64"):
        assert hdr.index("bdsp_hip_mat_interpolate_hermite" + s) < hdr.index("bdsp_hip_mat_sqrt" + s) < \
            hdr.index("bdsp_hip_mat_set_mag_phase" + s)
    assert hdr.index("bdsp_hip_mat_set_mag_phase32") < hdr.index("bdsp_hip_mat_new64")
    comment = hdr[hdr.index("bdsp_hip_mat_interpolate_hermite32"):hdr.index("bdsp_hip_mat_sqrt32")]
    for ref in ("general/elementary.rs:226-350", "real.rs:58-130", "elementary.rs:190-198", "complex.rs:203-211",
                "elementary.rs:117-188", "complex.rs:119-201", "complex.rs:135-151"):
        assert ref in comment, ref


def test_python_binds_the_methods():
    import inspect
    from basic_dsp_amd.matrix import DspMat
    from basic_dsp_amd.vector import DspVec
    assert len(METHODS) == 28 + 2 + 4 + 9
    for n in METHODS:
        assert callable(getattr(DspMat, n)), n
        # the DspVec method's signature
        assert str(inspect.signature(getattr(DspMat, n))) == str(inspect.signature(getattr(DspVec, n))), n
        doc = getattr(DspMat, n).__doc__
        assert doc and "Codes" in doc and "-1" in doc, n


def test_no_row_loop_and_no_synchronise_in_the_new_host_functions():
    """op_reverse and mat_mul_cexp .. mat_set_pair use neither mat_each_row nor mat_resize_rows, no loop at
    all and no stream or device synchronise; the math family is op_math on the flat vector; the launchers of mat_ew.hip
    hold no loop either"""
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        src = f.read()
    start = src.index("int mat_mul_cexp(")
    end = src.index("} // namespace", start)
    body = src[start:end]
    for n in HOST_FUNCTIONS:
        assert "int %s(" % n in body, n
    banned = ("mat_each_row", "mat_resize_rows", "hipStreamSynchronize", "hipDeviceSynchronize")
    assert not [b for b in banned if b in body]
    assert not re.search(r"\b(for|while)\s*\(", body)
    # reverse: the vector's host function, which takes the matrix's rows
    start = src.index("int op_reverse(")
    shared = src[start:src.index("\ntemplate <", start)]
    for n in ROW_HOST_FUNCTIONS:
        assert "int %s(" % n in shared and "size_t rows = 1)" in shared[shared.index("int %s(" % n):].split("\n")[0], n
    assert "mw_reverse<T>(" in shared
    assert not [b for b in banned if b in shared]
    assert not re.search(r"\b(for|while)\s*\(", shared)
    # *_smaller_vector: op_binary_smaller, the vector's host function, with the matrix's rows (mat_smaller_vector is gone)
    assert "int mat_smaller_vector(" not in src
    start = src.index("int op_binary_smaller(")
    smaller = src[start:src.index("\ntemplate <", start)]
    assert "size_t rows = 1)" in smaller.split("\n")[0] and "mw_smaller<T>(" in smaller
    assert not [b for b in banned if b in smaller]
    assert not re.search(r"\b(for|while)\s*\(", smaller)
    entries = src[src.index("#define BDSP_MAT_EW_M0("):src.index("#undef BDSP_MAT_EW\n")]
    assert "op_reverse<T>(&a->v, a->rows)" in entries
    for op in range(4):
        assert "op_binary_smaller<T>(&a->v, H<T>(o), %d, a->rows)" % op in entries
    assert entries.count("op_math<T>(&a->v") == 3  # the two macros of the family and root
    assert not [b for b in banned if b in entries] and not re.search(r"\b(for|while)\s*\(", entries)
    with open(os.path.join(CSRC, "mat_ew.hip")) as f:
        unit = f.read()
    host = unit[unit.index("int mw_cexp("):]
    for n in ("int mw_cexp(", "int mw_reverse(", "int mw_smaller("):
        assert n in host, n
    assert "__global__" not in host
    assert not re.search(r"\b(for|while)\s*\(", host)
    assert "hipStreamSynchronize" not in unit and "hipDeviceSynchronize" not in unit


def test_elementwise_hip_shares_the_arithmetic_with_the_matrix_unit():
    """one definition of OpMulCexp's per-element expressions, compiled by both units without FMA contraction; the
    *_smaller expressions have one user, mat_ew.hip (vectors run its kernel with one row), and elementwise.hip keeps no
    copy and no kernel of them"""
    with open(os.path.join(CSRC, "elementwise.hip")) as f:
        vec = f.read()
    with open(os.path.join(CSRC, "mat_ew.hip")) as f:
        mat = f.read()
    with open(os.path.join(CSRC, "mat_ew_core.h")) as f:
        core = f.read()
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    for name in ("cexp_phasor<T>(", "cexp_mul<T>(", "smaller_real<T>(", "smaller_complex<T>("):
        if name.startswith("cexp"):
            assert name in vec and name in mat, name
        else:   # one copy left: nothing to keep equal
            assert name in mat and name not in vec, name
        assert re.search(r"BDSP_MW_HD \w+ %s\(" % name[:-4], core), name
    assert '#include "mat_ew_core.h"' in vec and '#include "mat_ew_core.h"' in mat
    # the vector unit keeps no second copy of the expressions
    assert "sincos(p.a" not in vec and "k_binary_smaller" not in vec
    for obj in ("elementwise.o", "mat_ew.o"):
        rule = re.search(r"\$\(BUILD\)/%s:[^\n]*\n\t([^\n]*)" % re.escape(obj), mk)
        assert rule and "$(EXACT)" in rule.group(1), obj
    assert "$(BUILD)/mat_ew.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "mat_ew_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    # the reason for $(EXACT) is stated above the rule
    assert re.search(r"#[^\n]*no FMA contraction\n\$\(BUILD\)/mat_ew\.o:", mk)


def test_mat_ew_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_ew.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_matrix_ew_kernels_use_no_scratch(tmp_path):
    """Every k_mw_* kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_mw_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # k_mw_cexp<T>: 2 precisions; k_mw_reverse<P, IDX>: 4 packets (real and complex elements of both precisions) x 32-
    # or 64-bit indices = 8; k_mw_smaller<T, CPLX, IDX>: 2 precisions x real or complex x 32- or 64-bit indices = 8
    cexp = [k for k in found if "k_mw_cexp" in k]
    rev = [k for k in found if "k_mw_reverse" in k]
    sml = [k for k in found if "k_mw_smaller" in k]
    assert len(cexp) == 2 and len(rev) == 8 and len(sml) == 8 and len(found) == 18, sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_maps_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_ew.cpp runs the loops of k_mw_cexp, k_mw_reverse and k_mw_smaller over the maps of
    mat_ew_core.h with threads as loops -- points 1 .. 70, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, rows 1, 2, 3,
    257, plus 70000 x 3 and, maps only, a rows x points pair above 2^32: every element written exactly once, every
    read in bounds, the phasor index is the position in the row, the reverse source and the operand index are right."""
    exe = str(tmp_path / "sim_mat_ew")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "sim_mat_ew.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    assert "shapes: points 1..70 127 128 129 255 256 257 1023 1024 1025 x rows 1 2 3 257" in r.stdout
    assert "shape: 70000 x 3" in r.stdout
    assert "70000 x 70002 > 2^32" in r.stdout
