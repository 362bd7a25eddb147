"""CPU-only checks of the matrix's time-domain convolution with an impulse-response function and of its real-row
interpolations (bdsp_hip_mat_convolve / convolve_real / convolve_complex / interpolate_lin / interpolate_hermite): the
header declares the ten entry points, the built library exports them, DspMat binds the four methods, the host functions
hold no row loop, mat_interp.hip builds without a warning, none of its kernels uses scratch, and the tiling, staging and
index maps of the kernels hold on the host."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
ENTRIES = ("convolve", "convolve_real", "convolve_complex", "interpolate_lin", "interpolate_hermite")
METHODS = ("convolve", "convolve_complex", "interpolate_lin", "interpolate_hermite")


def expected_names():
    return ["bdsp_hip_mat_%s%s" % (b, s) for b in ENTRIES for s in ("32", "64")]


def test_header_declares_and_library_exports_the_10_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    names = expected_names()
    assert len(set(names)) == 10
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]
    # the prototypes the Python layer calls through: five arguments after the handle at most, int32 codes
    for n in names:
        assert getattr(L.lib, n).restype is C.c_int32, n


def test_python_binds_the_methods():
    import inspect
    from basic_dsp_amd.matrix import DspMat
    from basic_dsp_amd.vector import DspVec
    for n in METHODS:
        assert callable(getattr(DspMat, n)), n
        # the DspVec method's signature, defaults included
        assert str(inspect.signature(getattr(DspMat, n))) == str(inspect.signature(getattr(DspVec, n))), n
        doc = getattr(DspMat, n).__doc__
        assert doc and "Codes" in doc and "-1" in doc, n


def test_no_row_loop_in_the_new_host_functions():
    """mat_convolve_function, its two callback forms and mat_interpolate_real use neither mat_each_row nor
    mat_resize_rows, and no loop at all (the callbacks are sampled by helpers the vector forms share)"""
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        src = f.read()
    start = src.index("int mat_convolve_function(")
    end = src.index("// FFT-domain resampling and decimation of the rows", start)
    body = src[start:end]
    for n in ("mat_convolve_function", "mat_convolve_callback", "mat_convolve_callback_complex", "mat_interpolate_real"):
        assert "int %s(" % n in body, n
    assert "mat_each_row" not in body and "mat_resize_rows" not in body
    assert not re.search(r"\b(for|while)\s*\(", body)
    assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body
    # the launchers of the unit walk no rows on the host either
    with open(os.path.join(CSRC, "mat_interp.hip")) as f:
        unit = f.read()
    host = unit[unit.index("int mt_conv_direct("):]
    assert not re.search(r"\b(for|while)\s*\(", host)


def test_interp_hip_shares_the_arithmetic_with_the_matrix_unit():
    """one definition of the per-output expressions and of the Hermite regions, compiled by both units without FMA
    contraction"""
    with open(os.path.join(CSRC, "interp.hip")) as f:
        vec = f.read()
    with open(os.path.join(CSRC, "mat_interp.hip")) as f:
        mat = f.read()
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    for name in ("interp_lin_value<T>(", "interp_hermite_value<T>(", "interp_hermite_regions<T>("):
        assert name in vec and name in mat, name
    assert '#include "mat_interp_core.h"' in vec and '#include "mat_interp_core.h"' in mat
    for obj in ("interp.o", "mat_interp.o"):
        rule = re.search(r"\$\(BUILD\)/%s:[^\n]*\n\t([^\n]*)" % re.escape(obj), mk)
        assert rule and "$(EXACT)" in rule.group(1), obj
    assert "mat_interp_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)


def test_mat_interp_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_interp.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_matrix_interp_kernels_use_no_scratch(tmp_path):
    """Every k_mt_* kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_mt_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # k_mt_conv_direct<T, CPLX, CW, STAGED, PER>: 2 precisions x (real, complex rows, complex rows and weights) x
    # (staged with four outputs per lane, staged with one, unstaged) = 18; k_mt_interp_lin / _hermite<T, IDX>: 2
    # precisions x 32- or 64-bit indices = 4 each
    conv = [k for k in found if "k_mt_conv_direct" in k]
    lin = [k for k in found if "k_mt_interp_lin" in k]
    her = [k for k in found if "k_mt_interp_hermite" in k]
    assert len(conv) == 18 and len(lin) == 4 and len(her) == 4 and len(found) == 26, sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_maps_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_interp.cpp runs k_mt_conv_direct's loop (virtual blocks, staging into an LDS image,
    accumulation) over the maps of mat_interp_core.h with threads as loops -- points 1 .. 70, 255, 256, 257, 1023, 1024,
    1025, rows 1, 2, 3, L in {0, 1, points / 2, points, 3 * points clipped}: every output written exactly once, every LDS
    read in bounds and staged, results equal to the plain double loop -- and the flat index map of the interpolation
    kernels, including a rows x dest_len pair above 2^32."""
    exe = str(tmp_path / "sim_mat_interp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "sim_mat_interp.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    assert "conv: points 1..70 255 256 257 1023 1024 1025" in r.stdout
    m = re.search(r"\((\d+) four-output, (\d+) one-output, (\d+) unstaged\)", r.stdout)
    assert m and all(int(x) > 0 for x in m.groups()), r.stdout
    assert "70000 x 70001 > 2^32" in r.stdout and "interp values" in r.stdout
