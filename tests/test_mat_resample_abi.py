"""CPU-only checks of the matrix resampling family (bdsp_hip_mat_interpolatei / interpolate / interpft / decimatei): the
header declares the eight entry points, the built library exports them, DspMat binds the four methods,
mat_resample.hip builds without a warning, none of its kernels uses scratch, and the index math of the fused kernel
holds on the host."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")


def expected_names():
    bases = ["interpolatei", "interpolate", "interpft", "decimatei"]
    return ["bdsp_hip_mat_%s%s" % (b, s) for b in bases for s in ("32", "64")]


def test_header_declares_and_library_exports_the_8_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    names = expected_names()
    assert len(set(names)) == 8
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]


def test_python_binds_the_methods():
    import inspect
    from basic_dsp_amd.matrix import DspMat
    from basic_dsp_amd.vector import DspVec
    for n in ("interpolatei", "interpolate", "interpft", "decimatei"):
        assert callable(getattr(DspMat, n))
        # the DspVec method's signature, defaults included
        assert str(inspect.signature(getattr(DspMat, n))) == str(inspect.signature(getattr(DspVec, n))), n
        assert getattr(DspMat, n).__doc__


def test_no_row_loop_in_the_new_host_functions():
    """mat_interpolatei / mat_interpolate and their helpers, and op_decimatei (one body for vectors and matrices, rows = 1
    by default; mat_decimatei is gone), use neither mat_each_row nor mat_resize_rows"""
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        src = f.read()
    start = src.index("int mat_resample_general(")
    end = src.index("} // namespace", start)
    body = src[start:end]
    for n in ("mat_resample_fused", "mat_interpolatei", "mat_interpolate"):
        assert "int %s(" % n in body, n
    assert "int mat_decimatei(" not in src
    start = src.index("int op_decimatei(")
    shared = src[start:src.index("\ntemplate <", start)]
    assert "size_t rows = 1)" in shared.split("\n")[0] and "rs_decimate_rows<T>(" in shared
    assert "op_decimatei<T>(&a->v, decimation_factor, delay, a->rows)" in src   # the matrix entry points
    body += shared
    assert "mat_each_row" not in body and "mat_resize_rows" not in body
    assert not re.search(r"\b(for|while)\s*\(", shared)


def test_mat_resample_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_resample.o"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_matrix_resampling_kernels_use_no_scratch(tmp_path):
    """Every k_rs_* kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_rs_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # k_rs_fused<T, N>: 2 precisions x the 9 fused lengths N = 16, 32, ..., 4096 (rs_fused's switch) = 18;
    # k_rs_spectrum_rows<T, MODE>: 2 precisions x 3 modes = 6; k_rs_decimate_rows<P>: real or complex element of 2
    # precisions = 4
    fused = [k for k in found if "k_rs_fused" in k]
    spectrum = [k for k in found if "k_rs_spectrum_rows" in k]
    decimate = [k for k in found if "k_rs_decimate_rows" in k]
    assert len(fused) == 18 and len(spectrum) == 6 and len(decimate) == 4 and len(found) == 28, sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_fused_kernel_index_math_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_resample.cpp runs the kernel's stages (the host + device templates of fft_core.h) with
    threads as loops against a direct O(N^2) evaluation of the chain: every N = 16 ... 4096, every factor with
    p = N / f >= 1, real and complex rows, an arbitrary multiplier table."""
    exe = str(tmp_path / "sim_mat_resample")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "host_sim", "sim_mat_resample.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    # 9 lengths x 2 precisions, none skipped
    assert len(re.findall(r"real and complex rows: ok", r.stdout)) == 18, r.stdout[-3000:]
