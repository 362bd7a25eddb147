"""CPU-only checks of the per-row diff / cum_sum / wrap / unwrap of the matrix API (bdsp_hip_mat_diff* / _cum_sum* /
_wrap* / _unwrap*): the header declares the ten entry points, the built library exports them, DspMat binds the five
methods, mat_scan.hip and vecmath.hip build without a warning, none of the k_ms_* kernels uses scratch, and the tile
index math of the unwrap kernel holds on the host."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")


def expected_names():
    bases = ["diff", "diff_with_start", "cum_sum", "wrap", "unwrap"]
    return ["bdsp_hip_mat_%s%s" % (b, s) for b in bases for s in ("32", "64")]


def test_header_declares_and_library_exports_the_10_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    names = expected_names()
    assert len(set(names)) == 10
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]


def test_python_binds_the_methods():
    from basic_dsp_amd.matrix import DspMat
    for n in ("diff", "diff_with_start", "cum_sum", "wrap", "unwrap"):
        assert callable(getattr(DspMat, n))


def test_mat_scan_and_vecmath_build_without_warnings(tmp_path):
    """The scan unit (vectors and matrices) and the vector unit of the math family, compiled with the Makefile's flags."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_scan.o", build + "/vecmath.o"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_matrix_scan_kernels_use_no_scratch(tmp_path):
    """Every k_ms_* kernel of the shipped library: present, .private_segment_fixed_size 0 (the unwrap kernel keeps a
    whole prefetched tile, 64 registers per lane, in fully unrolled loops)."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_ms_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))

    def count(part):
        return len([k for k in found if part in k])
    # two precisions each: k_ms_diff 1; k_ms_scan_short real / complex x lane groups 4, 16, 64; k_ms_scan_row,
    # k_ms_scan_sums, k_ms_scan_apply real / complex; k_ms_unwrap 4 tile shapes; k_ms_scan_offsets<E>: 2 in all
    assert count("k_ms_diff") == 2 and count("k_ms_scan_short") == 12 and count("k_ms_scan_row") == 4, sorted(found)
    assert count("k_ms_scan_sums") == 4 and count("k_ms_scan_apply") == 4 and count("k_ms_scan_offsets") == 2, sorted(found)
    assert count("k_ms_unwrap") == 8 and len(found) == 36, sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_unwrap_tile_index_math_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_scan.cpp drives mat_scan_core.h with threads as loops: every element to exactly one LDS
    slot and back to its own address, no bank conflict among the lanes of a group in the walk and in the fill / drain
    passes, the walk bit-identical to the plain recurrence; f32 and f64, all four tile shapes, rows in {1, 63, 64, 65,
    257} x row lengths in {0, 1, W-1, W, W+1, 3W+5}."""
    exe = str(tmp_path / "sim_mat_scan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "host_sim", "sim_mat_scan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
