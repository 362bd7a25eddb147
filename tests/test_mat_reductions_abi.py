"""CPU-only checks of the per-row matrix reductions (bdsp_hip_mat_*statistics* / *sum* / *dot_product*): the header
declares the 48 entry points, the built library exports them, mat_reduce.hip builds without a warning and none of its
kernels uses scratch."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")


def expected_names():
    bases = ["real_statistics", "complex_statistics", "real_statistics_split", "complex_statistics_split",
             "real_sum", "real_sum_sq", "complex_sum", "complex_sum_sq",
             "real_dot_product", "complex_dot_product", "real_dot_product_vector", "complex_dot_product_vector"]
    return ["bdsp_hip_mat_%s%s%s" % (b, p, s) for b in bases for p in ("", "_prec") for s in ("32", "64")]


def test_header_declares_and_library_exports_the_48_matrix_reductions():
    import ctypes as C
    import basic_dsp_amd._lib as L
    names = expected_names()
    assert len(set(names)) == 48
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]


def test_mat_reduce_and_reduce_build_without_warnings(tmp_path):
    """The new unit and the vector unit that now shares reduce_common.h, compiled with the Makefile's flags."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_reduce.o", build + "/reduce.o"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_matrix_reduction_kernels_use_no_scratch(tmp_path):
    """Every k_mr_* kernel of the shipped library: present, .private_segment_fixed_size 0 (StatPartial is 104 bytes
    and the lane-group folds shuffle it field by field)."""
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
            # each kernel's metadata block: .name then, later, .private_segment_fixed_size
            for blk in re.split(r"\n\s*- \.", notes):
                nm = re.search(r"\.name:\s+(_Z\S*k_mr_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    assert len(found) >= 76, len(found)  # stats 2 x 2 x 2 x 6, dot 2 x 2 x 6, fold 2 x 2
    assert not {k: v for k, v in found.items() if v}, found
