"""CPU-only checks of the matrix's symmetric real-signal transforms (bdsp_hip_mat_plain_sfft / sfft / windowed_sfft /
plain_sifft / sifft / windowed_sifft / mirror / to_complex): the header declares the sixteen entry points, the built
library exports them, DspMat binds the eight methods, the host functions hold no row loop, mat_sym.hip builds without a
warning, none of its kernels uses scratch, and the index maps of the two kernels hold on the host."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
METHODS = ("plain_sfft", "sfft", "windowed_sfft", "plain_sifft", "sifft", "windowed_sifft", "mirror", "to_complex")


def expected_names():
    return ["bdsp_hip_mat_%s%s" % (b, s) for b in METHODS for s in ("32", "64")]


def test_header_declares_and_library_exports_the_16_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    names = expected_names()
    assert len(set(names)) == 16
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]


def test_python_binds_the_methods():
    import inspect
    from basic_dsp_amd.matrix import DspMat
    from basic_dsp_amd.vector import DspVec
    for n in METHODS:
        assert callable(getattr(DspMat, n)), n
        sig = str(inspect.signature(getattr(DspMat, n)))
        if hasattr(DspVec, n):
            # the DspVec method's signature, defaults included
            assert sig == str(inspect.signature(getattr(DspVec, n))), n
        else:
            assert n == "to_complex" and sig == "(self)"
        assert getattr(DspMat, n).__doc__, n


def test_no_row_loop_in_the_new_host_functions():
    """mat_sfft / mat_sifft / mat_mirror use neither mat_each_row nor mat_resize_rows, and no loop at all"""
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        src = f.read()
    start = src.index("int mat_sfft(")
    end = src.index("} // namespace", start)
    body = src[start:end]
    for n in ("mat_sfft", "mat_sifft", "mat_mirror"):
        assert "int %s(" % n in body, n
    assert "mat_each_row" not in body and "mat_resize_rows" not in body
    assert not re.search(r"\b(for|while)\s*\(", body)
    # one stream synchronisation in the whole family: the symmetry flag of the inverse forms
    assert body.count("hipStreamSynchronize") == 1 and "hipDeviceSynchronize" not in body


def test_mat_sym_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_sym.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_matrix_symmetric_kernels_use_no_scratch(tmp_path):
    """Every k_sy_* kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_sy_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # k_sy_crop_rows<C, IDX>: 2 precisions x 32- or 64-bit indices = 4; k_sy_mirror_rows<C, IDX, SCALED>: 2 precisions x
    # 2 index widths x with or without the 1/p scale = 8
    crop = [k for k in found if "k_sy_crop_rows" in k]
    mirror = [k for k in found if "k_sy_mirror_rows" in k]
    assert len(crop) == 4 and len(mirror) == 8 and len(found) == 12, sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_index_maps_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_sym.cpp runs the loops of k_sy_mirror_rows and k_sy_crop_rows over the maps of
    mat_sym_core.h with threads as loops: every p = 1 .. 70 (mirror) and odd N = 1 .. 139 (crop), rows 1, 2, 3, rot 0 and
    p / 2, against a direct restatement of scale -> rotate -> mirror, every output element written exactly once; and the
    first-bin rule against a table of hand cases."""
    exe = str(tmp_path / "sim_mat_sym")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "sim_mat_sym.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    assert "mirror: p 1..70" in r.stdout and "crop: odd N 1..139" in r.stdout
    assert re.search(r"first-bin rule: \d+ hand cases", r.stdout)
