"""CPU-only checks of the batched DspMat.interpolatef and its per-row delays (bdsp_hip_mat_interpolatef_delays32 / 64):
the header declares the two entry points and the built library exports them, DspMat.interpolatef keeps DspVec's
signature, the host functions hold no row loop and no synchronisation (mat_resize_rows is gone), interp.hip builds
without a warning, none of its kernels uses scratch, and the block, staging and index maps of the matrix kernels hold
on the host (tests/host_sim/sim_mat_interpf.cpp, also under the address and undefined-behaviour sanitizers)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
NAMES = ["bdsp_hip_mat_interpolatef_delays32", "bdsp_hip_mat_interpolatef_delays64"]
SIM = os.path.join(ROOT, "tests", "host_sim", "sim_mat_interpf.cpp")


def _capi():
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        return f.read()


def _function(src, head):
    """the text of the function that starts with `head`, up to its closing brace in column 0"""
    start = src.index(head)
    return src[start:src.index("\n}\n", start) + 3]


def test_header_declares_and_library_exports_the_two_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    declared = set(declared_functions())
    assert not [n for n in NAMES if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in NAMES if not hasattr(lib, n)]
    for n in NAMES:
        assert getattr(L.lib, n).restype is C.c_int32, n
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    comment = hdr[hdr.index("interpolatef with one delay per row"):hdr.index("int32_t bdsp_hip_mat_interpolatef_delays32")]
    assert "7" in comment and "-1" in comment and "captured" in comment


def test_python_keeps_the_vector_signature_and_documents_the_codes():
    import inspect
    from basic_dsp_amd.matrix import DspMat
    from basic_dsp_amd.vector import DspVec
    assert str(inspect.signature(DspMat.interpolatef)) == str(inspect.signature(DspVec.interpolatef))
    doc = DspMat.interpolatef.__doc__
    assert doc and "Codes" in doc and "7" in doc and "-1" in doc and "delay[r]" in doc


def test_no_row_loop_and_no_synchronisation_in_the_host_functions():
    src = _capi()
    assert "mat_resize_rows" not in src and "mat_each_row" not in src
    for head in ("int mat_interpolatef(", "int mat_interpolatef_delays("):
        body = _function(src, head)
        assert not re.search(r"\b(for|while)\s*\(", body), head
        assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body, head
        assert body.count("reserve(") == 1 and body.count("mat_interpolatef_dev<T>(") == 1 and "trade()" in body, head
    assert _function(src, "int mat_interpolatef_delays(").count("hipMemcpyAsync(") == 1
    fill = _function(src, "void mat_interpf_fill_rows(")
    assert re.search(r"\bfor\s*\(", fill) and "hip" not in fill.lower()
    # the launcher of the unit walks no rows on the host either
    with open(os.path.join(CSRC, "interp.hip")) as f:
        unit = f.read()
    launcher = _function(unit, "int mat_interpolatef_dev(")
    assert not re.search(r"\bfor\s*\(|\bwhile\s*\((?!0\))", launcher)  # (its macros end in `while (0)`)
    assert "hipStreamSynchronize" not in launcher and "hipDeviceSynchronize" not in launcher


def test_one_body_per_kernel_and_one_plan():
    """the vector kernels and the matrix kernels instantiate the same bodies, and both launchers take the path from
    interp_plan; the unit is built without FMA contraction and dev_fma is where it was"""
    with open(os.path.join(CSRC, "interp.hip")) as f:
        unit = f.read()
    for body in ("interp_table_walk<T, CPLX>(", "interp_inner_tile<T, CPLX, FACTOR, QB, ", "interp_scalar_body<T, CPLX, ",
                 "interp_scalar_v2_body<T, CPLX, ", "interp_frac_pk_body<T, CPLX, "):
        assert unit.count(body) >= 2, body
    assert unit.count("interp_plan<T>(") == 2
    assert "T dev_fma(T a, T b, T c);" in unit and '#include "interp_core.h"' in unit
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    rule = re.search(r"\$\(BUILD\)/interp\.o:[^\n]*\n\t([^\n]*)", mk)
    assert rule and "$(EXACT)" in rule.group(1)
    assert "interp_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)


def test_interp_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/interp.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_interp_kernels_use_no_scratch(tmp_path):
    """Every kernel of interp.hip in the shipped library -- the vector kernels k_interp_* and the matrix kernels
    k_mat_interpf_* -- has .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*(?:k_mat_interpf_|k_interp_)\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    count = lambda name: len([k for k in found if name in k])
    # k_mat_interpf_inner<T, CPLX, FACTOR, QB>: 2 precisions x real / complex x factors 2, 3, 4, 8 = 16, as k_interp_inner;
    # _table<T, CPLX>: 4; the three scalar kernels <T, CPLX, IDX>: 2 x 2 x 32- / 64-bit walks = 8 each;
    # k_interp_taps<T, ROWS>: 2 x 2
    assert count("k_mat_interpf_inner") == 16 and count("k_interp_inner") == 16, sorted(found)
    assert count("k_mat_interpf_table") == 4 and count("k_interp_table") == 4, sorted(found)
    for name in ("k_mat_interpf_scalarI", "k_mat_interpf_scalar_v2", "k_mat_interpf_frac_pk"):
        assert count(name) == 8, (name, sorted(found))
    assert count("k_interp_taps") == 4, sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def _run_sim(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "integer: points 1..70 255 256 257 1023 1024 1025, rows 1..3 and 70000, factors 2 3 4 5 8" in r.stdout
    m = re.search(r"\((\d+) blocked, (\d+) table; (\d+) tiles on unaligned rows, (\d+) row crossings\)", r.stdout)
    assert m and all(int(x) > 0 for x in m.groups()), r.stdout
    assert "70000 x 70002 > 2^32" in r.stdout


def test_maps_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_interpf.cpp runs the loops of the matrix kernels over the maps of interp_core.h with
    threads as loops: every output of every row written exactly once, every global read of row r inside row r, every LDS
    slot that is read staged for the current row, the values of the integer path equal to the reference's formulas."""
    exe = str(tmp_path / "sim_mat_interpf")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, SIM])
    _run_sim(exe)


def test_maps_on_the_host_under_the_sanitizers(tmp_path):
    """the same program, stand-alone, under -fsanitize=address,undefined (host code only)"""
    exe = str(tmp_path / "sim_mat_interpf_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, SIM], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    _run_sim(exe)
