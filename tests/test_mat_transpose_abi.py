"""CPU-only checks of the moves across the rows of a matrix (bdsp_hip_mat_transpose / from_interleaved / to_interleaved /
zero_interleave): the header declares the eight new entry points, the built library exports them, _lib gives them int32
results, DspMat binds the four methods with docstrings that list the codes, the host functions hold no row loop, no
pointer table and no synchronisation, mat_transpose.hip builds without a warning, none of its kernels uses scratch,
and the tile geometry, the lane loops and the LDS bank arithmetic of the kernels hold on the host."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
ENTRIES = ("transpose", "from_interleaved", "to_interleaved", "zero_interleave")
KERNELS = ("k_tp_tiled", "k_tp_flat")


def expected_names():
    return ["bdsp_hip_mat_%s%s" % (b, s) for b in ENTRIES for s in ("32", "64")]


def _host_function(src, name):
    """the text of the host function template `int name(` of capi.cpp up to the next template or the namespace's end"""
    start = src.index("int %s(" % name)
    ends = [e for e in (src.find("\ntemplate <", start), src.find("} // namespace", start)) if e >= 0]
    return src[start:min(ends)]


def test_header_declares_and_library_exports_the_8_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    names = expected_names()
    assert len(set(names)) == 8
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]
    for n in names:  # the prototypes the Python layer calls through: int32 codes
        assert getattr(L.lib, n).restype is C.c_int32, n
        assert getattr(L.lib, n).argtypes, n
    # the block sits after mat_from_vectors, in the 32 and again in the 64 section, under a comment that names the
    # reference and states the codes
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for s in ("32", "64"):
        at = [hdr.index("bdsp_hip_mat_%s%s(" % (b, s)) for b in ("from_vectors",) + ENTRIES]
        assert at == sorted(at), s
    assert hdr.index("bdsp_hip_mat_zero_interleave32(") < hdr.index("bdsp_hip_mat_new64")
    assert hdr.index("bdsp_hip_mat_zero_interleave64(") < hdr.index("bdsp_hip_dev_fft(")
    for s in ("32", "64"):
        comment = hdr[hdr.index("bdsp_hip_mat_from_vectors%s(" % s):hdr.index("bdsp_hip_mat_transpose%s(" % s)]
        assert "data_reorganization.rs" in comment, s
    comment = hdr[hdr.index("bdsp_hip_mat_from_vectors32("):hdr.index("bdsp_hip_mat_transpose32(")]
    for word in (": 7,", "-1", "P % channels != 0", "WITHOUT ROWS", "delta"):
        assert word in comment, word


def test_python_binds_the_methods():
    import inspect
    from basic_dsp_amd.matrix import DspMat
    assert str(inspect.signature(DspMat.transpose)) == "(self)"
    assert str(inspect.signature(DspMat.from_interleaved)) == "(vector, channels)"
    assert str(inspect.signature(DspMat.to_interleaved)) == "(self)"
    assert str(inspect.signature(DspMat.zero_interleave)) == "(self, factor)"
    assert isinstance(inspect.getattr_static(DspMat, "from_interleaved"), classmethod)
    for n, codes in (("transpose", ("0", "-1")), ("from_interleaved", ("0", "7", "-1")), ("to_interleaved", ("0", "-1")),
                     ("zero_interleave", ("0", "-1"))):
        doc = getattr(DspMat, n).__doc__
        assert doc and "Codes" in doc and "Graph" in doc, n
        listed = doc[doc.index("Codes"):]
        assert not [c for c in codes if not re.search(r"(?<![\w.])%s(?![\w.])" % re.escape(c), listed)], n
    assert "cannot be captured" in DspMat.from_interleaved.__doc__ and "cannot be captured" in DspMat.to_interleaved.__doc__
    assert "can be captured" in DspMat.transpose.__doc__


def test_no_row_loop_no_pointer_table_and_no_synchronise_in_the_host_functions():
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        src = f.read()
    banned = ("mat_each_row", "mat_resize_rows", "hipStreamSynchronize", "hipDeviceSynchronize", "upload_parts")
    for n in ("mat_transpose", "mat_from_interleaved", "mat_to_interleaved", "mat_zero_interleave"):
        body = _host_function(src, n)
        assert len(body) > 100, n
        assert not [b for b in banned if b in body], n
        assert not re.search(r"\b(for|while)\s*\(", body), n
    for n in ("mat_transpose", "mat_from_interleaved", "mat_to_interleaved"):
        assert _host_function(src, n).count("tp_transpose<T>(") == 1, n   # one launch
    assert _host_function(src, "mat_zero_interleave").count("rg_zero_interleave<T>(") == 1
    assert "mat_extent(" in _host_function(src, "mat_from_interleaved") and "mat_extent(" in _host_function(src, "mat_zero_interleave")
    assert ".trade()" in _host_function(src, "mat_transpose")
    entries = src[src.index("#define BDSP_MAT_TRANSPOSE("):src.index("#undef BDSP_MAT_TRANSPOSE\n")]
    assert not [b for b in banned if b in entries] and not re.search(r"\b(for|while)\s*\(", entries)
    assert entries.count("mat_code<T>(") == 2  # the two in-place calls, transpose and zero_interleave
    # the launchers of the unit hold no loop and no synchronisation; the kernels' loops live in the core header
    with open(os.path.join(CSRC, "mat_transpose.hip")) as f:
        unit = f.read()
    host = unit[unit.index("static int tp_launch("):]
    for n in ("static int tp_launch(", "static int tp_launch_bytes(", "int tp_transpose("):
        assert n in host, n
    assert "__global__" not in host
    assert not re.search(r"\b(for|while)\s*\(", host)
    code = unit.split("namespace bdsp")[1]
    assert "hipStreamSynchronize" not in unit and "hipDeviceSynchronize" not in unit and "atomic" not in code
    assert '#include "mat_transpose_core.h"' in unit
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/mat_transpose.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "mat_transpose_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    rule = re.search(r"#([^\n]*)\n\$\(BUILD\)/mat_transpose\.o:[^\n]*\n\t([^\n]*)", mk)
    assert rule and "$(EXACT)" not in rule.group(2) and "$(EXACT)" in rule.group(1)  # the comment says why it is not needed


def test_mat_transpose_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_transpose.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_matrix_transpose_kernels_use_no_scratch(tmp_path):
    """Every k_tp_* kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_tp_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # every kernel is <P, IDX>: 3 packets (elements of 4, 8 and 16 bytes; f64 and c32 share the 8-byte one) x 32- or
    # 64-bit indices = 6
    for k in KERNELS:
        assert len([n for n in found if k in n]) == 6, (k, sorted(found))
    assert len(found) == 12, sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_tiles_lane_loops_and_lds_banks_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_transpose.cpp runs the load and store loops and the flat map of mat_transpose_core.h -- the
    functions the kernels call -- with threads as loops over arrays that count every write and refuse every access out
    of bounds, in global memory and in LDS: the shapes its header comment lists, the tiled and the thin path on every
    one of them, both index widths, one extent above 2^32 (maps only), and the bank conflicts of both sides of the LDS
    tile from the banking rule -- 0 for every element size, as the unit's header comment claims."""
    exe = str(tmp_path / "sim_mat_transpose")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "sim_mat_transpose.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    assert "tiled (64, 32) and flat: R x C 1..70 x 1..70, 127 128 129 1023 1024 1025 x 1 2 3 both ways round" in r.stdout
    assert "32- and 64-bit indices" in r.stdout
    assert "70000 x 70002 > 2^32" in r.stdout
    assert "LDS bank conflicts at pitch S + 1: 4 B write 0 read 0, 8 B write 0 read 0, 16 B write 0 read 0" in r.stdout
    with open(os.path.join(CSRC, "mat_transpose.hip")) as f:
        head = f.read().split("#include")[0]
    assert "S + 1 elements" in head and "every element size: 0" in head and "TP_THIN = 16" in head
