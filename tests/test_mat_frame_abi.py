"""CPU-only checks of the vector <-> matrix moves (bdsp_hip_mat_from_frames / overlap_add / from_vectors) and of the
batched zero_pad / swap_halves / fft_shift / ifft_shift: the header declares the six new entry points, the built
library exports them, _lib gives them int32 results, DspMat binds the three methods with docstrings that list the
codes, the host functions hold no row loop and no synchronisation, mat_frame.hip builds without a warning, none of its
kernels uses scratch, and the lane loops and index maps of the kernels hold on the host."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
ENTRIES = ("from_frames", "overlap_add", "from_vectors")
KERNELS = ("k_mf_from_frames", "k_mf_overlap_add", "k_mf_from_vectors", "k_mf_zero_pad", "k_mf_rotate")


def expected_names():
    return ["bdsp_hip_mat_%s%s" % (b, s) for b in ENTRIES for s in ("32", "64")]


def _host_function(src, name):
    """the text of the host function template `int name(` of capi.cpp up to the next template or the namespace's end"""
    start = src.index("int %s(" % name)
    ends = [e for e in (src.find("\ntemplate <", start), src.find("} // namespace", start)) if e >= 0]
    return src[start:min(ends)]


def test_header_declares_and_library_exports_the_6_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    names = expected_names()
    assert len(set(names)) == 6
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]
    for n in names:  # the prototypes the Python layer calls through: int32 codes
        assert getattr(L.lib, n).restype is C.c_int32, n
        assert getattr(L.lib, n).argtypes, n
    # the block sits after mat_set_mag_phase, in the 32 and again in the 64 section, under a comment that names the
    # reference
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for s in ("32", "64"):
        at = [hdr.index("bdsp_hip_mat_%s%s(" % (b, s)) for b in ("set_mag_phase",) + ENTRIES]
        assert at == sorted(at), s
    assert hdr.index("bdsp_hip_mat_from_vectors32(") < hdr.index("bdsp_hip_mat_new64")
    for s in ("32", "64"):
        comment = hdr[hdr.index("bdsp_hip_mat_set_mag_phase%s(" % s):hdr.index("bdsp_hip_mat_from_frames%s(" % s)]
        assert "matrix/src/to_from_mat_conversions.rs" in comment, s


def test_python_binds_the_methods():
    import inspect
    from basic_dsp_amd.matrix import DspMat
    assert str(inspect.signature(DspMat.from_frames)) == "(vector, frame_points, hop, pad_tail=False)"
    assert str(inspect.signature(DspMat.overlap_add)) == "(self, hop)"
    assert list(inspect.signature(DspMat.from_vectors).parameters)[0] == "vectors"
    for n in ("from_frames", "from_vectors"):
        assert isinstance(inspect.getattr_static(DspMat, n), classmethod), n
    for n, codes in (("from_frames", ("0", "7", "-1")), ("overlap_add", ("0", "7", "-1")),
                     ("from_vectors", ("0", "7", "2", "-1"))):
        doc = getattr(DspMat, n).__doc__
        assert doc and "Codes" in doc and "Graph" in doc, n
        listed = doc[doc.index("Codes"):]
        assert not [c for c in codes if not re.search(r"(?<![\w.])%s(?![\w.])" % re.escape(c), listed)], n
    # the handle path of the constructor, as DspVec's
    params = inspect.signature(DspMat.__init__).parameters
    assert "_handle" in params and "_sfx" in params


def test_no_row_loop_and_no_synchronise_in_the_host_functions():
    """op_swap (the host function of the shifts, for vectors and matrices), mat_zero_pad, mat_from_frames, mat_overlap_add and mat_from_vectors use neither mat_each_row nor
    mat_resize_rows and no stream or device synchronise.  The one exception: mat_from_vectors uploads its pointer table
    with upload_parts, which waits for that copy (as split_into and merge do) -- that helper holds the call's only
    synchronisation, and the host loop of mat_from_vectors only reads the handles' metadata."""
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        src = f.read()
    banned = ("mat_each_row", "mat_resize_rows", "hipStreamSynchronize", "hipDeviceSynchronize")
    for n in ("op_swap", "mat_zero_pad", "mat_from_frames", "mat_overlap_add", "mat_from_vectors"):
        body = _host_function(src, n)
        assert len(body) > 100, n
        assert not [b for b in banned if b in body], n
        if n != "mat_from_vectors":
            assert not re.search(r"\b(for|while)\s*\(", body), n
    body = _host_function(src, "mat_from_vectors")
    assert body.count("upload_parts<T>(") == 1 and body.count("mf_from_vectors<T>(") == 1
    assert len(re.findall(r"\b(for|while)\s*\(", body)) == 1  # the metadata loop; no copy in it
    loop = body[body.index("for ("):body.index("if (count)")]
    assert "hip" not in loop and "mf_" not in loop and "reserve" not in loop
    assert _host_function(src, "upload_parts").count("hipStreamSynchronize") == 1
    assert "mf_rotate<T>(" in _host_function(src, "op_swap") and "mf_zero_pad<T>(" in _host_function(src, "mat_zero_pad")
    entries = src[src.index("#define BDSP_MAT_FRAME("):src.index("#undef BDSP_MAT_FRAME\n")]
    assert not [b for b in banned if b in entries] and not re.search(r"\b(for|while)\s*\(", entries)
    # the launchers of the unit hold no loop and no synchronisation either; the kernels' loops live in the core header
    with open(os.path.join(CSRC, "mat_frame.hip")) as f:
        unit = f.read()
    host = unit[unit.index("int mf_from_frames("):]
    for n in ("int mf_from_frames(", "int mf_overlap_add(", "int mf_from_vectors(", "int mf_zero_pad(", "int mf_rotate("):
        assert n in host, n
    assert "__global__" not in host
    assert not re.search(r"\b(for|while)\s*\(", host)
    assert "hipStreamSynchronize" not in unit and "hipDeviceSynchronize" not in unit and "atomic" not in unit.split("namespace bdsp")[1]
    assert '#include "mat_frame_core.h"' in unit
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/mat_frame.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "mat_frame_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    rule = re.search(r"#([^\n]*)\n\$\(BUILD\)/mat_frame\.o:[^\n]*\n\t([^\n]*)", mk)
    assert rule and "$(EXACT)" not in rule.group(2) and "$(EXACT)" in rule.group(1)  # the comment says why it is not needed


def test_mat_frame_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/mat_frame.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_matrix_frame_kernels_use_no_scratch(tmp_path):
    """Every k_mf_* kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_mf_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # every kernel is <P, IDX>: 4 packets (real and complex elements of both precisions) x 32- or 64-bit indices = 8
    for k in KERNELS:
        assert len([n for n in found if k in n]) == 8, (k, sorted(found))
    assert len(found) == 8 * len(KERNELS), sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_lane_loops_and_maps_on_the_host(tmp_path):
    """tests/host_sim/sim_mat_frame.cpp runs the lane loops of mat_frame_core.h -- the functions the kernels call -- with
    threads as loops over arrays that count every write and refuse every access out of bounds: the shapes its header
    comment lists, both row counts against a brute-force count, every output written exactly once, every read in bounds
    or replaced by zero, overlap_add's first and last contributing rows exact and its sum bit-equal to the row loop,
    zero_pad and rotate equal to the per-row maps, and, maps only, one extent pair above 2^32."""
    exe = str(tmp_path / "sim_mat_frame")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "sim_mat_frame.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    assert "from_frames: P 0..20 x F 1..6 x H 1..6 x pad_tail 0 1, (1025, 256, 128) (1000, 127, 1) (70002, 3, 1)" in r.stdout
    assert "overlap_add: rows 1..20 x F 1..6 x H 1..6, (257, 100, 25) (2, 4097, 4096) (70000, 3, 1)" in r.stdout
    assert "zero_pad, rotate: row points 1..70 127 128 129 1023 1024 1025 x rows 1 2 3, End Surround Center" in r.stdout
    assert "32- and 64-bit indices" in r.stdout
    assert "70000 x 70002 > 2^32" in r.stdout
