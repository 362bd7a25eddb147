"""CPU-only checks of zoom_fft (chirp-z transform of a frequency band): the header declares the six entry points, the
built library exports them, basic_dsp_amd.zoom_fft exists as a module-level function while DspVec and DspMat gained no
public name, zoom_fft.hip builds without a warning, every k_zf_ kernel of the shipped library is there without scratch,
a plain Bluestein plan and a zoom plan cannot be taken for each other, and the templates of zoom_fft_core.h -- phase
reduction, chirp tables, the fused kernel's maps, the general path's maps -- hold on the host against the definition in
long double (tests/host_sim/sim_zoom_fft.cpp)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
ENTRIES = ("bdsp_hip_zoom_fft", "bdsp_hip_mat_zoom_fft", "bdsp_hip_mat_zoom_fft_starts")


def test_header_declares_and_library_exports_the_6_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    names = [b + s for b in ENTRIES for s in ("32", "64")]
    declared = set(declared_functions())
    assert not [n for n in names if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]
    for n in names:  # the prototypes the Python layer calls through: int32 codes, start and step as doubles in both precisions
        fn = getattr(L.lib, n)
        assert fn.restype is C.c_int32, n
        if "starts" in n:
            assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_double, C.c_size_t], n
        else:
            assert fn.argtypes == [C.c_void_p, C.c_double, C.c_double, C.c_size_t], n
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    comment = hdr[hdr.index("/* zoom_fft:"):hdr.index("bdsp_hip_zoom_fft32(")]
    for word in ("Codes: 7", "5 for frequency-domain", "-1 for a poisoned", "BDSP_ERR_UNSUPPORTED", "2^30", "step / delta"):
        assert word in comment, word


def test_zoom_fft_is_a_module_level_function_and_the_classes_gained_no_name():
    import inspect
    import basic_dsp_amd as b
    from basic_dsp_amd import spectral
    assert b.zoom_fft is spectral.zoom_fft and "zoom_fft" in b.__all__
    assert str(inspect.signature(b.zoom_fft)) == "(x, start, step, bins)"
    assert "one value per row" in b.zoom_fft.__doc__ and "step / delta" in b.zoom_fft.__doc__
    for cls in (b.DspVec, b.DspMat):
        assert not [n for n in dir(cls) if "zoom" in n.lower() or "czt" in n.lower() or "chirp" in n.lower()], cls
    with pytest.raises(TypeError):
        b.zoom_fft([1.0, 2.0], 0.0, 0.1, 4)


def test_a_bluestein_lookup_never_matches_a_zoom_plan_and_the_reverse():
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        src = f.read()
    bs = src[src.index("int bs_plan("):src.index("int zf_plan(")]
    zf = src[src.index("int zf_plan("):src.index("int fft_any_len(", src.index("int zf_plan("))]
    assert "if (!p.zoom && p.n == n" in bs
    assert "if (p.zoom && p.n == n && p.bins == bins && p.start == start && p.step == step" in zf
    for body in (bs, zf):  # one byte budget, the same capture rules
        assert body.count("bs_make_room(p.bytes)") == 1
        assert "warm the plan" in body and "++p.pins" in body and "g_capture_plans.push_back(p.chirp)" in body
    # the unit leaves bluestein.hip alone and has kernel names of its own
    with open(os.path.join(CSRC, "zoom_fft.hip")) as f:
        unit = f.read()
    kernels = set(re.findall(r"\bvoid (k_\w+)\(", unit))
    assert kernels == {"k_zf_tables", "k_zf_wg", "k_zf_pre", "k_zf_post"}
    assert "blockIdx.y" not in unit and "atomic" not in unit.split("namespace bdsp")[1]
    assert '#include "zoom_fft_core.h"' in unit
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/zoom_fft.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "zoom_fft_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)


def test_zoom_fft_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/zoom_fft.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_zoom_fft_kernels_use_no_scratch(tmp_path):
    """Every k_zf_ kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_zf_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # per precision: the tables, the fused kernel at 4 lengths x real / complex rows x one start / per-row starts, the pre
    # kernel in the same 4 kinds, the post kernel
    per_kernel = {"k_zf_tables": 2, "k_zf_wg": 32, "k_zf_pre": 8, "k_zf_post": 2}
    for k, want in per_kernel.items():
        assert len([n for n in found if k + "I" in n]) == want, (k, sorted(found))
    assert len(found) == sum(per_kernel.values()), sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_core_templates_against_the_definition_on_the_host(tmp_path):
    """tests/host_sim/sim_zoom_fft.cpp: the fused kernel with threads as loops at all four lengths and the shapes (1, 1),
    (2, 3), (300, 213), (300, 214), (2048, 2049), f32 and f64, real and complex rows, one start and per-row starts,
    against the O(N bins) sum in long double at the project's tolerances; the phase reduction against __int128
    arithmetic at j = 2^30 - 1."""
    exe = str(tmp_path / "sim_zoom_fft")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "sim_zoom_fft.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:]
    assert "FAIL" not in r.stdout
    for prec in ("f32", "f64"):
        for shape in ("L  512     1 ->    1", "L  512     2 ->    3", "L  512   300 ->  213", "L 1024   300 ->  214",
                      "L 2048  1000 ->   64", "L 4096  2048 -> 2049"):
            assert "%s %s" % (prec, shape) in r.stdout, (prec, shape)
    assert "phase_sq   worst" in r.stdout and "phase_lin  worst" in r.stdout
