"""CPU-only checks of sosfilt (IIR filtering of a DspVec or of every row of a DspMat on the device): the header declares
the four entry points and names their codes, the built library exports them with the stated prototypes, the Python
function is module-level while DspVec and DspMat gained no name, iir.hip and iir_core.h have no atomic operation, no
environment variable and no function-level static cache, every dispatch constant says whether it was measured, the unit is
in the Makefile and builds without a warning, its kernels use no scratch, the TypeErrors come before any device is
touched, and the plan, the LDS map, the scan tree and the accuracy ratios of iir_core.h hold on the host for every line of
tests/iir_shapes.txt, which the GPU test reads too (tests/host_sim/sim_iir.cpp, a stand-alone program built plainly and
with the address and undefined-behaviour sanitizers)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
NAMES = ("bdsp_hip_sosfilt32", "bdsp_hip_mat_sosfilt32", "bdsp_hip_sosfilt64", "bdsp_hip_mat_sosfilt64")
KERNELS = {"k_iir_tile", "k_iir_carry"}
LENGTHS = [0, 1, 2, 3, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 17]


def test_header_declares_and_library_exports_the_4_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    declared = set(declared_functions())
    assert not [n for n in NAMES if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in NAMES if not hasattr(lib, n)]
    for name in NAMES:
        fn = getattr(L.lib, name)
        assert fn.restype is C.c_int32, name
        assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_void_p], name
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for sfx in ("32", "64"):
        for proto in ("int32_t bdsp_hip_sosfilt%s(VecBuf%s *v, const double *sos, size_t sections, VecBuf%s *state /* may be NULL */);",
                      "int32_t bdsp_hip_mat_sosfilt%s(MatBuf%s *m, const double *sos, size_t sections, MatBuf%s *state /* may be NULL */);"):
            assert proto % (sfx, sfx, sfx) in hdr, proto % (sfx, sfx, sfx)
    assert hdr.index("int32_t bdsp_hip_mat_eigh32(") < hdr.index("/* sosfilt:") < hdr.index("int32_t bdsp_hip_sosfilt32(")  # after the eigh block
    assert hdr.index("int32_t bdsp_hip_mat_eigh64(") < hdr.index("see bdsp_hip_sosfilt32 */") < hdr.index("int32_t bdsp_hip_sosfilt64(")
    comment = hdr[hdr.index("/* sosfilt:"):hdr.index("int32_t bdsp_hip_sosfilt32(")]
    assert comment.count("/*") == 1  # one comment block
    comment = re.sub(r"\s*\n \*\s*", " ", comment)  # (one line: a phrase may be wrapped)
    for word in ("Codes: 0", "7, with the data untouched", "not finite", "a0 == 0", "sections above 16 (IIR_MAX_SECTIONS)", "state of the wrong shape",
                 "-1 for a poisoned", "5 for frequency-domain", "2 for a state of the other number kind", "sections == 0, no rows, or rows of no points",
                 "b0 b1 b2 a0 a1 a2", "direct form II transposed", "may be NULL", "two independent real signals", "BDSP_ERR_HIP",
                 "BDSP_ERR_UNSUPPORTED", "captured", "inf or NaN", "No atomics", "Deterministic", "CU count", "bit-equal", "three launches"):
        assert word in comment, word


def test_the_function_is_module_level_and_the_classes_gained_no_name():
    import inspect
    import numpy as np
    import basic_dsp_amd as b
    from basic_dsp_amd import iir
    assert b.sosfilt is iir.sosfilt
    assert "sosfilt" in b.__all__
    assert str(inspect.signature(b.sosfilt)) == "(x, sos, state=None)"
    for word in ("Graph", "Deterministic", "TypeError", "b0 b1 b2 a0 a1 a2", "bit-equal", "reverse", "two independent real signals",
                 "inf or NaN"):
        assert word in b.sosfilt.__doc__, word
    for cls in (b.DspVec, b.DspMat):
        assert not [n for n in dir(cls) if "sos" in n.lower() or "iir" in n.lower() or "biquad" in n.lower()], cls
    sos = [[1.0, 0.0, 0.0, 1.0, -0.5, 0.0]]
    for bad in ([1.0, 2.0], np.ones((2, 8), dtype=np.float32), None, "x"):  # (no device is touched before the type check)
        with pytest.raises(TypeError):
            b.sosfilt(bad, sos)
        with pytest.raises(TypeError):
            b.sosfilt(bad, sos, state=None)
    # a state of another class or precision: handles that name no device object, so a device call would not survive
    for cls, other in ((b.DspVec, b.DspMat), (b.DspMat, b.DspVec)):
        fakes = [cls(_handle=1, _sfx="32"), other(_handle=1, _sfx="32"), cls(_handle=1, _sfx="64")]
        try:
            for bad_state in fakes[1:] + [np.zeros(2, dtype=np.float32), [0.0, 0.0]]:
                with pytest.raises(TypeError):
                    b.sosfilt(fakes[0], sos, bad_state)
        finally:
            for f in fakes:
                f._h = None  # (nothing to delete)


def test_the_unit_has_no_atomic_and_is_in_the_makefile():
    with open(os.path.join(CSRC, "iir.hip")) as f:
        unit = f.read()
    with open(os.path.join(CSRC, "iir_core.h")) as f:
        core = f.read()
    assert "atomic" not in unit.lower() and "atomic" not in core.lower()
    assert "getenv" not in unit and "getenv" not in core  # no new environment variable
    assert set(re.findall(r"\bvoid (k_\w+)\(", unit)) == KERNELS
    assert '#include "iir_core.h"' in unit
    # no function-level static cache; the attribute for more than 64 KB of dynamic LDS is set before every launch
    for text in (unit, core):
        assert not re.search(r"^\s+static\s+(?!_assert)", text.replace("static_assert", "static__assert"), re.M)
        assert "thread_local" not in text
    # (through kernel_lds of runtime.cpp, the one place that names the attribute)
    with open(os.path.join(CSRC, "runtime.cpp")) as f:
        runtime = f.read()
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in runtime.split("int kernel_lds(")[1].split("\n}\n")[0]
    launches = list(re.finditer(r"hipLaunchKernelGGL\(kern,", unit))
    assert len(launches) == 3 and len(re.findall(r"BDSP_TRY\(kernel_lds\(kern, lds\)\);", unit)) == 3
    for m in launches:  # the line before the launch sets it
        assert "kernel_lds(kern, lds)" in unit[:m.start()].rstrip().splitlines()[-1]
    assert "__shfl_up" in unit and "__syncthreads" in unit  # cross-lane inside a wave, LDS across the waves
    # every dispatch constant is named, and its line cites the profile or says that nobody measured it
    for name in ("IIR_TILE", "IIR_MAX_SECTIONS", "IIR_CARRY_BATCH"):
        m = re.search(r"^constexpr int %s = \d+;.*$" % name, core, re.M)
        assert m and ("not measured" in m.group(0) or "profiles/iir.txt" in m.group(0)), name
    assert re.search(r"constexpr int IIR_TILE = 4096;", core) and re.search(r"constexpr int IIR_MAX_SECTIONS = (16|32);", core)
    assert "RE-RUNS ITS CHUNK" in core and "conflict-free" in core and "ms_lds_stride" in core
    for fn in ("iir_step", "iir_scan_step", "iir_wave_in", "iir_advance", "iir_lane_in", "iir_carry_dot", "iir_lds_slot", "iir_launches",
               "iir_make_tables"):
        assert re.search(r"\b%s\(" % fn, core), fn
    assert "iir_fma" in core and "fmaf(a, b, c)" in core  # explicit fma throughout
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/iir.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "iir_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    rule = mk[:mk.index("$(BUILD)/iir.o: iir.hip")].rstrip().splitlines()
    assert "no $(EXACT) is needed" in rule[-1] and rule[-1].startswith("#")
    assert "$(EXACT)" not in mk[mk.index("$(BUILD)/iir.o: iir.hip"):].split("\n")[1]
    assert os.path.exists(os.path.join(ROOT, "profiles", "iir.txt")) and os.path.exists(os.path.join(ROOT, "tools", "iir_bench.py"))


def test_iir_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/iir.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_iir_kernels_use_no_scratch(tmp_path):
    """Every k_iir_ kernel of the shipped library: present, .private_segment_fixed_size 0."""
    import basic_dsp_amd._lib as L
    llvm = "/opt/rocm/lib/llvm/bin"
    objcopy, readelf = os.path.join(llvm, "llvm-objcopy"), os.path.join(llvm, "llvm-readelf")
    if not (os.path.exists(objcopy) and os.path.exists(readelf)):
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    fat = tmp_path / "fat.bin"
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=%s" % fat, L.LIB_PATH, str(tmp_path / "copy.so")], check=True)
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
                nm = re.search(r"\.name:\s+(_Z\S*k_iir_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # the tile kernel for f32 / f64 x real / complex, the carry kernel for f32 / f64
    assert len([n for n in found if "k_iir_tileI" in n]) == 4 and len([n for n in found if "k_iir_carryI" in n]) == 2, sorted(found)
    assert len(found) == 6, sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_core_functions_on_the_host(tmp_path):
    """tests/host_sim/sim_iir.cpp, a stand-alone program with its own main, built with the host compiler once plainly and
    once with -fsanitize=address,undefined and run on tests/iir_shapes.txt: the one-tile and three-launch plans; every
    output and state scalar written exactly once; the LDS map a bijection inside the allocation with the bank cycles the
    core header claims; the scan tree joins adjacent runs with the table of the right power; the worst accuracy ratios
    are printed and stay within 8, so that R = 16 in tests/test_gpu_iir.py is at least twice what the simulation sees."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_iir.cpp")
    with open(src) as f:
        text = f.read()
    assert re.search(r"^int main\(int argc, char\*\* argv\)", text, re.M) and '#include "../../basic_dsp_amd/csrc/iir_core.h"' in text
    shapes_file = os.path.join(ROOT, "tests", "iir_shapes.txt")
    shapes = [l.split() for l in open(shapes_file) if l.strip() and not l.startswith("#")]
    for kind in ("real", "complex"):
        for prec in ("f32", "f64"):
            mine = [s for s in shapes if s[0] == kind and s[1] == prec]
            assert sorted(set(int(s[3]) for s in mine)) == LENGTHS, (kind, prec)
            assert set(int(s[2]) for s in mine) == {1, 3} and set(int(s[4]) for s in mine) == {1, 2, 8, 16}
            assert set(s[5] for s in mine) == {"lowpass", "resonator", "integrator", "fir"}
            assert [s for s in mine if int(s[3]) == 2 * 4096 + 17 and int(s[2]) == 3]
    assert [s for s in shapes if s[:2] == ["real", "f32"] and int(s[2]) == 3 and int(s[3]) % 4]  # rows off the 16-byte boundary
    for flags, name in (([], "sim_iir"), (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], "sim_iir_san")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, src])
        r = subprocess.run([exe, shapes_file], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        assert "%d shape lines (each with and without an incoming state), 0 failures" % len(shapes) in r.stdout
        m = re.search(r"^worst e_dev / max\(e_ser, eps max\|truth\|\): f32 (\d+\.\d+), f64 (\d+\.\d+)$", r.stdout, re.M)
        s = re.search(r"^worst final-state ratio: f32 (\d+\.\d+), f64 (\d+\.\d+)$", r.stdout, re.M)
        assert m and s and max(float(g) for g in m.groups() + s.groups()) <= 8.0, r.stdout[-600:]
        assert re.search(r"^LDS real: chunk side f32 0, f64 read 0, f64 write 0 extra bank cycles", r.stdout, re.M)
        assert re.search(r"^LDS complex: chunk side f32 0, f64 read 0, f64 write 0 extra bank cycles; row side \(\d+ accesses\) f32 0, f64 read 0, f64 write 0$",
                         r.stdout, re.M)
