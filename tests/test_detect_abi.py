"""CPU-only checks of detect and argrelmax (the detections of a DspVec or of every row of a DspMat as a compact list): the
header declares the four entry points and names their codes and rules, the built library exports them with the stated
prototypes, the Python functions are module-level while DspVec and DspMat gained no name, the TypeErrors and the
Python-side 7s come before any device is touched, detect.hip and detect_core.h have no atomic operation, no environment
variable, no function-level static and no experiment switch, kernel_lds comes before every launch with dynamic LDS, each
dispatch constant says whether it was measured, the unit is in the Makefile and builds without a warning, its kernels use
no scratch, tests/detect_shapes.txt covers what it must, and the index maps, the predicate, the boundary index, the LDS
map and the prefix arithmetic hold on the host for every line of it (tests/host_sim/sim_detect.cpp, a stand-alone program
built plainly and with the address and undefined-behaviour sanitizers)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
NAMES = ("bdsp_hip_detect32", "bdsp_hip_mat_detect32", "bdsp_hip_detect64", "bdsp_hip_mat_detect64")
SHAPES_FILE = os.path.join(ROOT, "tests", "detect_shapes.txt")
KINDS = ("none", "scalar", "scalar-inf", "row", "profile", "cell")


def core_constants():
    with open(os.path.join(CSRC, "detect_core.h")) as f:
        core = f.read()
    return {k: int(v) for k, v in re.findall(r"^constexpr int (DETECT_\w+) = (\d+);", core, re.M)}


def shapes():
    """[(rows, n, order, boundary, kind)] of tests/detect_shapes.txt"""
    out = []
    for line in open(SHAPES_FILE):
        if line.strip() and not line.startswith("#"):
            rows, n, order, boundary, kind = line.split()
            out.append((int(rows), int(n), int(order), boundary, kind))
    return out


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
        assert fn.argtypes == [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p], name
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    flat = re.sub(r"\s+", " ", hdr)
    for sfx, real in (("32", "float"), ("64", "double")):
        for proto in ("int32_t bdsp_hip_detect%s(const VecBuf%s *v, int32_t kind, const void *threshold, size_t order, int32_t boundary, "
                      "size_t capacity, int64_t *counts /* 1 */, int64_t *index /* capacity */, %s *value /* capacity */);",
                      "int32_t bdsp_hip_mat_detect%s(const MatBuf%s *m, int32_t kind, const void *threshold, size_t order, int32_t boundary, "
                      "size_t capacity, int64_t *counts /* rows */, int64_t *index, %s *value);"):
            assert proto % (sfx, sfx, real) in flat, proto % (sfx, sfx, real)
    assert hdr.index("int32_t bdsp_hip_mat_rank_filter32(") < hdr.index("/* detect:") < hdr.index("int32_t bdsp_hip_detect32(")  # after the rank_filter block
    assert hdr.index("int32_t bdsp_hip_mat_rank_filter64(") < hdr.index("see bdsp_hip_detect32 */") < hdr.index("int32_t bdsp_hip_detect64(")
    comment = hdr[hdr.index("/* detect:"):hdr.index("int32_t bdsp_hip_detect32(")]
    assert comment.count("/*") == 1  # one comment block
    comment = re.sub(r"\s*\n \*\s*", " ", comment)  # (one line: a phrase may be wrapped)
    for word in ("Codes: 0", "7, with nothing written", "unknown kind or boundary", "a NULL counts", "NULL lists with capacity > 0", "kind 4 on a vector",
                 "-1 for a poisoned x or operand", "4 (BDSP_ERR_MUST_BE_REAL) for a complex x or operand", "size and meta-data checks of add",
                 "BDSP_ERR_UNSUPPORTED for order above 1024 (DETECT_MAX_ORDER)", "rows x tiles above 2^31", "No rows, or rows of no points",
                 "counts zeroed", "0 none", "1 one value", "2 one value per row", "on a vector it means one value", "3 one profile for all rows",
                 "4 one value per cell", "double(x[j]) > t", "x[r][j] > t[r][j]", "IEEE >", "a NaN on either side is never a detection",
                 "-0 is not above +0", "denormals compare by value", "+inf > t", "0 < |d| <= order", "x[j] > x[j + d]", "0 (open)", "1 (wrap)",
                 "2 (nearest)", "with n = 1 every cell passes", "any number of turns", "order >= n", "scipy.signal.argrelmax", "never a peak",
                 "Plateaus yield no peak", "a NaN neighbour blocks a peak", "always the true number", "first min(total, capacity)", "row-major order",
                 "exactly the bits of the detected input", "follows from counts", "the write launch is skipped", "four launches", "64-bit ballot",
                 "No atomics", "Deterministic", "CU count", "equals the vector call", "x is read twice", "are not modified"):
        assert word in comment, word
    k = core_constants()
    assert k["DETECT_MAX_ORDER"] == 1024 and k["DETECT_TILE"] == 1024  # (the figures the comment prints)


def test_the_functions_are_module_level_and_the_classes_gained_no_name():
    import importlib
    import inspect
    import numpy as np
    import basic_dsp_amd as b
    module = importlib.import_module("basic_dsp_amd.detect")  # (the package attribute of that name is the function)
    assert b.detect is module.detect and b.argrelmax is module.argrelmax
    assert "detect" in b.__all__ and "argrelmax" in b.__all__
    assert str(inspect.signature(b.detect)) == "(x, threshold=None, order=0, boundary='open', capacity=None)"
    assert str(inspect.signature(b.argrelmax)) == "(x, order=1, mode='clip')"
    assert module.FIRST_CAPACITY == 65536
    for word in ("IEEE >", "a NaN on either side is never a detection", "-0 is not above +0", "denormals compare by value", "row-major order",
                 "exactly the bits of x[row, index]", "FIRST_CAPACITY", "count stays true", "TypeError", "Deterministic", "Plateaus yield no peak",
                 "a NaN neighbour blocks a peak", "x is not modified", "equals the vector call", '"open"', '"wrap"', '"nearest"', "BackendError"):
        assert word in " ".join(b.detect.__doc__.split()), word  # (a phrase may be wrapped)
    for word in ("scipy.signal.argrelmax", "same C entry", "order below 1", "unknown mode", "TypeError", "(row, index)", "(index,)"):
        assert word in " ".join(b.argrelmax.__doc__.split()), word
    for cls in (b.DspVec, b.DspMat):
        assert not [n for n in dir(cls) if "detect" in n.lower() or "argrel" in n.lower() or "peak" in n.lower()], cls
    for bad in ([1.0, 2.0], np.ones((2, 8), dtype=np.float32), None, "x", 1.0):  # (no device is touched before the type check)
        with pytest.raises(TypeError):
            b.detect(bad)
        with pytest.raises(TypeError):
            b.detect(bad, 0.0, -1, "no such rule", -1)  # (the type comes before the arguments)
        with pytest.raises(TypeError):
            b.argrelmax(bad)
        with pytest.raises(TypeError):
            b.argrelmax(bad, 0, "no such mode")
    # Python-side argument errors answer 7 without a device call: a handle that names no device object would not survive one
    for cls in (b.DspVec, b.DspMat):
        fake = cls(_handle=1, _sfx="32")
        try:
            for bad in ("0.0", b"0", {"t": 0.0}, 1j, ["a"], True, object(), np.array(1j)):  # a threshold of no known kind
                with pytest.raises(TypeError):
                    b.detect(fake, bad)
                with pytest.raises(TypeError):
                    b.detect(fake, bad, order=-1)
            for kwargs in ({"order": -1}, {"order": 1.0}, {"order": "1"}, {"order": None}, {"order": 1 << 64}, {"capacity": -1}, {"capacity": 2.0},
                           {"boundary": "zero"}, {"boundary": "clip"}, {"boundary": 0}, {"boundary": None}):
                assert b.detect(fake, **kwargs) == (7, None), kwargs
                assert b.detect(fake, 0.5, **kwargs) == (7, None) and b.detect(fake, [0.5], **kwargs) == (7, None), kwargs
            for args in ((0,), (-1,), (1.0,), ("1",), (1, "nearest"), (1, "open"), (1, None), (1, 0)):
                assert b.argrelmax(fake, *args) == (7, None), args
        finally:
            fake._h = None  # (nothing to delete)
    fake_v, fake_m = b.DspVec(_handle=1, _sfx="32"), b.DspMat(_handle=1, _sfx="32")
    try:
        assert b.detect(fake_v, fake_m) == (7, None)  # one value per cell on a vector
    finally:
        fake_v._h = fake_m._h = None


def test_the_unit_has_no_atomic_and_is_in_the_makefile():
    with open(os.path.join(CSRC, "detect.hip")) as f:
        unit = f.read()
    with open(os.path.join(CSRC, "detect_core.h")) as f:
        core = f.read()
    assert "atomic" not in unit.lower() and "atomic" not in core.lower()
    assert "getenv" not in unit and "getenv" not in core  # no environment variable
    assert set(re.findall(r"\bvoid (k_\w+)\(", unit)) == {"k_detect_count", "k_detect_scan_tiles", "k_detect_scan_rows", "k_detect_write"}
    assert '#include "detect_core.h"' in unit
    # the core is plain C++: no HIP include, the markers only under __HIPCC__; the boundary index is rank_filter's
    assert "hip/" not in core and "bdsp_internal.h" not in core
    assert re.search(r"#if defined\(__HIPCC__\)\n#define BDSP_DETECT_HD __host__ __device__ __forceinline__\n#else\n#define BDSP_DETECT_HD inline\n#endif", core)
    assert '#include "rank_filter_core.h"' in core and "rank_src_index(" in unit
    # no function-level static, no experiment switch
    for text in (unit, core):
        assert not re.search(r"^\s+static\s+(?!_assert)", text.replace("static_assert", "static__assert"), re.M)
        assert "thread_local" not in text and "#ifdef" not in text and "#ifndef" not in text
    # four launches; dynamic LDS goes through kernel_lds, on the line before each launch that has any
    launches = list(re.finditer(r"hipLaunchKernelGGL\((\w+), [^;]*;", unit))
    assert [m.group(1) for m in launches] == ["count", "k_detect_scan_tiles", "k_detect_scan_rows", "write"]
    for m in launches:
        lds_arg = m.group(0).split(",")[3].strip()
        before = unit[:m.start()].rstrip().splitlines()[-1]
        if m.group(1) in ("count", "write"):
            assert lds_arg == "lds" and "BDSP_TRY(kernel_lds(%s, lds));" % m.group(1) in before, m.group(0)
        else:
            assert lds_arg == "0", m.group(0)  # static LDS only
        assert "BDSP_LAUNCH_CHECK();" in unit[m.end():].lstrip().splitlines()[0]
    assert "hipFuncSetAttribute" not in unit and unit.count("extern __shared__") == 1
    # the launch with capacity 0 is skipped, before the write kernel's attributes are touched
    assert unit.index("if (capacity == 0) return BDSP_OK;") < unit.index("auto write = k_detect_write<T>;")
    # places come from the 64-bit ballot, the mbcnt pair and the population count
    for word in ("__ballot(", "__builtin_amdgcn_mbcnt_lo(", "__builtin_amdgcn_mbcnt_hi(", "__popcll("):
        assert word in unit, word
    # rows need not be aligned: one value per lane and step, no vector type
    assert not re.search(r"\b(float[24]|double2|uint4|int4|uint2)\b", unit)
    # every dispatch constant is named, and its line cites the profile or says that nobody measured it
    for name in ("DETECT_TILE", "DETECT_MAX_ORDER", "DETECT_SCAN_ITEMS", "DETECT_SCAN_CHUNK"):
        m = re.search(r"^constexpr int %s = \d+;.*$" % name, core, re.M)
        assert m, name
        assert "not measured" in m.group(0) or ("measured" in m.group(0) and "profiles/detect.txt" in m.group(0)), name
    k = core_constants()
    assert k["DETECT_TILE"] == k["DETECT_THREADS"] * k["DETECT_PER_LANE"] == 1024 and k["DETECT_MAX_ORDER"] == 1024 and k["DETECT_THREADS"] == 256
    assert k["DETECT_SEGMENTS"] * k["DETECT_WAVE"] == k["DETECT_TILE"] and k["DETECT_WAVE"] == 64
    assert 1 << k["DETECT_SCAN_STEPS"] == k["DETECT_THREADS"] and k["DETECT_SCAN_CHUNK"] == k["DETECT_THREADS"] * k["DETECT_SCAN_ITEMS"]
    for fn in ("detect_args_valid", "detect_tiles", "detect_tile_points", "detect_scan_blocks", "detect_lds_bytes", "detect_loaded", "detect_cell",
               "detect_segment", "detect_slot", "detect_reach", "detect_above", "detect_is_peak", "detect_lane_rank", "detect_segment_base",
               "detect_scan_own", "detect_scan_step", "detect_scan_write"):
        assert re.search(r"\b%s\(" % fn, core), fn
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/detect.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "detect_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    rule = mk[:mk.index("$(BUILD)/detect.o: detect.hip")].rstrip().splitlines()
    assert "no $(EXACT) is needed" in rule[-1] and "compares and copies only" in rule[-1] and rule[-1].startswith("#")
    assert "$(EXACT)" not in mk[mk.index("$(BUILD)/detect.o: detect.hip"):].split("\n")[1]
    assert os.path.exists(os.path.join(ROOT, "profiles", "detect.txt")) and os.path.exists(os.path.join(ROOT, "tools", "detect_bench.py"))
    # op_detect serves the vector as a matrix of one row and orders its checks as the header says
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        capi = f.read()
    op = capi[capi.index("int op_detect("):]
    op = op[:op.index("\n}\n")]
    assert (op.index("detect_args_valid(") < op.index("erroneous()") < op.index("BDSP_ERR_MUST_BE_REAL") < op.index("BDSP_ERR_SAME_SIZE")
            < op.index("BDSP_ERR_META_DATA") < op.index("BDSP_ERR_UNSUPPORTED") < op.index("detect_rows<T>("))
    assert "op_detect<T>(H<T>(vector), 1, true," in capi and "op_detect<T>(&a->v, a->rows, false," in capi
    assert "trade()" not in op  # x is not modified


def test_detect_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/detect.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_detect_kernels_use_no_scratch(tmp_path):
    """Every k_detect_ kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_detect_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # the count and the write kernel for f32 / f64, and the two prefix kernels
    assert len(found) == 6, sorted(found)
    for part, copies in (("k_detect_countI", 2), ("k_detect_writeI", 2), ("k_detect_scan_tiles", 1), ("k_detect_scan_rows", 1)):
        assert len([n for n in found if part in n]) == copies, (part, sorted(found))
    assert not {k: v for k, v in found.items() if v}, found


def test_the_shapes_file_covers_what_it_must():
    k = core_constants()
    tile, max_order, chunk = k["DETECT_TILE"], k["DETECT_MAX_ORDER"], k["DETECT_SCAN_CHUNK"]
    sh = shapes()
    assert all(b in ("open", "wrap", "nearest") and kind in KINDS and 0 <= order <= max_order for _, _, order, b, kind in sh)
    # nothing larger than the chunk line and 7 x 2065
    assert all((rows in (1, 7) and 1 <= n <= 2 * tile + 17) or (rows, n) == (chunk + 3, 3) for rows, n, _, _, _ in sh)
    assert {n for _, n, _, _, _ in sh} >= {1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 17}
    assert [s for s in sh if s[0] == 1] and [s for s in sh if s[0] == 7] and {s[1:] for s in sh if s[0] == 7} <= {s[1:] for s in sh if s[0] == 1}
    assert [s for s in sh if s[0] > 1 and s[1] % 4 and s[1] > tile]  # f32 rows off the 16-byte boundary, more than one tile
    assert {0, 1, 2, max_order} <= {order for _, _, order, _, _ in sh}
    assert [s for s in sh if tile < 2 * s[2] < 2 * max_order and s[1] > tile]  # a halo longer than the tile, on more than one tile
    for boundary in ("open", "wrap", "nearest"):
        assert [s for s in sh if s[3] == boundary and s[2] >= s[1]], boundary  # order >= n
        assert [s for s in sh if s[3] == boundary and s[0] > 1 and s[1] > tile], boundary
    assert [s for s in sh if s[3] == "wrap" and s[2] >= 2 * s[1]]  # more than one turn
    assert {kind for _, _, _, _, kind in sh} == set(KINDS)
    assert [s for s in sh if (s[0], s[1]) == (chunk + 3, 3)]  # both prefix launches loop
    assert [s for s in sh if s[4] == "scalar-inf" and s[2] == 0 and s[1] % tile == 0]  # dense: every cell of full tiles
    assert [s for s in sh if s[4] == "scalar-inf" and s[2] == 0 and s[1] == 2 * tile]


def test_core_functions_on_the_host(tmp_path):
    """tests/host_sim/sim_detect.cpp, a stand-alone program with its own main, built with the host compiler once plainly and
    once with -fsanitize=address,undefined and run as its own process on tests/detect_shapes.txt: every detection written
    exactly once at the slot a serial scan gives, nothing at or beyond the capacity; every LDS slot inside the allocation
    and written before it is read; the boundary index against a brute-force walk; the ballot and prefix arithmetic against
    a serial count across the wave and step seams; the 64-bit prefixes over more entries than one chunk."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_detect.cpp")
    with open(src) as f:
        text = f.read()
    assert re.search(r"^int main\(int argc, char\*\* argv\)", text, re.M) and '#include "../../basic_dsp_amd/csrc/detect_core.h"' in text
    assert "hip" not in re.sub(r"detect\.hip", "", text).lower()
    n_lines = len(shapes())
    for flags, name in (([], "sim_detect"), (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], "sim_detect_san")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, src])
        r = subprocess.run([exe, SHAPES_FILE], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        assert "%d shape lines (both precisions), %d cases" % (n_lines, 2 * n_lines) in r.stdout
        for pattern in (r"^detections: (\d+) writes, each slot below min\(total, capacity\) exactly once at its serial place, none at or beyond the capacity$",
                        r"^LDS: (\d+) accesses, all inside the allocation and written before read$",
                        r"^boundary index: (\d+) positions agree with the brute-force walk$",
                        r"^ballot and prefix arithmetic: (\d+) segments, \d+ lane ranks agree with the serial count$",
                        r"^64-bit prefixes: (\d+) entries scanned, sums past 2\^32 over more than one chunk$"):
            m = re.search(pattern, r.stdout, re.M)
            assert m and int(m.group(1)) > 0, (pattern, r.stdout[-800:])
        assert re.search(r"^0 failures$", r.stdout, re.M)
