"""CPU-only checks of rank_filter and medfilt (sliding order statistics along a DspVec or along every row of a DspMat on the
device): the header declares the four entry points and names their codes, the built library exports them with the stated
prototypes, the Python functions are module-level while DspVec and DspMat gained no name, rank_filter.hip and
rank_filter_core.h have no atomic operation, no environment variable and no function-level static, each crossover constant
says whether it was measured, the unit is in the Makefile and builds without a warning, its kernels use no scratch, the
TypeErrors come before any device is touched, tests/rank_filter_shapes.txt covers what it must, and the key map, the
boundary index, the LDS map, both selectors and the count selector's bank behaviour hold on the host for every line of it
(tests/host_sim/sim_rank_filter.cpp, a stand-alone program built plainly and with the address and undefined-behaviour
sanitizers)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
NAMES = ("bdsp_hip_rank_filter32", "bdsp_hip_mat_rank_filter32", "bdsp_hip_rank_filter64", "bdsp_hip_mat_rank_filter64")
SHAPES_FILE = os.path.join(ROOT, "tests", "rank_filter_shapes.txt")


def core_constants():
    with open(os.path.join(CSRC, "rank_filter_core.h")) as f:
        core = f.read()
    return {k: int(v) for k, v in re.findall(r"^constexpr int (RANK_\w+) = (\d+);", core, re.M)}


def shapes():
    """[(rows, n, half, rank, guard or None, boundary)] of tests/rank_filter_shapes.txt"""
    out = []
    for line in open(SHAPES_FILE):
        if line.strip() and not line.startswith("#"):
            rows, n, half, rank, guard, boundary = line.split()
            out.append((int(rows), int(n), int(half), int(rank), None if guard == "none" else int(guard), boundary))
    return out


def window_size(half, guard):
    return 2 * half + 1 if guard is None else 2 * (half - guard)


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
        assert fn.argtypes == [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int64, C.c_int32], name
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for sfx in ("32", "64"):
        for proto in ("int32_t bdsp_hip_rank_filter%s(VecBuf%s *v, size_t half, size_t rank, int64_t guard /* -1: none */, int32_t boundary);",
                      "int32_t bdsp_hip_mat_rank_filter%s(MatBuf%s *m, size_t half, size_t rank, int64_t guard /* -1: none */, int32_t boundary);"):
            assert proto % (sfx, sfx) in hdr, proto % (sfx, sfx)
    assert hdr.index("int32_t bdsp_hip_mat_sosfilt32(") < hdr.index("/* rank_filter:") < hdr.index("int32_t bdsp_hip_rank_filter32(")  # after the sosfilt block
    assert hdr.index("int32_t bdsp_hip_mat_sosfilt64(") < hdr.index("see bdsp_hip_rank_filter32 */") < hdr.index("int32_t bdsp_hip_rank_filter64(")
    comment = hdr[hdr.index("/* rank_filter:"):hdr.index("int32_t bdsp_hip_rank_filter32(")]
    assert comment.count("/*") == 1  # one comment block
    comment = re.sub(r"\s*\n \*\s*", " ", comment)  # (one line: a phrase may be wrapped)
    for word in ("Codes: 0", "7, with the data untouched", "rank >= W", "guard >= half", "unknown boundary", "-1 for a poisoned",
                 "4 (BDSP_ERR_MUST_BE_REAL) for complex data", "BDSP_ERR_UNSUPPORTED for half above 1024 (RANK_MAX_HALF)", "rows x tiles above 2^31",
                 "No rows, or rows of no points", "guard < |d| <= half", "W = 2 half + 1", "2 (half - guard)", "as it was on entry", "+0.0",
                 "scipy.signal.medfilt", "wraps more than once", "first or last point", "totalOrder", "-NaN < -inf", "-0 < +0", "+inf < +NaN",
                 "bits ^ (sign ? all ones : sign bit)", "exactly the bits of the selected input", "NaN payloads and denormals", "no flush",
                 "trade buffer", "No atomics", "no early exit", "Deterministic", "CU count", "bit-equal", "one launch"):
        assert word in comment, word
    assert core_constants()["RANK_MAX_HALF"] == 1024  # (the figure the comment prints)


def test_the_functions_are_module_level_and_the_classes_gained_no_name():
    import inspect
    import numpy as np
    import basic_dsp_amd as b
    import importlib
    module = importlib.import_module("basic_dsp_amd.rank_filter")  # (the package attribute of that name is the function)
    assert b.rank_filter is module.rank_filter and b.medfilt is module.medfilt
    assert "rank_filter" in b.__all__ and "medfilt" in b.__all__
    assert str(inspect.signature(b.rank_filter)) == "(x, half, rank, guard=None, boundary='zero')"
    assert str(inspect.signature(b.medfilt)) == "(x, kernel_size=3, boundary='zero')"
    for word in ("totalOrder", "-NaN < -inf", "exactly the bits of the selected input", "NaN payloads and denormals", "TypeError",
                 "Deterministic", "bit-equal", "guard < |d| <= half", "as it was on entry", "wraps more than", "scipy.signal.medfilt"):
        assert word in " ".join(b.rank_filter.__doc__.split()), word  # (a phrase may be wrapped)
    for word in ("scipy.signal.medfilt", "same C entry", "even or zero", "totalOrder", "TypeError"):
        assert word in " ".join(b.medfilt.__doc__.split()), word
    for cls in (b.DspVec, b.DspMat):
        assert not [n for n in dir(cls) if "rank" in n.lower() or "med" in n.lower() or "filt" in n.lower()], cls
    for bad in ([1.0, 2.0], np.ones((2, 8), dtype=np.float32), None, "x"):  # (no device is touched before the type check)
        with pytest.raises(TypeError):
            b.rank_filter(bad, 1, 1)
        with pytest.raises(TypeError):
            b.rank_filter(bad, 1, 5, guard=3, boundary="no such rule")  # (the type comes before the arguments)
        with pytest.raises(TypeError):
            b.medfilt(bad)
        with pytest.raises(TypeError):
            b.medfilt(bad, 4)
    # Python-side argument errors answer 7 without a device call: a handle that names no device object would not survive one
    for cls in (b.DspVec, b.DspMat):
        fake = cls(_handle=1, _sfx="32")
        try:
            assert b.rank_filter(fake, 1, 1, boundary="reflect") == 7 and b.rank_filter(fake, 1, 1, boundary=0) == 7
            assert b.rank_filter(fake, -1, 0) == 7 and b.rank_filter(fake, 1, -1) == 7 and b.rank_filter(fake, 1.0, 0) == 7
            assert b.rank_filter(fake, 2, 0, guard=-1) == 7 and b.rank_filter(fake, 2, 0, guard="0") == 7
            assert b.medfilt(fake, 0) == 7 and b.medfilt(fake, 4) == 7 and b.medfilt(fake, -3) == 7 and b.medfilt(fake, 3.0) == 7
        finally:
            fake._h = None  # (nothing to delete)


def test_the_unit_has_no_atomic_and_is_in_the_makefile():
    with open(os.path.join(CSRC, "rank_filter.hip")) as f:
        unit = f.read()
    with open(os.path.join(CSRC, "rank_filter_core.h")) as f:
        core = f.read()
    assert "atomic" not in unit.lower() and "atomic" not in core.lower()
    assert "getenv" not in unit and "getenv" not in core  # no environment variable
    assert set(re.findall(r"\bvoid (k_\w+)\(", unit)) == {"k_rank_tile"}
    assert '#include "rank_filter_core.h"' in unit
    # the core is plain C++: no HIP include, the markers only under __HIPCC__
    assert "hip/" not in core and "bdsp_internal.h" not in core
    assert re.search(r"#if defined\(__HIPCC__\)\n#define BDSP_RANK_HD __host__ __device__ __forceinline__\n#else\n#define BDSP_RANK_HD inline\n#endif", core)
    # no function-level static, no experiment switch
    for text in (unit, core):
        assert not re.search(r"^\s+static\s+(?!_assert)", text.replace("static_assert", "static__assert"), re.M)
        assert "thread_local" not in text and "#ifdef" not in text and "#ifndef" not in text
    # dynamic LDS goes through kernel_lds, on the line before the one launch
    launches = list(re.finditer(r"hipLaunchKernelGGL\(kern,", unit))
    assert len(launches) == 1 and len(re.findall(r"BDSP_TRY\(kernel_lds\(kern, lds\)\);", unit)) == 1
    assert "kernel_lds(kern, lds)" in unit[:launches[0].start()].rstrip().splitlines()[-1]
    assert "hipFuncSetAttribute" not in unit
    # rows need not be aligned: no vector type, integers in and out, no floating-point type in the kernel
    kernel = unit[unit.index("__global__"):unit.index("template <typename K, bool COUNT>\nstatic int rank_launch")]
    assert not re.search(r"\b(float|double|float[24]|double2|uint4|int4|uint2)\b", kernel)
    # every dispatch constant is named, and its line cites the profile or says that nobody measured it
    for name in ("RANK_TILE", "RANK_MAX_HALF", "RANK_CROSS_F32", "RANK_CROSS_F64"):
        m = re.search(r"^constexpr int %s = \d+;.*$" % name, core, re.M)
        assert m, name
        assert "not measured" in m.group(0) or ("measured" in m.group(0) and "profiles/rank_filter.txt" in m.group(0)), name
    k = core_constants()
    assert k["RANK_TILE"] == k["RANK_THREADS"] * k["RANK_PER_LANE"] == 1024 and k["RANK_MAX_HALF"] == 1024
    # the selectors leave no loop early
    for fn in ("rank_select_count", "rank_select_bisect", "rank_count_segment"):
        body = core[core.index("%s(const L& lds" % fn):]
        body = body[:body.index("\n}\n")]
        assert "break" not in body and "continue" not in body and "goto" not in body and body.count("return") <= 1, fn
    for fn in ("rank_key", "rank_bits", "rank_src_index", "rank_window", "rank_window_size", "rank_args_valid", "rank_uses_count",
               "rank_lds_keys", "rank_loaded", "rank_out_index", "rank_tile_points"):
        assert re.search(r"\b%s\(" % fn, core), fn
    assert "totalOrder" in core and "conflict-free" in core and "NaN payloads" in core
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/rank_filter.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "rank_filter_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    rule = mk[:mk.index("$(BUILD)/rank_filter.o: rank_filter.hip")].rstrip().splitlines()
    assert "no $(EXACT) is needed" in rule[-1] and "no floating-point arithmetic at all" in rule[-1] and rule[-1].startswith("#")
    assert "$(EXACT)" not in mk[mk.index("$(BUILD)/rank_filter.o: rank_filter.hip"):].split("\n")[1]
    assert os.path.exists(os.path.join(ROOT, "profiles", "rank_filter.txt")) and os.path.exists(os.path.join(ROOT, "tools", "rank_filter_bench.py"))
    # op_rank_filter orders its checks as op_sosfilt does: arguments, poisoned, number kind; then the trade
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        capi = f.read()
    op = capi[capi.index("int op_rank_filter("):]
    op = op[:op.index("\n}\n")]
    assert op.index("rank_args_valid(") < op.index("erroneous()") < op.index("BDSP_ERR_MUST_BE_REAL") < op.index("BDSP_ERR_UNSUPPORTED") < op.index("v->trade();")
    assert "v->data, v->buf" in op


def test_rank_filter_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/rank_filter.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_rank_filter_kernels_use_no_scratch(tmp_path):
    """Every k_rank_ kernel of the shipped library: present, .private_segment_fixed_size 0."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_rank_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # the tile kernel for 32- / 64-bit keys x the count / bisect selector
    assert len(found) == 4 and all("k_rank_tileI" in n for n in found), sorted(found)
    assert not {k: v for k, v in found.items() if v}, found


def test_the_shapes_file_covers_what_it_must():
    k = core_constants()
    tile, max_half = k["RANK_TILE"], k["RANK_MAX_HALF"]
    sh = shapes()
    assert all(1 <= rows <= 8 and 1 <= n <= 2 * tile + 17 and half <= max_half for rows, n, half, _, _, _ in sh)
    assert all(rank < window_size(half, guard) and (guard is None or 0 <= guard < half) for _, _, half, rank, guard, _ in sh)
    assert {n for _, n, _, _, _, _ in sh} >= {1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 17}
    assert [s for s in sh if s[0] > 1 and s[1] % 4 and s[1] > tile]  # f32 rows off the 16-byte boundary, more than one tile
    assert {0, 1, max_half} <= {half for _, _, half, _, _, _ in sh}
    for boundary in ("zero", "wrap", "nearest"):
        assert [s for s in sh if s[5] == boundary and s[2] >= s[1]], boundary  # half >= n
        assert [s for s in sh if s[5] == boundary and s[0] > 1 and s[1] > tile], boundary
    assert [s for s in sh if s[5] == "wrap" and s[2] >= 2 * s[1]]  # the window wraps more than once
    assert [s for s in sh if 2 * s[2] > tile and s[1] > tile]  # a halo longer than the tile, on more than one tile
    for cross in (k["RANK_CROSS_F32"], k["RANK_CROSS_F64"]):
        for w in (cross - 1, cross, cross + 1):
            assert [s for s in sh if window_size(s[2], s[4]) == w and s[1] >= tile - 1], w
    assert max(window_size(s[2], s[4]) for s in sh) == 2 * max_half + 1
    ranks = {(0 if rank == 0 else "top" if rank == window_size(half, guard) - 1 else "median" if rank == (window_size(half, guard) - 1) // 2 else "other")
             for _, _, half, rank, guard, _ in sh if window_size(half, guard) >= 5}
    assert ranks == {0, "top", "median", "other"}
    assert [s for s in sh if s[4] is None] and [s for s in sh if s[4] == 0] and [s for s in sh if s[4] is not None and s[4] == s[2] - 1 and s[2] > 1]
    assert [s for s in sh if s[0] == 1] and [s for s in sh if s[0] == 7] and {(s[1:]) for s in sh if s[0] == 7} <= {(s[1:]) for s in sh if s[0] == 1}


def test_core_functions_on_the_host(tmp_path):
    """tests/host_sim/sim_rank_filter.cpp, a stand-alone program with its own main, built with the host compiler once
    plainly and once with -fsanitize=address,undefined and run as its own process on tests/rank_filter_shapes.txt: every
    output written exactly once; every LDS slot inside the allocation and written before it is read; the boundary index
    against a brute-force walk; the key map a strictly monotone bijection on the edge patterns; both selectors against
    std::sort on every window; consecutive lanes of the count selector read consecutive slots with no extra bank cycle."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_rank_filter.cpp")
    with open(src) as f:
        text = f.read()
    assert re.search(r"^int main\(int argc, char\*\* argv\)", text, re.M) and '#include "../../basic_dsp_amd/csrc/rank_filter_core.h"' in text
    assert "hip" not in re.sub(r"rank_filter\.hip", "", text).lower()
    n_lines = len(shapes())
    for flags, name in (([], "sim_rank_filter"), (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], "sim_rank_filter_san")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, src])
        r = subprocess.run([exe, SHAPES_FILE], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        assert "%d shape lines (both key widths, both selectors), 0 failures" % n_lines in r.stdout
        assert re.search(r"^key map: strictly monotone bijection on 22 edge patterns per width$", r.stdout, re.M)
        m = re.search(r"^count selector LDS reads: f32 (\d+) group steps, 0 extra bank cycles; f64 (\d+) group steps, 0 extra bank cycles$", r.stdout, re.M)
        assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, r.stdout[-600:]
