"""CPU-only checks of sort, argsort, top_k, quantile and median (the order statistics of a DspVec or of every row of a DspMat
on the device): the header declares the eight entry points after the detect block and names their codes, the built library
exports them with the stated prototypes, the Python functions are module-level while DspVec and DspMat gained no name, the
TypeErrors and the Python-side argument errors come before any device is touched, sort.hip and sort_core.h have no atomic
operation, no environment variable, no function-level static and no experiment switch, each dispatch constant says whether
it was measured, the unit is in the Makefile and builds without a warning, its kernels use no scratch, tests/sort_shapes.txt
covers what it must, and the network, the LDS map and the merge-path split hold on the host for every line of it
(tests/host_sim/sim_sort.cpp, a stand-alone program built plainly and with the address and undefined-behaviour
sanitizers)."""
import os
import re
import struct
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
NAMES = tuple("bdsp_hip_%s%s%s" % (m, f, s) for s in ("32", "64") for m in ("", "mat_") for f in ("sort", "order_select"))
SHAPES_FILE = os.path.join(ROOT, "tests", "sort_shapes.txt")


def core_constants():
    with open(os.path.join(CSRC, "sort_core.h")) as f:
        core = f.read()
    return {k: int(v) for k, v in re.findall(r"^constexpr int (SORT_\w+) = (\d+);", core, re.M)}


def shapes():
    """[(rows, n)] of tests/sort_shapes.txt"""
    out = []
    for line in open(SHAPES_FILE):
        if line.strip() and not line.startswith("#"):
            rows, n = line.split()
            out.append((int(rows), int(n)))
    return out


def test_header_declares_and_library_exports_the_8_entry_points():
    import ctypes as C
    import basic_dsp_amd._lib as L
    assert len(NAMES) == 8
    declared = set(declared_functions())
    assert not [n for n in NAMES if n not in declared]
    lib = C.CDLL(L.LIB_PATH)
    assert not [n for n in NAMES if not hasattr(lib, n)]
    for name in NAMES:
        fn = getattr(L.lib, name)
        assert fn.restype is C.c_int32, name
        if "order_select" in name:
            assert fn.argtypes == [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p], name
        else:
            assert fn.argtypes == [C.c_void_p, C.c_int32], name
    with open(os.path.join(ROOT, "include", "basic_dsp_hip.h")) as f:
        hdr = f.read()
    for sfx in ("32", "64"):
        for proto in ("int32_t bdsp_hip_sort%s(VecBuf%s *v, int32_t descending);",
                      "int32_t bdsp_hip_mat_sort%s(MatBuf%s *m, int32_t descending);",
                      "int32_t bdsp_hip_order_select%s(const VecBuf%s *v, int32_t descending, size_t count, const uint64_t *ranks, int64_t *index, void *value);",
                      "int32_t bdsp_hip_mat_order_select%s(const MatBuf%s *m, int32_t descending, size_t count, const uint64_t *ranks, int64_t *index, void *value);"):
            assert proto % (sfx, sfx) in hdr, proto % (sfx, sfx)
    assert ("/* the elements of sorted ranks ranks[0..count) of every row, as rows x count row-major entries; ranks: a host array, each\n"
            " * < n, any order, repeats allowed; NULL: 0 .. count - 1 (count <= n).  index and value may each be NULL.  x is not modified. */\n"
            "int32_t bdsp_hip_order_select32(") in hdr
    assert hdr.index("int32_t bdsp_hip_mat_detect32(") < hdr.index("/* sort, order_select:") < hdr.index("int32_t bdsp_hip_sort32(")  # after the detect block
    assert hdr.index("int32_t bdsp_hip_mat_detect64(") < hdr.index("see bdsp_hip_sort32 */") < hdr.index("int32_t bdsp_hip_sort64(")
    comment = hdr[hdr.index("/* sort, order_select:"):hdr.index("int32_t bdsp_hip_sort32(")]
    assert comment.count("/*") == 1  # one comment block
    comment = re.sub(r"\s*\n \*\s*", " ", comment)  # (one line: a phrase may be wrapped)
    for word in ("Codes: 0", "7, with the data untouched", "not 0 or 1", "a rank at or above n", "count above n without ranks", "-1 for a poisoned",
                 "4 (BDSP_ERR_MUST_BE_REAL) for complex data", "BDSP_ERR_UNSUPPORTED for n at or above 2^32", "rows x tiles above 2^31",
                 "No rows, or rows of no points", "totalOrder", "-NaN < -inf", "-0 < +0", "+inf < +NaN", "bits ^ (sign ? all ones : sign bit)",
                 "ties are broken by ascending index", "complemented key", "the lower index first", "not the reverse of the ascending permutation",
                 "exactly the bits of the selected input", "NaN payloads and denormals", "no flush", "trade buffer", "1 + P launches", "2 + P launches",
                 "P = ceil(log2(ceil(n / 4096)))", "merge path", "ties to the left run", "rows x n x (4 + 4) or (8 + 4)", "one synchronisation",
                 "No atomics", "no loop leaves early", "Deterministic", "CU count", "equals the vector call", "the full sort and a crop"):
        assert word in comment, word
    k = core_constants()
    assert k["SORT_TILE"] == 4096 and k["SORT_THREADS"] == 256  # (the figures the comment prints)


def test_the_functions_are_module_level_and_the_classes_gained_no_name():
    import importlib
    import inspect
    import numpy as np
    import basic_dsp_amd as b
    module = importlib.import_module("basic_dsp_amd.sorting")
    names = ("sort", "argsort", "top_k", "quantile", "median")
    for name in names:
        assert getattr(b, name) is getattr(module, name) and name in b.__all__, name
    assert str(inspect.signature(b.sort)) == "(x, descending=False)" and str(inspect.signature(b.argsort)) == "(x, descending=False)"
    assert str(inspect.signature(b.top_k)) == "(x, k, largest=True)" and str(inspect.signature(b.median)) == "(x)"
    assert str(inspect.signature(b.quantile)) == "(x, q, method='linear')"
    for word in ("totalOrder", "-NaN < -inf", "exactly the bits of the inputs", "NaN payloads and denormals", "TypeError", "Deterministic",
                 "1 + P launches", "bit-equal"):
        assert word in " ".join(b.sort.__doc__.split()), word  # (a phrase may be wrapped)
    for word in ("stable", "not the reverse of the ascending permutation", "2 + P launches", "x is not modified"):
        assert word in " ".join(b.argsort.__doc__.split()), word
    for word in ("the full sort and a crop", "k > n", "exactly the bits of x[row, index]", "x is not modified"):
        assert word in " ".join(b.top_k.__doc__.split()), word
    for word in ("p = q (n - 1)", "lo = floor(p)", "hi = min(lo + 1, n - 1)", "equal bits", "differs from numpy", "one NaN poisons", "in double",
                 "x is not modified"):
        assert word in " ".join(b.quantile.__doc__.split()), word
    assert "quantile(x, 0.5)" in b.median.__doc__
    for cls in (b.DspVec, b.DspMat):
        assert not [n for n in dir(cls) if "sort" in n.lower() or "quantile" in n.lower() or "median" in n.lower() or "top_k" in n.lower()], cls
    calls = (lambda x: b.sort(x), lambda x: b.sort(x, 7), lambda x: b.argsort(x), lambda x: b.argsort(x, "no"), lambda x: b.top_k(x, 1),
             lambda x: b.top_k(x, -1), lambda x: b.quantile(x, 0.5), lambda x: b.quantile(x, 2.0, "no such method"), lambda x: b.median(x))
    for bad in ([1.0, 2.0], np.ones((2, 8), dtype=np.float32), None, "x"):  # (no device is touched before the type check,
        for call in calls:                                                  # and the type comes before the arguments)
            with pytest.raises(TypeError):
                call(bad)
    # Python-side argument errors answer 7 without a device call: a handle that names no device object would not survive one
    for cls in (b.DspVec, b.DspMat):
        fake = cls(_handle=1, _sfx="32")
        try:
            assert b.sort(fake, 2) == 7 and b.sort(fake, None) == 7 and b.sort(fake, "yes") == 7 and b.sort(fake, 1.0) == 7
            assert b.argsort(fake, 2) == (7, None) and b.argsort(fake, None) == (7, None)
            assert b.top_k(fake, 1.5) == (7, None) and b.top_k(fake, -1) == (7, None) and b.top_k(fake, "3") == (7, None)
            assert b.top_k(fake, 1, largest=None) == (7, None) and b.top_k(fake, 1, largest=2) == (7, None)
            for q in (-0.001, 1.001, float("nan"), float("inf"), [0.5, 1.5], [0.5, float("nan")], "0.5", None, True, [[0.5]], 1j):
                assert b.quantile(fake, q) == (7, None), q
            for method in ("nearest", "midpoint", "", None, 0):
                assert b.quantile(fake, 0.5, method) == (7, None), method
        finally:
            fake._h = None  # (nothing to delete)


def test_the_unit_has_no_atomic_and_is_in_the_makefile():
    with open(os.path.join(CSRC, "sort.hip")) as f:
        unit = f.read()
    with open(os.path.join(CSRC, "sort_core.h")) as f:
        core = f.read()
    assert "atomic" not in unit.lower() and "atomic" not in core.lower()
    assert "getenv" not in unit and "getenv" not in core  # no environment variable
    assert set(re.findall(r"\bvoid (k_\w+)\(", unit)) == {"k_sort_tile", "k_sort_merge", "k_sort_gather"}
    assert '#include "sort_core.h"' in unit and '#include "rank_filter_core.h"' in core
    # the core is plain C++: no HIP include, the markers only under __HIPCC__
    assert "hip/" not in core and "bdsp_internal.h" not in core and "__syncthreads" not in core and "threadIdx" not in core
    assert re.search(r"#if defined\(__HIPCC__\)\n#define BDSP_SORT_HD __host__ __device__ __forceinline__\n#define BDSP_SORT_UNROLL _Pragma\(\"unroll\"\)\n"
                     r"#else\n#define BDSP_SORT_HD inline\n#define BDSP_SORT_UNROLL\n#endif", core)
    assert core.count("__HIPCC__") == 1 and "__device__" not in core.replace("#define BDSP_SORT_HD __host__ __device__", "")
    # no function-level static, no experiment switch
    for text in (unit, core):
        assert not re.search(r"^\s+static\s+(?!_assert)", text.replace("static_assert", "static__assert"), re.M)
        assert "thread_local" not in text and "#ifdef" not in text and "#ifndef" not in text
    # dynamic LDS goes through kernel_lds, on the line before each of the two launches that use it
    launches = list(re.finditer(r"hipLaunchKernelGGL\(kern,", unit))
    assert len(launches) == 2 and len(re.findall(r"BDSP_TRY\(kernel_lds\(kern, lds\)\);", unit)) == 2
    for launch in launches:
        assert "kernel_lds(kern, lds)" in unit[:launch.start()].rstrip().splitlines()[-1]
    assert len(re.findall(r"hipLaunchKernelGGL\(", unit)) == 3 and "hipLaunchKernelGGL(k_sort_gather<K>, dim3((unsigned)blocks), dim3(SORT_THREADS), 0, s," in unit
    assert "hipFuncSetAttribute" not in unit
    # rows need not be aligned: no vector type, integers in and out, no floating-point type in the kernels or the core
    kernels = unit[unit.index("template <int FROM, int TO"):unit.index("template <typename K, bool INDEX>\nstatic int sort_launch_tile")]
    assert kernels.count("__global__") == 3
    for text in (kernels, core[core.index("#pragma once"):]):
        assert not re.search(r"\b(float|double|float[24]|double2|uint4|int4|uint2)\b", text)
    # register arrays are indexed under unrolled loops only
    assert len(re.findall(r"#pragma unroll\n    for \(int r = 0; r < SORT_PER_LANE; \+\+r\)", kernels)) == 4
    assert len(re.findall(r"BDSP_SORT_UNROLL\n\s+for \(", core)) == 5 and len(re.findall(r"\n\s+for \(", core[core.index("struct SortRegs"):core.index("struct SortMerge")])) == 5
    # every dispatch constant is named, and its line cites the profile or says that nobody measured it
    for name in ("SORT_TILE", "SORT_PER_LANE"):
        m = re.search(r"^constexpr int %s = \d+;.*$" % name, core, re.M)
        assert m, name
        assert "not measured" in m.group(0) or ("measured" in m.group(0) and "profiles/sort.txt" in m.group(0)), name
    k = core_constants()
    assert k["SORT_TILE"] == k["SORT_THREADS"] * k["SORT_PER_LANE"] == 4096 == 1 << k["SORT_TILE_LOG2"]
    # the network and the split leave no loop early
    for fn in ("sort_steps(SortRegs", "sort_cmpx(SortRegs", "sort_split_step(const A& a", "sort_first_stages(SortRegs", "sort_lds_store(const LK& lk",
               "sort_lds_load(const LK& lk"):
        body = core[core.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "break" not in body and "continue" not in body and "goto" not in body and "return" not in body, fn
    for fn in ("sort_to_key", "sort_to_bits", "sort_plan", "sort_supported", "sort_lds_bytes", "sort_tile_cell", "sort_slot", "sort_phys",
               "sort_merge_geom", "sort_split_steps", "sort_split_range", "sort_merge_source"):
        assert re.search(r"\b%s\(" % fn, core), fn
    assert "totalOrder" in core and "NaN payloads" in core and "rank_key<K>(bits)" in core and "rank_bits<K>(" in core
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "$(BUILD)/sort.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    assert "sort_core.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1)
    rule = mk[:mk.index("$(BUILD)/sort.o: sort.hip")].rstrip().splitlines()
    assert "no $(EXACT) is needed" in rule[-1] and "no floating-point arithmetic at all" in rule[-1] and rule[-1].startswith("#")
    assert "$(EXACT)" not in mk[mk.index("$(BUILD)/sort.o: sort.hip"):].split("\n")[1]
    assert os.path.exists(os.path.join(ROOT, "profiles", "sort.txt")) and os.path.exists(os.path.join(ROOT, "tools", "sort_bench.py"))
    # op_sort and op_order_select order their checks as op_rank_filter and op_detect do: arguments, poisoned, number kind, unsupported
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        capi = f.read()
    op = capi[capi.index("int op_sort("):]
    op = op[:op.index("\n}\n")]
    assert op.index("BDSP_ERR_ARG_LENGTH") < op.index("erroneous()") < op.index("BDSP_ERR_MUST_BE_REAL") < op.index("BDSP_ERR_UNSUPPORTED") < op.index("v->trade();")
    assert "v->data, v->buf" in op and "if (in_buf) v->trade();" in op
    op = capi[capi.index("int op_order_select("):]
    op = op[:op.index("\n}\n")]
    assert op.rindex("BDSP_ERR_ARG_LENGTH") < op.index("BDSP_ERR_POISONED") < op.index("BDSP_ERR_MUST_BE_REAL") < op.index("BDSP_ERR_UNSUPPORTED")
    assert op.count("hipStreamSynchronize") == 1 and "v->trade" not in op and "hipMemcpyHostToDevice" in op


def test_sort_builds_without_warnings(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    build = str(tmp_path / "b")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, build + "/sort.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in (r.stdout + r.stderr).lower(), (r.stdout + r.stderr)[-4000:]


def test_sort_kernels_use_no_scratch(tmp_path):
    """Every k_sort_ kernel of the shipped library: present, .private_segment_fixed_size 0 (from the kernel metadata notes)."""
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
                nm = re.search(r"\.name:\s+(_Z\S*k_sort_\S+)", blk)
                sz = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and sz:
                    found[nm.group(1)] = int(sz.group(1))
    # tile and merge for 32- / 64-bit keys x with / without index, gather for the two key widths
    assert len(found) == 10, sorted(found)
    assert sum("k_sort_tileI" in n for n in found) == 4 and sum("k_sort_mergeI" in n for n in found) == 4 and sum("k_sort_gatherI" in n for n in found) == 2
    assert not {k: v for k, v in found.items() if v}, found


def test_the_shapes_file_covers_what_it_must():
    tile = core_constants()["SORT_TILE"]
    sh = shapes()
    wanted = {1, 2, 3, 63, 64, 65, 100, tile // 2 - 1, tile // 2, tile // 2 + 1, tile - 1, tile, tile + 1, 2 * tile + 17, 5 * tile + 3, 8 * tile}
    for rows in (1, 7):
        assert {n for r, n in sh if r == rows} >= wanted, rows
    assert all(rows >= 1 and n >= 1 and rows * n <= 8 * tile * 7 for rows, n in sh)
    assert [s for s in sh if s[0] > tile // 64 and s[1] in (63, 65)]  # rows share workgroups, the last one partly empty
    assert [s for s in sh if s[0] > tile // 64 and s[1] in (63, 65) and s[0] % (tile // 64)]
    assert [s for s in sh if s[0] > 1 and s[1] % 2 and s[1] > tile]  # f32 rows off the 16-byte boundary, more than one tile
    assert [s for s in sh if -(-s[1] // tile) % 2 and s[1] > 2 * tile]  # an odd number of runs: a lone last run


def test_core_functions_on_the_host(tmp_path):
    """tests/host_sim/sim_sort.cpp, a stand-alone program with its own main, built with the host compiler once plainly and
    once with -fsanitize=address,undefined and run as its own process on tests/sort_shapes.txt: every output of every
    launch written exactly once; every LDS word inside the allocation and written before it is read; every merge-path split
    unique, monotone and summing to the outputs produced; keys and indices equal to std::stable_sort; no pad in an output;
    the bank cycles of every LDS store and load counted."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_sort.cpp")
    with open(src) as f:
        text = f.read()
    assert re.search(r"^int main\(int argc, char\*\* argv\)", text, re.M) and '#include "../../basic_dsp_amd/csrc/sort_core.h"' in text
    assert "hip" not in re.sub(r"sort\.hip", "", text).lower()
    assert "std::stable_sort" in text
    n_lines = len(shapes())
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = " ".join(f.read().split())
    for flags, name in (([], "sim_sort"), (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], "sim_sort_san")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, src])
        r = subprocess.run([exe, SHAPES_FILE], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        assert "%d shape lines (both key widths, both directions, with and without index), 0 failures" % n_lines in r.stdout
        m = re.search(r"^LDS bank cycles of the layout changes: f32 (\d+) group steps, (\d+) extra bank cycles; f64 (\d+) group steps, (\d+) extra bank cycles$",
                      r.stdout, re.M)
        assert m and int(m.group(1)) > 0 and int(m.group(3)) > 0, r.stdout[-600:]
        # DESIGN.md states the counted figure, whatever it is
        assert "%s extra bank cycles in %s group steps (f32) and %s in %s (f64)" % (m.group(2), m.group(1), m.group(4), m.group(3)) in design
