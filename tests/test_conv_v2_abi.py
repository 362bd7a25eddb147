"""CPU-only checks of the second-generation block convolution (k_overlap_save_v2): its schedule -- the plan of a launch
and the kernel's index functions -- lives in conv_v2_core.h, a host+device header without a HIP runtime call that the
library and the host simulation both compile; the simulation (tests/host_sim/sim_conv_v2.cpp, built plainly and with the
address and undefined-behaviour sanitizers) walks the kernel's loops for every case of its sweep and runs the block chain
against a long double convolution at the shapes of tests/conv_v2_shapes.txt, which tests/test_gpu_conv_routes.py reads
too."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
SHAPES = os.path.join(ROOT, "tests", "conv_v2_shapes.txt")


def read_shapes():
    """(tap counts as (M, R0, d), length rules as ("taps",) or (a, c, from R0), share overrides)."""
    taps, lens, shares = [], [], []
    for line in open(SHAPES):
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "taps":
            taps.append(tuple(int(v) for v in w[1:4]))
        elif w[0] == "len":
            lens.append(("taps",) if w[1] == "taps" else (int(w[1]), int(w[2]), int(w[3]) if len(w) > 3 else 0))
        elif w[0] == "share":
            shares.append((int(w[1]), int(w[2])))
        else:
            raise AssertionError(line)
    return taps, lens, shares


def test_the_shapes_are_the_ones_that_can_go_wrong():
    taps, lens, shares = read_shapes()
    want = {1, 2} | {256 * r + 1 for r in range(1, 13)} | {256 * (r - 1) + 2 for r in range(1, 13)}
    assert {m for m, _, _ in taps} == want
    for m, r0, d in taps:
        assert r0 == max(1, (m - 1 + 255) // 256) and d == 256 * r0 - (m - 1), m
    assert {r0 for _, r0, _ in taps} == set(range(1, 13))
    assert {d for m, _, d in taps if m > 2} == {0, 255}
    for rule in (("taps",), (1, -1, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (5, 7, 0)):
        assert rule in lens, rule
    # four overrides that bdsp_hip_dev_convolve_ex accepts (capi.cpp: first >= 1, second >= 0, first + second <= 99), two
    # of them extreme: nearly nothing and nearly everything for the first dispatch group
    assert len(shares) == 4 and len(set(shares)) == 4
    assert all(a >= 1 and b >= 0 and a + b <= 99 for a, b in shares)
    assert (1, 0) in shares and any(a + b == 99 and a >= 90 for a, b in shares)


def test_the_library_and_the_simulation_compile_the_same_schedule():
    core = open(os.path.join(CSRC, "conv_v2_core.h")).read()
    impl = open(os.path.join(CSRC, "conv_v2_impl.h")).read()
    sim = open(os.path.join(ROOT, "tests", "host_sim", "sim_conv_v2.cpp")).read()
    # host + device, no HIP runtime call, no environment variable, no atomic
    code = re.sub(r"//[^\n]*", "", core)
    assert not re.search(r"\bhip[A-Z_]\w*|#include\s*<hip|__global__|getenv|atomic", code)
    assert '#include "conv_v2_core.h"' in impl and '#include "../../basic_dsp_amd/csrc/conv_v2_core.h"' in sim
    # the plan is computed in one place: conv_v2_run calls it with the device's CU count, the simulation with its own
    assert len(re.findall(r"\bconv_v2_plan\(", impl)) == 1 and "num_cus()" in re.search(r"conv_v2_plan\([^;]*;", impl).group(0)
    assert "struct ConvV2Args" in core and "struct ConvV2Args" not in impl
    assert "xcd_contiguous(unsigned bid" in core and "xcd_contiguous(unsigned bid" not in impl
    # one r0 rule: the step, the predicate and the plan
    assert len(re.findall(r"255\) / 256", core)) == 1 and "/ 256" not in re.sub(r"//[^\n]*", "", impl)
    for fn in ("conv_v2_r0", "conv_v2_plan", "conv_v2_set_geometry", "xcd_contiguous", "conv_v2_delay", "conv_v2_in_off",
               "conv_v2_wrap_count", "conv_v2_wrap_block", "conv_v2_window_start", "conv_v2_obase", "conv_v2_store_limit",
               "conv_v2_group_lo", "conv_v2_group_hi", "conv_v2_split_id"):
        assert re.search(r"\b%s\(" % fn, core), fn
        assert re.search(r"\b%s(<\w+>)?\(" % fn, sim), fn
        # the kernel calls it, or keeps the expression inline and says which function repeats it
        assert re.search(r"\b%s(<\w+>)?\(|\b%s\b[^\n]* of conv_v2_core\.h" % (fn, fn), impl), fn
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "conv_v2_core.h" in re.search(r"^HDRS = (.*)$", f.read(), re.M).group(1)


def test_schedule_and_block_chain_on_the_host(tmp_path):
    """tests/host_sim/sim_conv_v2.cpp, a stand-alone program, built with the host compiler once plainly and once with
    -fsanitize=address,undefined.  Geometry: 3 and 2 dispatch groups x 1, 8, 256, 304 CUs x 38 tap counts (1, 2, 18, either
    side of every 256-row boundary up to 3073) x up to 22 lengths (n = taps; V, 2 V, 5 V and 4096, 8192, 12288, each - 1, + 0,
    + 1; 5 V + 7; 9 V + 7; 300 V + 5; 2200 V + 1; those below the tap count left out) x complex / real x batch 1, 3 x five
    partial runs x the default shares and the four overrides: 653 600 cases, a fifth of them (130 720) with the default
    shares.  Every block is taken by exactly one workgroup, every output is written exactly once, nothing is read or
    written outside its vector, grid is a multiple of 8 groups.  Numbers: the block chain in f32 and f64 for every R0,
    both tap forms, complex data and real pairs, against a long double convolution within 1e-6 / 1e-12."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_conv_v2.cpp")
    for flags, name in (([], "sim_conv_v2"), (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], "sim_conv_v2_san")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + flags + ["-o", exe, src])
        r = subprocess.run([exe, SHAPES], capture_output=True, text=True)
        print(r.stdout[-2000:])
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        m = re.search(r"^geometry: (\d+) cases \((\d+) element-level geometries\), 0 failures$", r.stdout, re.M)
        assert m and int(m.group(1)) == 653600 and int(m.group(1)) // 5 >= 68448 and int(m.group(2)) == 10818, r.stdout[-3000:]
        assert re.search(r"^numbers: 1310 blocks$", r.stdout, re.M)
        m = re.search(r"^numbers: worst rel-L2 per case: f32 (\d\.\d+e-\d+) \(bound 1e-06\), f64 (\d\.\d+e-\d+) \(bound 1e-12\)$", r.stdout, re.M)
        assert m and 0 < float(m.group(1)) <= 1e-6 and 0 < float(m.group(2)) <= 1e-12, r.stdout[-3000:]
        assert re.search(r"^0 failures$", r.stdout, re.M)
