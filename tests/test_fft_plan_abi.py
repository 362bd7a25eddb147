"""CPU-only checks of the global passes of a power-of-two transform above 4096 points (k_fft_pass).  What such a transform
launches -- the plan, the route of every pass (which k_fft_pass instantiation, its LDS, threads and grid), the buffer
order of the two-buffer driver and the facade's operations as transform options -- is decided in fft_plan_core.h, a
host+device header without a HIP runtime call that the library and the host simulation both compile;
tests/fft_pass_shapes.txt states the route of 434 transforms, and tests/test_gpu_fft_pass_routes.py runs those lines on the
device."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
SHAPES = os.path.join(ROOT, "tests", "fft_pass_shapes.txt")
WINDOWS = ("triangular", "hamming", "blackman_harris", "rectangular")


def read_lines():
    """(dtype, bits, batch, entry, op, route, buffers, cu_dependent) of every line of the table."""
    out = []
    for line in open(SHAPES):
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        assert w[5] == "->", line
        cu = w[-1] == "cu256"
        rest = w[6:-1] if cu else w[6:]
        out.append((w[0], int(w[1]), int(w[2]), w[3], w[4], tuple(rest[:-1]), rest[-1], cu))
    return out


def test_the_table_holds_the_lines_that_were_asked_for():
    lines = read_lines()
    have = {(d, b, n, e, o) for d, b, n, e, o, _, _, _ in lines}
    assert len(have) == len(lines)
    mag = "flags=8,scale=1,window=-1"
    for d in ("f32", "f64"):
        # every two-pass length, every facade operation, every reference window both ways, a custom window, magnitude
        for bits in range(13, 23):
            for op in ["plain_fft", "plain_ifft", "fft", "ifft", "real_plain_fft", "windowed_custom_fft", "windowed_custom_ifft"] + \
                    ["windowed_fft:" + w for w in WINDOWS] + ["windowed_ifft:" + w for w in WINDOWS]:
                assert (d, bits, 1, "vec", op) in have, (d, bits, op)
            assert (d, bits, 1, "dev", mag) in have
        # 2^19 / 2^20 alone (4-wide 1024-point tiles) and as a batch (8-wide), 2^23 (three passes), three rows
        for bits, batch in ((19, 8), (20, 4)):
            first = {(r[0], c) for dd, b, n, e, o, r, _, c in lines if (dd, b, n) == (d, bits, 1)}
            assert {f.split(":")[0] for f, _ in first} == {"1024x4"} and all(c for _, c in first)
            first = {(r[0], c) for dd, b, n, e, o, r, _, c in lines if (dd, b, n) == (d, bits, batch)}
            assert {f.split(":")[0] for f, _ in first} == {"1024x8"} and all(c for _, c in first)
        for op in ("plain_fft", "plain_ifft", "fft", "ifft", "windowed_fft:hamming", "windowed_ifft:hamming", "real_plain_fft"):
            assert (d, 23, 1, "vec", op) in have
        for bits in (13, 16, 17):
            for op in ("fft", "ifft", "windowed_fft:hamming", "real_plain_fft"):
                assert (d, bits, 3, "mat", op) in have
            assert (d, bits, 3, "dev", mag) in have
        convs = {b: o for dd, b, n, e, o, _, _, _ in lines if dd == d and e == "conv"}
        assert {14: "taps=3074", 15: "taps=4098", 16: "taps=8194"}.items() <= {b: o.split(",")[0] for b, o in convs.items()}.items()
    routes = {(d, b, n, o): r for d, b, n, e, o, r, _, _ in lines}
    # the one-workgroup kernel at 8192 points f32, two passes once a window, real input or magnitude is fused
    assert routes[("f32", 13, 1, "plain_fft")] == ("wg4",) and routes[("f64", 13, 1, "plain_fft")] == ("128x32:simple+ntl", "64x64:simple")
    assert routes[("f32", 13, 1, "windowed_fft:hamming")] == ("128x32:opts", "64x64:opts") and routes[("f32", 13, 1, mag)] == ("128x32:simple", "64x64:opts")
    # the f64 batch on the split 1024 x 8 tile: plain forward with non-temporal loads, the two fixed windows on the first
    # pass (windowed_fft) and on the last (windowed_ifft, 2^20: both passes are 1024 x 8)
    assert routes[("f64", 19, 8, "plain_fft")] == ("1024x8:simple+ntl", "512x8:simple")
    assert routes[("f64", 19, 8, "windowed_fft:triangular")][0] == "1024x8:win0+ntl" and routes[("f64", 20, 4, "windowed_fft:blackman_harris")][0] == "1024x8:win2+ntl"
    assert routes[("f64", 20, 4, "windowed_ifft:triangular")][1] == "1024x8:win0" and routes[("f64", 20, 4, "windowed_ifft:blackman_harris")][1] == "1024x8:win2"
    # three passes and their buffer order
    for d, tiles in (("f32", "256x16:simple 256x16:simple 128x32:simple"), ("f64", "256x16:simple+ntl 256x16:simple 128x32:simple")):
        assert " ".join(routes[(d, 23, 1, "plain_fft")]) == tiles
    assert {bf for d, b, n, e, o, r, bf, _ in lines if b == 23} == {"abab"}
    assert {bf for d, b, n, e, o, r, bf, _ in lines if b >= 19 and b <= 22 and e == "vec" and o == "plain_fft"} == {"abb"}
    assert {bf for d, b, n, e, o, r, bf, _ in lines if b <= 18 and e != "conv" and r != ("wg4",)} == {"aba"}


def test_the_library_and_the_simulation_compile_the_same_rule():
    core = open(os.path.join(CSRC, "fft_plan_core.h")).read()
    impl = open(os.path.join(CSRC, "fft_impl.h")).read()
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    internal = open(os.path.join(CSRC, "bdsp_internal.h")).read()
    sim = open(os.path.join(ROOT, "tests", "host_sim", "sim_fft_passes.cpp")).read()
    strip = lambda text: re.sub(r"//[^\n]*", "", text)
    # host + device, no HIP runtime call, no environment variable, nothing that needs the device
    assert not re.search(r"\bhip[A-Z_]\w*|#include\s*<hip|__global__|getenv|atomic|num_cus\(\)", strip(core))
    assert '#include "fft_plan_core.h"' in internal and '#include "../../basic_dsp_amd/csrc/fft_plan_core.h"' in sim
    # the rule is defined in one place ...
    for fn in ("plan_passes", "wg4_serves", "io_in_generic", "io_out_generic", "io_is_generic", "pass_split_exchange", "pass_lds_twiddles",
               "pass_tile_lds_bytes", "pass_ntl_candidate", "pass_first_only", "col_stride", "map_window", "fft_pass_route", "fft_plan",
               "fft_buffer_order", "fft_op_args"):
        defined = r"^[\w<>:\s&\*]*\b%s(_rt)?\s*\([^;{]*\)\s*(\{|$)" % fn
        assert re.search(defined, strip(core), re.M), fn
        for name, text in (("fft_impl.h", impl), ("capi.cpp", capi), ("bdsp_internal.h", internal)):
            for m in re.finditer(defined, strip(text), re.M):
                # (a call that opens a block, `if (io_is_generic(io)) {`, is no definition)
                assert re.match(r"\s*(if|while|return|else|for)\b", m.group(0)) or "=" in m.group(0), (fn, name, m.group(0))
    # ... and so are the expressions of launch_pass: the route's fields come from the struct
    body = strip(impl)
    assert "struct FftIo" not in body + strip(internal) and "struct FftIo" in core
    assert not re.search(r"\bsimple\s*=\s*!gen", body) and re.search(r"\bsimple = r\.simple;", body)
    assert re.search(r"\bgen = r\.gen;", body) and re.search(r"\bntl = r\.ntl;", body) and re.search(r"\bwin_fixed = r\.win_fixed;", body)
    assert "FFT_WINDOW_OUT_DIV" not in re.search(r"static int launch_pass\(.*?\n}\n", body, re.S).group(0).split("BDSP_PASS_K")[0].replace("io.flags & FFT_WINDOW_OUT_DIV", "")
    assert len(re.findall(r"\bfft_plan\(", body)) == 1 and "num_cus()" in re.search(r"fft_plan\([^;]*;", body).group(0)
    assert "num_cus()" not in body.split("int fft_pow2(")[0].split("static int launch_pass(")[1]
    # capi.cpp orders its buffers and maps the facade's operations through the header
    assert len(re.findall(r"\bfft_buffer_order\(", strip(capi))) == 1 and len(re.findall(r"\bfft_op_args<T>\(", strip(capi))) == 1
    assert "size_t(1) << 19" not in strip(capi).split("int fft_two_buffers(")[1].split("\n}\n")[0]
    # the simulation calls the rule, not a copy of it
    for fn in ("fft_plan", "fft_op_args", "map_window", "fft_buffer_order", "plan_passes", "pass_tile_built", "pass_first_only_rt",
               "pass_split_exchange", "col_stride", "plan_pass_count"):
        assert re.search(r"\b%s(<[\w, ]+>)?\(" % fn, sim), fn
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "fft_plan_core.h" in re.search(r"^HDRS = (.*)$", f.read(), re.M).group(1)


def test_route_table_index_maps_and_numbers_on_the_host(tmp_path):
    """tests/host_sim/sim_fft_passes.cpp, a stand-alone program, built with the host compiler once plainly and once with
    -fsanitize=address,undefined.  The 434 lines of the table against the rule at 256 CUs; a sweep of the rule over both
    precisions x 2^13 .. 2^30 points x batch 1, 3, 8, 64, 4096 x every option combination of the facade, of
    bdsp_hip_dev_fft and of the library's own callers x 256, 8, 304 CUs (149 580 plans): 142 route classes (one per
    k_fft_pass instantiation that can be launched, plus k_fft_wg4 both ways), every one of them reached by the sweep at
    or below 2^23 points and by a line of the table; launch parameters of every route.  One pass of every (tile, lane
    map) pair against the Stockham iteration in long double, with the XCD tile remap, both shift renamings and the f64
    split exchange: every point loaded once and stored once, a last-pass workgroup reads what it writes.  Numbers, the
    plain variants, forward and inverse, against a long double transform (bound: north_star's 1e-6 / 1e-12 per
    transform): worst rel-L2 f32 3.556e-07 (64 x 64 x 64 points; 2.8e-07 at 2^16), f64 6.431e-16."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_fft_passes.cpp")
    for flags, name in (([], "sim_fft_passes"), (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"], "sim_fft_passes_san")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + flags + ["-o", exe, src])
        r = subprocess.run([exe, SHAPES], capture_output=True, text=True)
        print(r.stdout[-3000:])
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        m = re.search(r"^table: (\d+) lines, (\d+) route classes witnessed$", r.stdout, re.M)
        assert m and int(m.group(1)) == len(read_lines()) == 434 and int(m.group(2)) == 142
        m = re.search(r"^sweep: (\d+) plans, (\d+) route classes, (\d+) without a witness at or below 2\^23 points, (\d+) without a line$", r.stdout, re.M)
        assert m and int(m.group(1)) == 149580 and int(m.group(2)) == 142 and int(m.group(3)) == 0 and int(m.group(4)) == 0
        assert "reachable above 2^23 points only" not in r.stdout
        m = re.search(r"^tiles: 23 \(tile, lane map\) pairs, worst rel-L2 of one pass: f32 (\d\.\d+e-\d+) \(bound 1e-06\), f64 (\d\.\d+e-\d+) \(bound 1e-12\)$", r.stdout, re.M)
        assert m and 0 < float(m.group(1)) <= 1e-6 and 0 < float(m.group(2)) <= 1e-12
        assert re.search(r"^window lattice: 8 tiles$", r.stdout, re.M)
        assert len(re.findall(r"^numbers: (2\^13|2\^14|2\^16|64 x 64 x 64) points: ", r.stdout, re.M)) == 4
        m = re.search(r"^numbers: worst rel-L2 per transform: f32 (\d\.\d+e-\d+) \(bound 1e-06\), f64 (\d\.\d+e-\d+) \(bound 1e-12\)$", r.stdout, re.M)
        assert m and 0 < float(m.group(1)) <= 1e-6 and 0 < float(m.group(2)) <= 1e-12, r.stdout[-3000:]
        assert re.search(r"^0 failures$", r.stdout, re.M)
