"""rank_filter / medfilt (rank_filter.hip) on one MI355X beside a plain device copy of the same bytes, the numpy model on the
host and the download - host - upload round trip it replaces -> profiles/rank_filter.txt.

  median filters of 3, 9, 33, 129 and 1025 points, boundary "zero", on
  (a) 16384 x 2048 f32    (b) 64 x 2^20 f32    (c) 16384 x 2048 f64

  python tools/rank_filter_bench.py --build-variants basic_dsp_amd/csrc/build/rank_variants      (no GPU needed; needs the built tree)
  python tools/rank_filter_bench.py --variants basic_dsp_amd/csrc/build/rank_variants --out profiles/rank_filter.txt

ours / copy: device events around one call; every leg is warmed, then calls are added up to MIN_TIME seconds (at most
MAX_CALLS); the legs alternate copy, ours, copy, ours, copy and the smallest mean of each kind is shown, with the spread of
the copy legs.  copy is torch's device-to-device copy of the same bytes: the floor of any out-of-place row operation.
host: np.partition over sliding_window_view of the zero-padded rows, wall clock, once; where the full problem has more
than HOST_ELEMENTS window elements it is measured on a slice (some rows, and of long rows a segment) and scaled by the
number of outputs, and the line says so.  scipy: scipy.signal.medfilt on the same slice, likewise; "not available" where
scipy does not import.  round trip: download and upload of the whole matrix (wall clock) plus the host time.

The sweep places the crossover constants RANK_CROSS_F32 / RANK_CROSS_F64 of rank_filter_core.h.  The library has no
switch that forces a selector, so --build-variants compiles rank_filter.hip twice from a copy of the two source files
whose crossover constants are rewritten (count at every W, bisect at every W) and links each with the other objects of
the built tree; the sweep runs each variant in a child process that loads it through BDSP_HIP_LIBRARY.  Both selectors
are data-independent, so the time is a function of (shape, W, precision) alone.
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")
sys.path.insert(0, ROOT)

CASES = (("a", 16384, 2048, "float32"), ("b", 64, 1 << 20, "float32"), ("c", 16384, 2048, "float64"))
WINDOWS = (3, 9, 33, 129, 1025)
SWEEP_SHAPE = (4096, 2048)
SWEEP = {"float32": (5, 9, 13, 17, 21, 25, 29, 33, 41, 49, 65, 97, 129), "float64": (9, 17, 25, 33, 41, 49, 57, 65, 81, 97, 129, 193, 257)}
MIN_TIME = 0.2
MAX_CALLS = 2000
WARM = 2
HOST_ELEMENTS = 1 << 26


def ok(code):
    assert code == 0, code


def leg(timed_call, min_time=MIN_TIME):
    for _ in range(WARM):
        timed_call()
    total, count = 0.0, 0
    while total < min_time and count < MAX_CALLS:
        total += timed_call()
        count += 1
    return total / count


def build_variants(where):
    """two libraries that differ from the built one in rank_filter.o alone: count at every W, bisect at every W"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).replace("$(BUILD)", os.path.join(CSRC, "build")).split()
    missing = [o for o in objs if not os.path.exists(o)]
    assert not missing, "build the library first (make -C basic_dsp_amd/csrc): %s" % missing[:3]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for name, cross in (("count", 1 << 30), ("bisect", 0)):
        d = os.path.join(where, name)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(CSRC, "rank_filter_core.h")) as f:
            core, n = re.subn(r"^(constexpr int RANK_CROSS_F(?:32|64)) = \d+;", r"\1 = %d;" % cross, f.read(), flags=re.M)
        assert n == 2
        with open(os.path.join(d, "rank_filter_core.h"), "w") as f:
            f.write(core)
        shutil.copy(os.path.join(CSRC, "rank_filter.hip"), d)
        obj = os.path.join(d, "rank_filter.o")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-unused-result",
                               "-I", d, "-I", CSRC, "-c", os.path.join(d, "rank_filter.hip"), "-o", obj])
        rest = [o for o in objs if not o.endswith("/rank_filter.o")]
        out = os.path.join(d, "libbasic_dsp_hip_%s.so" % name)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, "build", "exports.map"),
                               "-o", out, obj] + rest)
        print("built", out)


def device_timer(bd):
    lib = bd.lib
    e0, e1 = C.c_void_p(lib.bdsp_hip_event_create()), C.c_void_p(lib.bdsp_hip_event_create())
    ms = C.c_float()

    def timed(call):
        ok(lib.bdsp_hip_event_record(e0, None))
        code = call()
        ok(lib.bdsp_hip_event_record(e1, None))
        ok(code)
        ok(lib.bdsp_hip_synchronize(None))
        ok(lib.bdsp_hip_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value * 1e-3
    return timed


def sweep_child(dtype):
    """the loaded library (BDSP_HIP_LIBRARY names a variant): one JSON line {W: seconds} for the sweep shape"""
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    timed = device_timer(bd)
    rows, n = SWEEP_SHAPE
    x = np.random.default_rng(7).standard_normal((rows, n)).astype(dtype)
    m = bd.DspMat(x)
    res = {}
    for w in SWEEP[dtype]:
        res[w] = leg(lambda: timed(lambda: bd.medfilt(m, w)), 0.1)
    print("SWEEP " + json.dumps({"library": os.path.basename(bd.LIB_PATH), "dtype": dtype, "seconds": res}), flush=True)


def host_slice(rows, n, w):
    """(rows, points) of the slice the host legs run on: at most HOST_ELEMENTS window elements"""
    if rows * n * w <= HOST_ELEMENTS:
        return rows, n
    pts = min(n, max(4 * w, HOST_ELEMENTS // w))
    return max(1, min(rows, HOST_ELEMENTS // (pts * w))), pts


def run(out, only, variants):
    import numpy as np
    import torch
    from numpy.lib.stride_tricks import sliding_window_view
    import basic_dsp_amd as bd
    try:
        from scipy.signal import medfilt as scipy_medfilt
    except ImportError:
        scipy_medfilt = None
    bd.require_gpu()
    lib = bd.lib
    timed = device_timer(bd)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# medfilt (rank_filter.hip), boundary zero, on one MI355X: tools/rank_filter_bench.py.  Device events around one call; every")
    w("# leg warmed, calls adding up to >= %.1f s (at most %d); legs alternate copy, ours, copy, ours, copy.  Shown: the smallest" % (MIN_TIME, MAX_CALLS))
    w("# mean of a kind of leg; spread of the copy legs.  copy: a device copy of the same bytes (torch).  numpy: np.partition over")
    w("# sliding_window_view on the host, wall clock; scipy: scipy.signal.medfilt; both on the slice shown where the whole problem")
    w("# has more than 2^26 window elements, scaled by the number of outputs.  round trip: download, numpy, upload.")
    w("# ** ours slower than that comparison **")
    w("%-5s %-4s %-15s %5s %-7s %11s %10s %7s %12s %-15s %12s %13s %12s %14s %14s %17s" % (
        "case", "kind", "shape", "W", "select", "ours us", "copy us", "spread", "ours / copy", "host slice", "numpy us", "ours / numpy", "scipy us",
        "ours / scipy", "round trip us", "ours / round trip"))
    rng = np.random.default_rng(20241021)
    with open(os.path.join(CSRC, "rank_filter_core.h")) as f:
        k = {a: int(b) for a, b in re.findall(r"^constexpr int (RANK_\w+) = (\d+);", f.read(), re.M)}
    for name, rows, n, dtype in CASES:
        if only and name not in only:
            continue
        x = rng.standard_normal((rows, n)).astype(dtype)
        m = bd.DspMat(x)
        src = torch.from_numpy(x).cuda()
        dst = torch.empty_like(src)

        def copy():
            t0.record()
            dst.copy_(src)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e-3

        t = time.perf_counter()
        h = m.data()
        t_down = time.perf_counter() - t
        t = time.perf_counter()
        up = bd.DspMat(h)
        ok(lib.bdsp_hip_synchronize(None))
        t_up = time.perf_counter() - t
        del up, h
        for win in WINDOWS:
            ours = lambda: timed(lambda: bd.medfilt(m, win))  # noqa: E731
            tc, to = [leg(copy)], []
            to.append(leg(ours))
            tc.append(leg(copy))
            to.append(leg(ours))
            tc.append(leg(copy))
            tm, tcp = min(to), min(tc)
            spread = (max(tc) - min(tc)) / min(tc)
            hr, hp = host_slice(rows, n, win)
            scale = (rows * n) / float(hr * hp)
            part = np.ascontiguousarray(x[:hr, :hp])
            t = time.perf_counter()
            padded = np.zeros((hr, hp + win - 1), part.dtype)
            padded[:, win // 2:win // 2 + hp] = part
            y = np.partition(sliding_window_view(padded, win, axis=1), win // 2, axis=2)[:, :, win // 2]
            t_numpy = (time.perf_counter() - t) * scale
            if scipy_medfilt is not None:
                t = time.perf_counter()
                ys = scipy_medfilt(part, (1, win))
                t_scipy = (time.perf_counter() - t) * scale
                assert np.array_equal(ys, y)
            else:
                t_scipy = None
            if (hr, hp) == (rows, n):  # the device result against the host's, where the host ran the whole problem
                ok(m._fn("upload")(m._h, x.ctypes.data_as(C.c_void_p), x.size))
                ok(bd.medfilt(m, win))
                assert np.array_equal(m.data(), y)
            trip = t_down + t_numpy + t_up

            def against(other):
                r = "%.4f" % (tm / other)
                return "**%s**" % r if tm > other else r

            rc = "%.2f" % (tm / tcp)
            if tm > tcp * (1.0 + spread):
                rc = "**%s**" % rc
            count = win <= (k["RANK_CROSS_F32"] if dtype == "float32" else k["RANK_CROSS_F64"])
            w("%-5s %-4s %-15s %5d %-7s %11.1f %10.1f %6.1f%% %12s %-15s %12.0f %13s %12s %14s %14.0f %17s" % (
                "(%s)" % name, "r32" if dtype == "float32" else "r64", "%d x %d" % (rows, n), win, "count" if count else "bisect", tm * 1e6, tcp * 1e6,
                spread * 100, rc, "%d x %d" % (hr, hp), t_numpy * 1e6, against(t_numpy), "%.0f" % (t_scipy * 1e6) if t_scipy is not None else "not available",
                against(t_scipy) if t_scipy is not None else "-", trip * 1e6, against(trip)))
        del m, src, dst
        torch.cuda.empty_cache()
    if not variants:
        w("# no sweep: no --variants directory given")
        return
    w("#")
    w("# crossover sweep: medfilt of W points on %d x %d, us per call with the count selector at every W and with the bisect selector" % SWEEP_SHAPE)
    w("# at every W (two builds that differ in the crossover constants alone, each in its own process)")
    w("%-4s %5s %12s %12s %15s" % ("kind", "W", "count us", "bisect us", "count / bisect"))
    for dtype in ("float32", "float64"):
        res = {}
        for name in ("count", "bisect"):
            path = os.path.join(variants, name, "libbasic_dsp_hip_%s.so" % name)
            assert os.path.exists(path), path
            env = dict(os.environ, BDSP_HIP_LIBRARY=os.path.abspath(path))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweep-child", dtype], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
            line = [l for l in r.stdout.splitlines() if l.startswith("SWEEP ")][-1]
            got = json.loads(line[len("SWEEP "):])
            assert got["library"] == os.path.basename(path), got["library"]
            res[name] = {int(a): b for a, b in got["seconds"].items()}
        for win in SWEEP[dtype]:
            c, b = res["count"][win], res["bisect"][win]
            w("%-4s %5d %12.1f %12.1f %15.2f" % ("r32" if dtype == "float32" else "r64", win, c * 1e6, b * 1e6, c / b))
        last = [win for win in SWEEP[dtype] if res["count"][win] <= res["bisect"][win]]
        w("# %s: count is at least as fast as bisect up to W = %s of the W measured" % (dtype, max(last) if last else "none"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="")
    ap.add_argument("--variants", default=None, help="the directory --build-variants wrote")
    ap.add_argument("--build-variants", default=None, metavar="DIR")
    ap.add_argument("--sweep-child", default=None, metavar="DTYPE")
    a = ap.parse_args()
    if a.build_variants:
        return build_variants(a.build_variants)
    if a.sweep_child:
        return sweep_child(a.sweep_child)
    out = []
    try:
        run(out, set(a.only.split(",")) - {""}, a.variants)
    finally:
        if a.out and out:
            with open(a.out, "w") as f:
                f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
