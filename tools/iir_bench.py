"""sosfilt (iir.hip) on one MI355X beside a plain device copy of the same bytes, scipy.signal.sosfilt on the host and the
download - host - upload round trip it replaces -> profiles/iir.txt.

  four sections (the lowpass family of tests/iir_shapes.txt) on
  (a) 1 x 2^24 complex f32   (b) 64 x 48 000 real f32   (c) 16 384 x 1000 complex f32   (d) 64 x 2^20 complex f64

  python tools/iir_bench.py --out profiles/iir.txt

Timing as in tools/mat_eigh_bench.py: device events around ONE call -- the library's on its own stream, torch's copy on
torch's; the call computes and uploads its coefficient tables, all of which is inside the window.  Every leg is warmed and
then repeated until the timed calls add up to at least 0.2 s (at most 2000 calls); a figure is the mean of a leg.  The legs
alternate copy, ours, copy, ours, copy; the copy legs give the spread (largest - smallest) / smallest, and the smallest
mean of each kind is shown.  The filter runs in place on its own output, call after call: the lowpass is stable, so the
data decay and stay finite.  scipy: scipy.signal.sosfilt on the downloaded array, wall clock, once; "not available" where
scipy does not import.  round trip: download, scipy (or nothing where it does not import), upload, wall clock, once.
ours / copy is at least 1 for the one-launch form (one read, one write) and at least 1.5 for the three-launch form (two
reads, one write).  No figure is a gate.  A figure of ours that is slower than its comparison is marked in bold (**...**).

Below the times: the worst accuracy ratio e_dev / max(e_ser, eps max|truth|) over every line of tests/iir_shapes.txt with
the models of tests/test_gpu_iir.py on this device, and from the host simulation tests/host_sim/sim_iir.cpp where a host
compiler is found."""
import argparse
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = (("a", 1, 1 << 24, "float32", True), ("b", 64, 48000, "float32", False), ("c", 16384, 1000, "float32", True),
         ("d", 64, 1 << 20, "float64", True))
MIN_TIME = 0.2
MAX_CALLS = 2000
WARM = 2
SECTIONS = 4


def ok(code):
    assert code == 0, code


def leg(timed_call):
    for _ in range(WARM):
        timed_call()
    total, count = 0.0, 0
    while total < MIN_TIME and count < MAX_CALLS:
        total += timed_call()
        count += 1
    return total / count


def run(out, only, ratios):
    import numpy as np
    import torch
    import basic_dsp_amd as bd
    import test_gpu_iir as T
    try:
        from scipy.signal import sosfilt as scipy_sosfilt
    except ImportError:
        scipy_sosfilt = None
    bd.require_gpu()
    lib = bd.lib
    e0, e1 = C.c_void_p(lib.bdsp_hip_event_create()), C.c_void_p(lib.bdsp_hip_event_create())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = C.c_float()
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# sosfilt (iir.hip) on one MI355X, %d sections: tools/iir_bench.py.  Device events around one call; every leg warmed, calls" % SECTIONS)
    w("# adding up to >= %.1f s (at most %d); legs alternate copy, ours, copy, ours, copy.  Shown: the smallest mean of a kind of" % (MIN_TIME, MAX_CALLS))
    w("# leg; spread of the copy legs.  copy: a device copy of the same bytes (torch).  scipy: scipy.signal.sosfilt on the host,")
    w("# wall clock.  round trip: download, scipy, upload (wall clock).  ** ours slower than that comparison **")
    w("%-5s %-4s %-14s %9s %10s %10s %7s %12s %12s %13s %13s %16s" % ("case", "kind", "shape", "launches", "ours us", "copy us", "spread",
                                                                  "ours / copy", "scipy us", "ours / scipy", "round trip us", "ours / round trip"))
    sos = T.make_sos("lowpass", SECTIONS)
    rng = np.random.default_rng(20241020)
    for name, rows, n, dtype, cplx in CASES:
        if only and name not in only:
            continue
        Cn = 2 if cplx else 1
        x = rng.uniform(-1, 1, (rows, n * Cn)).astype(dtype)
        m = bd.DspMat(x, is_complex=cplx)
        src = torch.from_numpy(x).cuda()
        dst = torch.empty_like(src)

        def ours():
            ok(lib.bdsp_hip_event_record(e0, None))
            code = bd.sosfilt(m, sos)
            ok(lib.bdsp_hip_event_record(e1, None))
            ok(code)
            ok(lib.bdsp_hip_synchronize(None))
            ok(lib.bdsp_hip_event_elapsed_ms(e0, e1, C.byref(ms)))
            return ms.value * 1e-3

        def copy():
            t0.record()
            dst.copy_(src)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e-3

        tc, to = [leg(copy)], []
        to.append(leg(ours))
        tc.append(leg(copy))
        to.append(leg(ours))
        tc.append(leg(copy))
        tm, tcp = min(to), min(tc)
        spread = (max(tc) - min(tc)) / min(tc)
        del src, dst
        torch.cuda.empty_cache()
        ok(m._fn("upload")(m._h, x.ctypes.data_as(C.c_void_p), x.size))  # the fresh input again for the host legs
        t = time.perf_counter()
        h = m.data()
        t_down = time.perf_counter() - t
        if scipy_sosfilt is not None:
            hv = h.view(np.complex64 if dtype == "float32" else np.complex128) if cplx else h
            t = time.perf_counter()
            y = scipy_sosfilt(sos, hv, axis=-1)
            t_host = time.perf_counter() - t
            y = np.ascontiguousarray(y.astype(hv.dtype)).view(dtype)
        else:
            t_host, y = None, h
        t = time.perf_counter()
        up = bd.DspMat(y, is_complex=cplx)
        ok(lib.bdsp_hip_synchronize(None))
        t_up = time.perf_counter() - t
        del up
        trip = t_down + (t_host or 0.0) + t_up

        def against(other):
            r = "%.2f" % (tm / other)
            return "**%s**" % r if tm > other else r

        rc = "%.2f" % (tm / tcp)
        if tm > tcp * (1.0 + spread):
            rc = "**%s**" % rc
        w("%-5s %-4s %-14s %9d %10.1f %10.1f %6.1f%% %12s %12s %13s %13.1f %16s" % (
            "(%s)" % name, ("c" if cplx else "r") + ("32" if dtype == "float32" else "64"), "%d x %d" % (rows, n), 1 if n <= T.TILE else 3,
            tm * 1e6, tcp * 1e6, spread * 100, rc, "%.1f" % (t_host * 1e6) if t_host is not None else "not available",
            against(t_host) if t_host is not None else "-", trip * 1e6, against(trip)))
        del m
    lib.bdsp_hip_event_destroy(e0)
    lib.bdsp_hip_event_destroy(e1)
    if not ratios:
        return
    worst = {"float32": 0.0, "float64": 0.0}
    worst_state = {"float32": 0.0, "float64": 0.0}
    for line, (kind, prec, rows, n, S, family) in enumerate(T.SHAPES):
        dtype, cplx = T.kind_of(kind, prec)
        Cn = 2 if cplx else 1
        key = np.dtype(dtype).name
        s = T.make_sos(family, S)
        x = T.draw(1000 + line, rows, n, dtype, cplx)
        s0 = 0.5 * T.draw(5000 + line, rows, 2 * S, dtype, cplx)
        for state in (None, s0):
            ty, sy, ts, ss = T.models(s, x, state, dtype, cplx)
            m = bd.DspMat(x, is_complex=cplx)
            st = bd.DspMat(state, is_complex=cplx) if state is not None else None
            ok(bd.sosfilt(m, s, st))
            worst[key] = max(worst[key], T.yardstick(T.signals(m.data(), cplx), ty, sy, np.finfo(dtype).eps))
            if st is not None and n:
                worst_state[key] = max(worst_state[key], T.yardstick(T.signals(st.data(), cplx), ts, ss, np.finfo(dtype).eps))
    w("# accuracy over the %d lines of tests/iir_shapes.txt, each with and without an incoming state: the worst" % len(T.SHAPES))
    w("# e_dev / max(e_ser, eps max|truth|), eps = numpy.finfo(T).eps, outputs and final states")
    w("device    outputs f32 %.3f f64 %.3f   final states f32 %.3f f64 %.3f" % (worst["float32"], worst["float64"], worst_state["float32"],
                                                                              worst_state["float64"]))
    if shutil.which("g++"):
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "sim_iir")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host_sim", "sim_iir.cpp")])
            text = subprocess.run([exe, os.path.join(ROOT, "tests", "iir_shapes.txt")], capture_output=True, text=True, check=True).stdout
        a = re.search(r"^worst e_dev / max\(e_ser, eps max\|truth\|\): f32 (\S+), f64 (\S+)$", text, re.M)
        b = re.search(r"^worst final-state ratio: f32 (\S+), f64 (\S+)$", text, re.M)
        w("host sim  outputs f32 %s f64 %s   final states f32 %s f64 %s" % (a.group(1), a.group(2), b.group(1), b.group(2)))
    else:
        w("host sim  not available (no host compiler)")
    w("# R of tests/test_gpu_iir.py: twice the largest figure above, rounded up to a power of two")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", default="", help="case letters, e.g. ad")
    ap.add_argument("--no-ratios", action="store_true", help="times only")
    a = ap.parse_args()
    lines = []
    run(lines, a.only, not a.no_ratios)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
