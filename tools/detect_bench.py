"""detect (detect.hip) on one MI355X beside a plain device copy of the same bytes, torch.nonzero on the same device and the
download + np.nonzero round trip it replaces -> profiles/detect.txt.

  boundary "wrap", order 0, 1, 8 and 1024, a scalar threshold and a matrix threshold (one value per cell) that let about
  1e-4 and 1e-1 of the cells through, on
  (a) 16384 x 2048 f32    (b) 64 x 2^20 f32    (c) 16384 x 2048 f64

  python tools/detect_bench.py --out profiles/detect.txt

ours: device events around one call of detect with capacity = the number of detections (one call of the C entry: four
launches, the counts and the complete lists copied to the host; the call synchronises twice, so the events span its host
gaps too).  count: the same with capacity = 0 (three launches, the counts only).  Every leg is warmed, then calls are added
up to MIN_TIME seconds (at most MAX_CALLS); the legs alternate copy, ours, copy, ours, copy and the smallest mean of each
kind is shown, with the spread of the copy legs.  copy: torch's device-to-device copy of the bytes of x, the floor of one
read and one write of the data (detect reads x twice and writes a short list).  torch: torch.nonzero of the same predicate
on the same device, result left on the device -- x > t for order 0, the three-way compare (x > t) & (x > roll(x, 1)) &
(x > roll(x, -1)) for order 1, nothing for the longer orders.  round trip: download of the matrix (wall clock, once per
shape) plus np.nonzero(x > t) on the host; for order > 0 the host would need more, so it is a lower bound there.
Where torch gives the same predicate (order 0 and 1) the lists are compared with it, entry by entry.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("a", 16384, 2048, "float32"), ("b", 64, 1 << 20, "float32"), ("c", 16384, 2048, "float64"))
ORDERS = (0, 1, 8, 1024)
# the standard normal quantiles that let 1e-4 and 1e-1 of the cells through (rounded to float32 before use)
LEVELS = ((1e-4, 3.719016485455709), (1e-1, 1.2815515655446004))
MIN_TIME = 0.1
MAX_CALLS = 1000
WARM = 2


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


def run(out, only):
    import numpy as np
    import torch
    import basic_dsp_amd as bd
    bd.require_gpu()
    timed = device_timer(bd)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# detect (detect.hip), boundary wrap, on one MI355X: tools/detect_bench.py.  Device events around one call; every leg warmed,")
    w("# calls adding up to >= %.1f s (at most %d); legs alternate copy, ours, copy, ours, copy.  Shown: the smallest mean of a kind" % (MIN_TIME, MAX_CALLS))
    w("# of leg; spread of the copy legs.  ours: capacity = the number of detections (four launches, counts and complete lists on")
    w("# the host).  count: capacity 0 (three launches, counts only).  copy: a device copy of the bytes of x (torch).  torch:")
    w("# torch.nonzero of the same predicate on the device (order 0: x > t; order 1: the three-way compare; longer orders: none).")
    w("# round trip: download of x plus np.nonzero(x > t) on the host, wall clock (a lower bound for order > 0).  thr: s one")
    w("# scalar, m one value per cell (a second matrix read).  pass: the share of cells above the threshold; det / cell: the")
    w("# detections per cell.  ** ours slower than that comparison **")
    w("%-5s %-4s %-15s %5s %3s %6s %10s %11s %11s %10s %7s %12s %10s %13s %14s %17s %s" % (
        "case", "kind", "shape", "order", "thr", "pass", "det / cell", "ours us", "count us", "copy us", "spread", "ours / copy", "torch us",
        "ours / torch", "round trip us", "ours / round trip", "checked"))
    rng = np.random.default_rng(20241021)
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
        del h
        for share, level in LEVELS:
            level = float(np.float32(level))  # a float32 value: double(x) > t, torch's x > float32(t) and the f64 compare are one predicate
            t = time.perf_counter()
            host = np.nonzero(x > level)
            t_host = time.perf_counter() - t
            floor_t = torch.full_like(src, level)
            floor = bd.DspMat(np.full((rows, n), level, dtype))
            for order in ORDERS:
                for thr in ("s", "m"):
                    arg = level if thr == "s" else floor
                    code, det = bd.detect(m, arg, order, "wrap")
                    ok(code)
                    total = int(det["count"].sum())
                    ours = lambda: timed(lambda: bd.detect(m, arg, order, "wrap", capacity=total)[0])  # noqa: E731
                    count = lambda: timed(lambda: bd.detect(m, arg, order, "wrap", capacity=0)[0])  # noqa: E731
                    tc, to = [leg(copy)], []
                    to.append(leg(ours))
                    tc.append(leg(copy))
                    to.append(leg(ours))
                    tc.append(leg(copy))
                    tm, tcp, tcount = min(to), min(tc), leg(count)
                    spread = (max(tc) - min(tc)) / min(tc)
                    bound = level if thr == "s" else floor_t
                    if order == 0:
                        pred = lambda: torch.nonzero(src > bound)  # noqa: E731
                    elif order == 1:
                        pred = lambda: torch.nonzero((src > bound) & (src > torch.roll(src, 1, 1)) & (src > torch.roll(src, -1, 1)))  # noqa: E731
                    else:
                        pred = None
                    checked = "-"
                    if pred is not None:
                        def torch_leg():
                            t0.record()
                            pred()
                            t1.record()
                            torch.cuda.synchronize()
                            return t0.elapsed_time(t1) * 1e-3
                        t_torch = leg(torch_leg)
                        want = pred().cpu().numpy()
                        assert len(want) == total, (name, order, thr, len(want), total)
                        assert np.array_equal(want[:, 0], det["row"]) and np.array_equal(want[:, 1], det["index"]), (name, order, thr)
                        assert np.array_equal(det["value"], x[det["row"], det["index"]])
                        checked = "= torch"
                        del want
                    else:
                        t_torch = None
                    if order == 0:
                        assert np.array_equal(host[0], det["row"]) and np.array_equal(host[1], det["index"])
                    trip = t_down + t_host

                    def against(other):
                        r = "%.4f" % (tm / other)
                        return "**%s**" % r if tm > other else r

                    rc = "%.2f" % (tm / tcp)
                    if tm > tcp * (1.0 + spread):
                        rc = "**%s**" % rc
                    w("%-5s %-4s %-15s %5d %3s %6.0e %10.2e %11.1f %11.1f %10.1f %6.1f%% %12s %10s %13s %14.0f %17s %s" % (
                        "(%s)" % name, "r32" if dtype == "float32" else "r64", "%d x %d" % (rows, n), order, thr, share, total / float(rows * n), tm * 1e6,
                        tcount * 1e6, tcp * 1e6, spread * 100, rc, "%.1f" % (t_torch * 1e6) if t_torch is not None else "-",
                        against(t_torch) if t_torch is not None else "-", trip * 1e6, against(trip), checked))
                    del det
            del floor, floor_t, host
        del m, src, dst
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    out = []
    try:
        run(out, set(a.only.split(",")) - {""})
    finally:
        if a.out and out:
            with open(a.out, "w") as f:
                f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
