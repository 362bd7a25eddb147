"""sort, top_k(8) and median (sort.hip) on one MI355X beside a plain device copy of the same bytes, torch's sort / topk / median
on the same device and the download - numpy - upload round trip they replace -> profiles/sort.txt.

  (a) 16384 x 2048 f32    (b) 65536 x 100 f32    (c) 64 x 2^20 f32    (d) 16384 x 2048 f64

  python tools/sort_bench.py --out profiles/sort.txt

ours / copy / torch: device events around one call (ours: the library's events on its stream; top_k and median include the
call's synchronisation and its copy of the results to the host); every leg is warmed, then calls are added up to MIN_TIME
seconds (at most MAX_CALLS); the legs alternate copy, ours, torch, copy, ours, torch, copy and the smallest mean of each kind
is shown, with the spread of the copy legs.  copy is torch's device-to-device copy of the same bytes: the floor of any
out-of-place row operation.  torch: torch.sort(dim=1), torch.topk(8, dim=1), torch.median(dim=1), results left on the
device.  round trip: download of the whole matrix, np.sort(axis=1) on the host, wall clock, once, and for sort the upload of
the result.  The network is data-independent, so sorting the already sorted matrix again takes the same time.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("a", 16384, 2048, "float32"), ("b", 65536, 100, "float32"), ("c", 64, 1 << 20, "float32"), ("d", 16384, 2048, "float64"))
MIN_TIME = 0.2
MAX_CALLS = 2000
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
    lib = bd.lib
    timed = device_timer(bd)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# sort, top_k(8), median (sort.hip) on one MI355X: tools/sort_bench.py.  Device events around one call; every leg warmed, calls")
    w("# adding up to >= %.1f s (at most %d); legs alternate copy, ours, torch.  Shown: the smallest mean of a kind of leg; spread of" % (MIN_TIME, MAX_CALLS))
    w("# the copy legs.  copy: a device copy of the same bytes (torch).  torch: torch.sort / torch.topk / torch.median along dim 1,")
    w("# results left on the device.  round trip: download, np.sort on the host (wall clock, once), and for sort the upload.")
    w("# ** ours slower than that comparison **")
    w("%-5s %-4s %-15s %-8s %9s %11s %10s %7s %12s %11s %13s %14s %17s" % (
        "case", "kind", "shape", "op", "launches", "ours us", "copy us", "spread", "ours / copy", "torch us", "ours / torch", "round trip us",
        "ours / round trip"))
    rng = np.random.default_rng(20241021)
    for name, rows, n, dtype in CASES:
        if only and name not in only:
            continue
        x = rng.standard_normal((rows, n)).astype(dtype)
        m = bd.DspMat(x)
        src = torch.from_numpy(x).cuda()
        dst = torch.empty_like(src)
        passes = max(0, (-(-n // 4096) - 1).bit_length())

        def torch_leg(fn):
            def call():
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                return t0.elapsed_time(t1) * 1e-3
            return call

        def first(result):
            return result[0]

        copy = torch_leg(lambda: dst.copy_(src))
        t = time.perf_counter()
        h = m.data()
        t_down = time.perf_counter() - t
        t = time.perf_counter()
        hs = np.sort(h, axis=1)
        t_sort = time.perf_counter() - t
        t = time.perf_counter()
        up = bd.DspMat(hs)
        ok(lib.bdsp_hip_synchronize(None))
        t_up = time.perf_counter() - t
        # the device results against the host's
        code, top = bd.top_k(m, 8)
        ok(code)
        assert np.array_equal(top["value"], hs[:, ::-1][:, :8])
        code, med = bd.median(m)
        ok(code)
        assert np.array_equal(med, np.quantile(hs.astype(np.float64), 0.5, axis=1)) or np.allclose(med, np.median(hs.astype(np.float64), axis=1), rtol=1e-12)
        ok(bd.sort(m))
        assert np.array_equal(m.data(), hs)
        del up, h, hs
        ops = (("sort", 1 + passes, lambda: bd.sort(m), lambda: torch.sort(src, dim=1), t_down + t_sort + t_up),
               ("top_k(8)", 2 + passes, lambda: first(bd.top_k(m, 8)), lambda: torch.topk(src, 8, dim=1), t_down + t_sort),
               ("median", 2 + passes, lambda: first(bd.median(m)), lambda: torch.median(src, dim=1), t_down + t_sort))
        for op, launches, ours_fn, torch_fn, trip in ops:
            ours = lambda: timed(ours_fn)  # noqa: E731
            other = torch_leg(torch_fn)
            tc, to, tt = [leg(copy)], [], []
            for _ in range(2):
                to.append(leg(ours))
                tt.append(leg(other))
                tc.append(leg(copy))
            tm, tcp, tto = min(to), min(tc), min(tt)
            spread = (max(tc) - min(tc)) / min(tc)

            def against(other_time, digits):
                r = "%.*f" % (digits, tm / other_time)
                return "**%s**" % r if tm > other_time else r

            rc = "%.2f" % (tm / tcp)
            if tm > tcp * (1.0 + spread):
                rc = "**%s**" % rc
            w("%-5s %-4s %-15s %-8s %9d %11.1f %10.1f %6.1f%% %12s %11.1f %13s %14.0f %17s" % (
                "(%s)" % name, "r32" if dtype == "float32" else "r64", "%d x %d" % (rows, n), op, launches, tm * 1e6, tcp * 1e6, spread * 100, rc,
                tto * 1e6, against(tto, 2), trip * 1e6, against(trip, 4)))
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
