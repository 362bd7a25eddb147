"""DspMat.transpose (mat_transpose.hip) on one MI355X against two yardsticks that are not the code under test, for the
four element kinds (f32, c32, f64, c64: 4, 8, 8 and 16 bytes) and the shapes
  16384 x 2048, 2048 x 16384, 16384 x 1000, 65536 x 100     the four large shapes the goal is about
  70000 x 3, 1 000 000 x 8                                  thin: the flat path (the second is to_interleaved's shape)
-> profiles/mat_transpose.txt.

  python tools/mat_transpose_bench.py --out profiles/mat_transpose.txt

Yardsticks, in the same process on tensors of the same shape and element size: torch's transpose-copy
x.t().contiguous(), and a plain device copy of the same bytes, y.copy_(x).

Timing: device events around ONE call -- the library's on its own stream, torch's on torch's -- because a transpose
changes the shape: the matrix is transposed back, untimed, before the next timed call.  Every leg is warmed and then
repeated until the timed calls add up to at least 0.2 s (at most 2000 calls); a figure is the mean of a leg.  The legs
alternate torch, transpose, torch, transpose, torch, copy: the torch leg's three repeats give the run-to-run spread
(largest - smallest) / smallest, and the smallest mean of each kind of leg is shown.  GB/s = the bytes a transpose has
to read once and write once over the time.

Goal (not fixed in advance): on the four large shapes transpose is no slower than torch's transpose-copy within the
spread of the torch leg; the ratio to the plain copy is reported beside it.  The verdict per shape is in the table.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LARGE = ((16384, 2048), (2048, 16384), (16384, 1000), (65536, 100))
THIN = ((70000, 3), (1000000, 8))
KINDS = (("f32", "float32", False), ("c32", "float32", True), ("f64", "float64", False), ("c64", "float64", True))
MIN_TIME = 0.2
MAX_CALLS = 2000
WARM = 3


def ok(code):
    assert code == 0, code


def leg(timed_call):
    """mean seconds of timed_call() -> seconds, warmed, over calls that add up to MIN_TIME"""
    for _ in range(WARM):
        timed_call()
    total, count = 0.0, 0
    while total < MIN_TIME and count < MAX_CALLS:
        total += timed_call()
        count += 1
    return total / count


def run(out):
    import numpy as np
    import torch
    import basic_dsp_amd as bd
    bd.require_gpu()
    lib = bd.lib
    e0, e1 = C.c_void_p(lib.bdsp_hip_event_create()), C.c_void_p(lib.bdsp_hip_event_create())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = C.c_float()
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# DspMat.transpose (mat_transpose.hip) on one MI355X: tools/mat_transpose_bench.py.  Device events around one call;")
    w("# every leg warmed, calls adding up to >= %.1f s (at most %d); legs alternate torch, transpose, torch, transpose, torch," % (MIN_TIME, MAX_CALLS))
    w("# copy.  Shown: the smallest mean of a kind of leg; spread = (largest - smallest) / smallest of the three torch legs.")
    w("# torch = x.t().contiguous() on a tensor of the same shape and element size; copy = y.copy_(x) of the same bytes.")
    w("# GB/s = (bytes read once + bytes written once) / time of transpose.  Goal on the four large shapes: transpose no")
    w("# slower than torch within the torch leg's spread.")
    w("%-5s %-16s %12s %8s %10s %8s %9s %11s %11s  %s" % ("kind", "rows x points", "transpose us", "GB/s", "torch us", "spread",
                                                        "copy us", "tr / torch", "tr / copy", "verdict"))
    verdicts = []
    for kind, dtype, cplx in KINDS:
        e = 2 if cplx else 1
        elem = np.dtype(dtype).itemsize * e
        tdt = {("float32", False): torch.float32, ("float32", True): torch.complex64, ("float64", False): torch.float64,
               ("float64", True): torch.complex128}[(dtype, cplx)]
        for rows, points in LARGE + THIN:
            m = bd.DspMat(rows=rows, row_len=points * e, is_complex=cplx, dtype=np.dtype(dtype).type)
            ok(m.offset(1.0))
            x = torch.ones(rows, points, dtype=tdt, device="cuda")
            y = torch.empty(rows, points, dtype=tdt, device="cuda")

            def ours():
                ok(lib.bdsp_hip_event_record(e0, None))
                ok(m.transpose())
                ok(lib.bdsp_hip_event_record(e1, None))
                ok(m.transpose())  # back, untimed
                ok(lib.bdsp_hip_synchronize(None))
                ok(lib.bdsp_hip_event_elapsed_ms(e0, e1, C.byref(ms)))
                return ms.value * 1e-3

            def theirs():
                t0.record()
                z = x.t().contiguous()
                t1.record()
                torch.cuda.synchronize()
                del z
                return t0.elapsed_time(t1) * 1e-3

            def copy():
                t0.record()
                y.copy_(x)
                t1.record()
                torch.cuda.synchronize()
                return t0.elapsed_time(t1) * 1e-3

            tt, to = [], []
            tt.append(leg(theirs))
            to.append(leg(ours))
            tt.append(leg(theirs))
            to.append(leg(ours))
            tt.append(leg(theirs))
            tc = leg(copy)
            assert m.rows() == rows and m.row_points() == points
            spread = (max(tt) - min(tt)) / min(tt)
            tr, th = min(to), min(tt)
            large = (rows, points) in LARGE
            verdict = "" if not large else ("holds" if tr <= th * (1.0 + spread) else "MISSES")
            if large:
                verdicts.append((kind, rows, points, tr / th, spread, verdict))
            w("%-5s %-16s %12.1f %8.0f %10.1f %7.1f%% %9.1f %11.2f %11.2f  %s" % (
                kind, "%d x %d" % (rows, points), tr * 1e6, 2 * rows * points * elem / tr / 1e9, th * 1e6, spread * 100,
                tc * 1e6, tr / th, tr / tc, verdict))
            del m, x, y
            torch.cuda.empty_cache()
    missed = [v for v in verdicts if v[5] != "holds"]
    w("# goal: holds on %d of %d (kind, large shape) cases" % (len(verdicts) - len(missed), len(verdicts)))
    for kind, rows, points, ratio, spread, _ in missed:
        w("#   misses: %s %d x %d: transpose / torch = %.2f at a spread of %.1f%%" % (kind, rows, points, ratio, spread * 100))
    lib.bdsp_hip_event_destroy(e0)
    lib.bdsp_hip_event_destroy(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []
    run(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
