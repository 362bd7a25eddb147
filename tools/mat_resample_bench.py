"""FFT-domain resampling / decimation of the rows of a matrix (DspMat, mat_resample.hip) against the composition
available without it, get_row -> vector call -> set_row into a fresh matrix of the new row length
-> profiles/mat_resample.txt.

  --mode time    per-call times, the row loop alternating with the batched call in one process (text table on stdout)
  --mode prof    a few calls of every case, at the full row count and at a small one, for a
                 `rocprofv3 --kernel-trace --stats` run of its own; every call sits between two one-element `scale`
                 calls that mark its boundaries in the trace; logs the call order as JSON (--out)
  --mode counts  (CPU) joins the call log (--seq) with the kernel-trace CSV (--trace): kernels per call, their times,
                 and the check that the launch count does not depend on the row count

Timing: every case is warmed, each figure is the mean over windows of at least 0.3 s in all, one call and a device
synchronisation inside each window (the library's calls are asynchronous).  A call changes the row length, so every
call gets a fresh matrix (copied on the device, untimed): the figure includes growing the matrix's two buffers to the
new size and moving the rows into them, as a user's first call on a matrix does.  The kernels alone are in the trace.
The row loop is timed on a slice of LOOP_ROWS rows and reported per row; what it would cost over all rows is an
extrapolation and marked as one.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s
LOOP_ROWS = 256
WINDOW = 0.3
# (rows, points, op, argument, complex, dtype name, path)
CASES = [
    (16384, 1024, "interpft", 4096, True, "float32", "fused"),
    (16384, 1024, "interpft", 4096, False, "float32", "fused"),
    (16384, 1000, "interpft", 4000, True, "float32", "general, mixed radix"),
    (65536, 128, "interpft", 256, True, "float32", "fused"),
    (64, 1048576, "interpft", 2097152, True, "float32", "general"),
    (16384, 1024, "interpft", 4096, True, "float64", "fused"),
    (16384, 4096, "decimatei", 4, True, "float32", "one gather"),
]


def sync(bd):
    bd.lib.bdsp_hip_synchronize(None)


def label(case):
    rows, points, op, arg, cplx, dt, _ = case
    new = arg if op == "interpft" else points // arg
    return "%s %s %dx%d->%d %s" % (dt, "cplx" if cplx else "real", rows, points, new, op)


def new_points(case):
    _, points, op, arg, _, _, _ = case
    return arg if op == "interpft" else (points + arg - 1) // arg


def call(obj, case):
    op, arg = case[2], case[3]
    code = obj.interpft(arg) if op == "interpft" else obj.decimatei(arg, 0)
    assert code == 0, (case, code)


def burst_time(bd, make, fn, min_time=WINDOW):
    """Mean seconds per call: fresh input from make() (untimed), then one call and a device synchronisation inside the
    timed window; repeated until the timed windows add up to min_time."""
    fn(make())
    sync(bd)
    total, count = 0.0, 0
    while total < min_time:
        obj = make()
        sync(bd)
        t0 = time.perf_counter()
        fn(obj)
        sync(bd)
        total += time.perf_counter() - t0
        count += 1
    return total / count


def build(np, rows, points, cplx, dtype):
    """band-limited noise would do; uniform noise tiled along the rows keeps the host generation cheap"""
    e = 2 if cplx else 1
    rng = np.random.default_rng(rows + points)
    tile = rng.uniform(-1.0, 1.0, (min(rows, 512), points * e))
    return np.ascontiguousarray(np.resize(tile, (rows, points * e))).astype(dtype)


def loop_rows(rows, points):
    return min(rows, LOOP_ROWS, max(1, (8 << 20) // points))


def run_time(out):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    w = lambda s: (print(s, flush=True), out.append(s))
    w("# Resampling / decimation of the rows of a matrix (mat_resample.hip) on one MI355X: tools/mat_resample_bench.py --mode time")
    w("# batched = one DspMat call; loop = get_row -> DspVec call -> set_row into a fresh matrix of the new row length, per row,")
    w("# timed on the first rows of the same data (%d rows; 8 for the rows of a million points) in the same process," % LOOP_ROWS)
    w("# alternating with the batched call: two rounds each, the smaller mean is shown.")
    w("# Every figure: a fresh matrix copied on the device (untimed), then ONE call and a device synchronisation inside the")
    w("# timed window; windows repeated until they add up to >= %.1f s; every case warmed first.  A call on a fresh matrix" % WINDOW)
    w("# grows its two buffers to the new size and moves the rows into them: that is part of the batched figure (and of the")
    w("# vector call in the loop); the kernels alone are in the trace table below.")
    w("# floor = rows x (points read + new points written) x bytes per element / 8 TB/s")
    w("%-52s %-22s %11s %9s %13s %14s" % ("case", "path", "batched us", "floor us", "loop us / row", "loop/batched*"))
    res = {}
    for case in CASES:
        rows, points, op, arg, cplx, dt, path = case
        dtype = np.dtype(dt).type
        e = 2 if cplx else 1
        x = build(np, rows, points, cplx, dtype)
        lrows = loop_rows(rows, points)
        npts = new_points(case)
        master, smaster = bd.DspMat(x, is_complex=cplx), bd.DspMat(x[:lrows], is_complex=cplx)
        del x

        def fresh(src, r):
            m = bd.DspMat(rows=r, row_len=points * e, dtype=dtype, is_complex=cplx)
            m.add(src)
            return m

        def loop(ms):
            dst = bd.DspMat(rows=lrows, row_len=npts * e, dtype=dtype, is_complex=cplx)
            for r in range(lrows):
                v = ms.get_row(r)
                call(v, case)
                assert dst.set_row(r, v) == 0
            return dst
        tb, tl = [], []
        for _ in range(2):
            tb.append(burst_time(bd, lambda: fresh(master, rows), lambda m: call(m, case)))
            tl.append(burst_time(bd, lambda: fresh(smaster, lrows), loop) / lrows)
        b, l = min(tb), min(tl)
        floor = rows * (points + npts) * e * np.dtype(dt).itemsize / HBM_PEAK
        res[label(case)] = b
        w("%-52s %-22s %11.1f %9.1f %13.2f %14.0f" % (label(case), path, b * 1e6, floor * 1e6, l * 1e6, l * rows / b))
        del master, smaster
    w("# * loop/batched: the per-row loop time times the row count, over the batched call -- an extrapolation from the")
    w("#   timed slice, not a measurement of the whole loop.")
    f, g = res[label(CASES[0])], res[label(CASES[2])]
    w("# fused 16384 x 1024 -> 4096 over general 16384 x 1000 -> 4000 (complex f32, per call): %.1f us / %.1f us = %.2f" % (
        f * 1e6, g * 1e6, f / g))


def run_prof(out_path):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    seq = []
    mark = bd.DspMat(np.ones((1, 1), np.float32))
    for case in CASES:
        rows, points, op, arg, cplx, dt, path = case
        dtype = np.dtype(dt).type
        small = LOOP_ROWS if rows > LOOP_ROWS else 8
        for r in (rows, small):
            x = build(np, r, points, cplx, dtype)
            call(bd.DspMat(x, is_complex=cplx), case)  # unmarked: plans and tables of these lengths exist afterwards
            for _ in range(3):
                m = bd.DspMat(x, is_complex=cplx)
                sync(bd)
                mark.scale(1.0)
                call(m, case)
                mark.scale(1.0)
                sync(bd)
                del m
            seq.append({"case": label(case), "path": path, "rows": r, "calls": 3})
    json.dump(seq, open(out_path, "w"), indent=1)


def run_counts(seq_path, trace_dir):
    seq = json.load(open(seq_path))
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "OpRealScale" in r["Kernel_Name"]]
    calls = sum(s["calls"] for s in seq)
    assert len(marks) == 2 * calls, (len(marks), calls)
    print("# kernels per call from rocprofv3 --kernel-trace (a run of its own): every dispatch between the two marker")
    print("# kernels around a call; kernel us = sum over the call's kernels, last of 3 calls")
    print("%-52s %6s %8s %10s  %s" % ("case", "rows", "launches", "kernel us", "kernels"))
    c = 0
    per_case = {}
    for s in seq:
        last = None
        counts = set()
        for _ in range(s["calls"]):
            grp = rows[marks[2 * c] + 1:marks[2 * c + 1]]
            c += 1
            counts.add(len(grp))
            last = grp
        assert len(counts) == 1, (s, counts)
        names = [r["Kernel_Name"].replace("void ", "").replace("bdsp::", "").split("(")[0] for r in last]
        us = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in last) * 1e-3
        per_case.setdefault(s["case"], []).append(len(last))
        print("%-52s %6d %8d %10.1f  %s" % (s["case"], s["rows"], len(last), us, " + ".join(names)))
    for k, v in per_case.items():
        assert len(set(v)) == 1, ("the launch count depends on the row count", k, v)
    print("# the launch count of every case is the same at both row counts")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("time", "prof", "counts"), required=True)
    ap.add_argument("--out")
    ap.add_argument("--seq")
    ap.add_argument("--trace")
    a = ap.parse_args()
    if a.mode == "time":
        lines = []
        run_time(lines)
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")
    elif a.mode == "prof":
        run_prof(a.out)
    else:
        run_counts(a.seq, a.trace)


if __name__ == "__main__":
    main()
