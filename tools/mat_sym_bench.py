"""Symmetric real-signal transforms of the rows of a matrix (DspMat.sfft / sifft, mat_sym.hip) against (a) the
composition available without them, get_row -> vector call -> set_row into a fresh matrix of the new row length, and
(b) what one batched call could do before: DspMat.fft() on the same real matrix, the full spectrum without the crop
(forward form only) -> profiles/mat_sym.txt.

  --mode time    per-call times, the row loop alternating with the batched calls in one process (text table on stdout)
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
FREQ = 1
# (rows, real points per row N, dtype name, transform path)
CASES = [
    (16384, 1001, "float32", "mixed radix, workgroup"),
    (65536, 45, "float32", "mixed radix, resident"),
    (64, 1048575, "float32", "chirp-z"),
    (16384, 1001, "float64", "mixed radix, workgroup"),
]
OPS = ("sfft", "fft", "sifft")  # fft: the full spectrum of the same real matrix, (b)


def sync(bd):
    bd.lib.bdsp_hip_synchronize(None)


def label(case, op):
    rows, n, dt, _ = case
    return "%s %dx%d %s" % (dt, rows, n, op)


def call(obj, op):
    code = getattr(obj, op)()
    assert code == 0, (op, code)


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


def build(np, rows, n, dtype, op):
    """uniform noise tiled along the rows keeps the host generation cheap; half spectra for the inverse form, the bin
    that is first after ifft_shift real"""
    p = n // 2 + 1
    width = 2 * p if op == "sifft" else n
    rng = np.random.default_rng(rows + n)
    tile = rng.uniform(-1.0, 1.0, (min(rows, 512), width))
    if op == "sifft":
        tile[:, 2 * (p // 2) + 1] = 0.0
    return np.ascontiguousarray(np.resize(tile, (rows, width))).astype(dtype)


def kwargs(op):
    return dict(is_complex=True, domain=FREQ) if op == "sifft" else {}


def out_len(n, op):
    p = n // 2 + 1
    return {"sfft": 2 * p, "fft": 2 * n, "sifft": n}[op]


def loop_rows(rows, points):
    return min(rows, LOOP_ROWS, max(1, (8 << 20) // points))


def run_time(out):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    w = lambda s: (print(s, flush=True), out.append(s))
    w("# Symmetric real-signal transforms of the rows of a matrix (mat_sym.hip) on one MI355X: tools/mat_sym_bench.py --mode time")
    w("# batched = one DspMat call; loop = get_row -> DspVec call -> set_row into a fresh matrix of the new row length, per row,")
    w("# timed on the first rows of the same data (%d rows; 8 for the rows of a million points) in the same process," % LOOP_ROWS)
    w("# alternating with the batched call: two rounds each, the smaller mean is shown.  fft = DspMat.fft() on the same real")
    w("# matrix: the full spectrum of N bins per row in one batched call, no crop (what one call could do before).")
    w("# Every figure: a fresh matrix copied on the device (untimed), then ONE call and a device synchronisation inside the")
    w("# timed window; windows repeated until they add up to >= %.1f s; every case warmed first.  A call on a fresh matrix" % WINDOW)
    w("# grows its two buffers to the new size: that is part of the batched figure (and of the vector call in the loop);")
    w("# the kernels alone are in the trace table below.")
    w("%-34s %-24s %11s %13s %14s" % ("case", "transform path", "batched us", "loop us / row", "loop/batched*"))
    res = {}
    for case in CASES:
        rows, n, dt, path = case
        dtype = np.dtype(dt).type
        lrows = loop_rows(rows, n)
        for op in OPS:
            x = build(np, rows, n, dtype, op)
            kw = kwargs(op)
            master, smaster = bd.DspMat(x, **kw), bd.DspMat(x[:lrows], **kw)
            width = x.shape[1]
            del x

            def fresh(src, r):
                m = bd.DspMat(rows=r, row_len=width, dtype=dtype, **kw)
                m.add(src)
                return m

            def loop(ms):
                dst = bd.DspMat(rows=lrows, row_len=out_len(n, op), dtype=dtype, is_complex=op != "sifft",
                                domain=FREQ if op != "sifft" else 0)
                for r in range(lrows):
                    v = ms.get_row(r)
                    call(v, op)
                    assert dst.set_row(r, v) == 0
                return dst
            tb, tl = [], []
            for _ in range(2):
                tb.append(burst_time(bd, lambda: fresh(master, rows), lambda m: call(m, op)))
                if op != "fft":
                    tl.append(burst_time(bd, lambda: fresh(smaster, lrows), loop) / lrows)
            b = min(tb)
            res[label(case, op)] = b
            if op == "fft":
                w("%-34s %-24s %11.1f %13s %14s" % (label(case, op), path, b * 1e6, "-", "-"))
            else:
                l = min(tl)
                w("%-34s %-24s %11.1f %13.2f %14.0f" % (label(case, op), path, b * 1e6, l * 1e6, l * rows / b))
            del master, smaster
    w("# * loop/batched: the per-row loop time times the row count, over the batched call -- an extrapolation from the")
    w("#   timed slice, not a measurement of the whole loop.")
    w("# the crop: sfft - fft per call, beside a copy of rows x (N + 1) complex elements (read + written) at 8 TB/s")
    for case in CASES:
        rows, n, dt, _ = case
        s, f = res[label(case, "sfft")], res[label(case, "fft")]
        copy = rows * (n + 1) * 2 * np.dtype(dt).itemsize / HBM_PEAK
        w("# %-32s sfft %9.1f us - fft %9.1f us = %8.1f us; copy floor %7.1f us" % (
            "%s %dx%d" % (dt, rows, n), s * 1e6, f * 1e6, (s - f) * 1e6, copy * 1e6))


def run_prof(out_path):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    seq = []
    mark = bd.DspMat(np.ones((1, 1), np.float32))
    for case in CASES:
        rows, n, dt, path = case
        dtype = np.dtype(dt).type
        small = LOOP_ROWS if rows > LOOP_ROWS else 8
        for op in OPS:
            for r in (rows, small):
                x = build(np, r, n, dtype, op)
                call(bd.DspMat(x, **kwargs(op)), op)  # unmarked: plans and tables of these lengths exist afterwards
                for _ in range(3):
                    m = bd.DspMat(x, **kwargs(op))
                    sync(bd)
                    mark.scale(1.0)
                    call(m, op)
                    mark.scale(1.0)
                    sync(bd)
                    del m
                seq.append({"case": label(case, op), "path": path, "rows": r, "calls": 3})
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
    print("%-34s %6s %8s %10s  %s" % ("case", "rows", "launches", "kernel us", "kernels"))
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
        print("%-34s %6d %8d %10.1f  %s" % (s["case"], s["rows"], len(last), us, " + ".join(names)))
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
