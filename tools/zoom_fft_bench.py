"""zoom_fft of the rows of a matrix (zoom_fft.hip) against the composition it replaces: 16 384 rows x 1000 complex f32
points -> 64 bins at 16x zoom (step 1 / 16 000), with one start for all rows and with one start per row, beside
zero_pad to 16 000 points -> plain_fft (the whole 16x grid; the crop to 64 bins that would follow has no call of its own
and is left out, in the composition's favour) -> profiles/zoom_fft.txt.  A vector call and a general-path shape
(8192 x 5000 -> 100 bins) are timed beside them.

  --mode time    per-call times (text table on stdout, --out writes it)
  --mode prof    a few calls of every case, at the full row count and at a small one, for a
                 `rocprofv3 --kernel-trace --stats` run of its own; every call sits between two one-element `scale`
                 calls that mark its boundaries in the trace; logs the call order as JSON (--out)
  --mode counts  (CPU) joins the call log (--seq) with the kernel-trace CSV (--trace): kernels per call, their times,
                 and the check that the launch count does not depend on the row count

Timing, as tools/mat_sym_bench.py: every case is warmed (the chirp tables are cached afterwards), each figure is the mean
over windows of at least 0.3 s in all, one call and a device synchronisation inside each window (the library's calls
are asynchronous).  A call changes the row length, so every call gets a fresh matrix (copied on the device, untimed):
the figure includes growing the matrix's two buffers where the result is longer than the input.  The kernels alone are
in the trace.  The cases alternate, two rounds each, the smaller mean is shown.
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

WINDOW = 0.3
SMALL_ROWS = 256
ZOOM, BINS = 16, 64
# (label, rows, N, bins, step, what)
CASES = [
    ("zoom one start", 16384, 1000, BINS, 1.0 / (ZOOM * 1000), "scalar"),
    ("zoom per-row starts", 16384, 1000, BINS, 1.0 / (ZOOM * 1000), "rows"),
    ("zero_pad + plain_fft", 16384, 1000, ZOOM * 1000, None, "composition"),
    ("zoom general path", 8192, 5000, 100, 1.0 / (ZOOM * 5000), "scalar"),
    ("zoom vector", 1, 1000, BINS, 1.0 / (ZOOM * 1000), "scalar"),
]


def sync(bd):
    bd.lib.bdsp_hip_synchronize(None)


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


def build(np, rows, n):
    """uniform noise tiled along the rows keeps the host generation cheap"""
    rng = np.random.default_rng(rows + n)
    tile = rng.uniform(-1.0, 1.0, (min(rows, 512), 2 * n))
    return np.ascontiguousarray(np.resize(tile, (rows, 2 * n))).astype(np.float32)


def runner(bd, np, case, rows):
    _, _, n, bins, step, what = case
    if what == "composition":
        def fn(m):
            assert m.zero_pad(bins, 0) == 0 and m.plain_fft() == 0
        return fn
    start = np.linspace(-0.4, 0.4, rows) if what == "rows" else 0.123

    def fn(m):
        assert bd.zoom_fft(m, start, step, bins) == 0
    return fn


def fresh_maker(bd, np, master, rows, n):
    def fresh():
        m = bd.DspMat(rows=rows, row_len=2 * n, dtype=np.float32, is_complex=True)
        m.add(master)
        return m
    return fresh


def run_time(out):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    w = lambda s: (print(s, flush=True), out.append(s))
    w("# zoom_fft of the rows of a matrix (zoom_fft.hip) on one MI355X: tools/zoom_fft_bench.py --mode time")
    w("# complex f32; every figure: a fresh matrix copied on the device (untimed), then ONE call and a device synchronisation")
    w("# inside the timed window; windows repeated until they add up to >= %.1f s; every case warmed first (chirp tables" % WINDOW)
    w("# cached); the cases alternate, two rounds each, the smaller mean is shown.  zero_pad + plain_fft computes the whole")
    w("# %dx grid (the crop to %d bins is left out: the library has no call for it) and grows the matrix's buffers %dx." % (ZOOM, BINS, ZOOM))
    w("%-24s %7s %6s %7s %12s" % ("case", "rows", "N", "bins", "us per call"))
    times = {c[0]: [] for c in CASES}
    masters = {}
    for _ in range(2):
        for case in CASES:
            label, rows, n = case[0], case[1], case[2]
            if (rows, n) not in masters:
                masters[(rows, n)] = bd.DspMat(build(np, rows, n), is_complex=True)
            times[label].append(burst_time(bd, fresh_maker(bd, np, masters[(rows, n)], rows, n), runner(bd, np, case, rows)))
    for case in CASES:
        w("%-24s %7d %6d %7d %12.1f" % (case[0], case[1], case[2], case[3], min(times[case[0]]) * 1e6))
    z, c = min(times["zoom one start"]), min(times["zero_pad + plain_fft"])
    w("# zero_pad + plain_fft / zoom one start = %.1f; / zoom per-row starts = %.1f" % (c / z, c / min(times["zoom per-row starts"])))


def run_prof(out_path):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    seq = []
    mark = bd.DspMat(np.ones((1, 1), np.float32))
    for case in CASES:
        label, rows, n = case[0], case[1], case[2]
        for r in sorted({rows, min(rows, SMALL_ROWS)}, reverse=True):
            x = build(np, r, n)
            fn = runner(bd, np, case, r)
            fn(bd.DspMat(x, is_complex=True))  # unmarked: plans and tables of these lengths exist afterwards
            for _ in range(3):
                m = bd.DspMat(x, is_complex=True)
                sync(bd)
                mark.scale(1.0)
                fn(m)
                mark.scale(1.0)
                sync(bd)
                del m
            seq.append({"case": label, "rows": r, "calls": 3})
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
    print("# kernels around a call; kernel us = sum over the call's kernels, last of 3 calls.  launches = the library's own")
    print("# kernels: the runtime's __amd_rocclr_copyBuffer (how it carries out a small host-to-device or device-to-device")
    print("# copy; larger ones go to a DMA engine and leave no kernel) is listed and timed but not counted")
    print("%-24s %7s %8s %10s  %s" % ("case", "rows", "launches", "kernel us", "kernels"))
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
        own = len([n for n in names if not n.startswith("__amd_rocclr")])
        per_case.setdefault(s["case"], []).append(own)
        print("%-24s %7d %8d %10.1f  %s" % (s["case"], s["rows"], own, us, " + ".join(names)))
    for k, v in per_case.items():
        if k.startswith("zoom"):
            assert len(set(v)) == 1, ("the launch count depends on the row count", k, v)
    print("# the launch count of every zoom_fft case is the same at both row counts")


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
