"""Per-row unwrap / cum_sum / diff of a matrix (DspMat, mat_scan.hip) against the composition available without them,
get_row -> vector op -> set_row over the rows -> profiles/mat_scan.txt.

  --mode time    per-call times, the row loop alternating with the batched call in one process (text table on stdout)
  --mode prof    a few calls of every op and shape for a `rocprofv3 --kernel-trace --stats` run of its own; logs the
                 call order as JSON (--out)
  --mode counts  (CPU) joins the call log (--seq) with the kernel-trace CSV (--trace): kernels per call and their times

Timing: every shape is warmed, each figure is the mean over a window of at least 0.3 s of back-to-back calls with a
device synchronisation inside the window (the library's calls are asynchronous).  The row loop is timed on a slice of
LOOP_ROWS rows and reported per row; what it would cost over all rows is stated in words only.
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
SHAPES = [(16384, 1000), (64, 1000000), (65536, 100)]
LOOP_ROWS = 256
WINDOW = 0.3
OPS = ("unwrap", "cum_sum", "diff")
TWO_PI = 6.283185307179586


def sync(bd):
    bd.lib.bdsp_hip_synchronize(None)


def burst_time(bd, make, fn, calls, min_time=WINDOW):
    """Mean seconds per call: fresh input from make() (untimed), then `calls` calls and a device synchronisation
    inside the timed window; bursts are repeated until the timed windows add up to min_time."""
    fn(make())
    sync(bd)
    total, count = 0.0, 0
    while total < min_time:
        obj = make()
        sync(bd)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(obj)
        sync(bd)
        total += time.perf_counter() - t0
        count += calls
    return total / count


def build(np, bd, rows, n, dtype):
    """wrapped phase ramps, a different slope per row: unwrap has work to do on every row"""
    rng = np.random.default_rng(rows + n)
    slopes = rng.uniform(0.5, 2.5, rows)[:, None]
    base = np.arange(min(n, 4096), dtype=np.float64)[None, :]
    tile = np.mod(base * slopes + np.pi, TWO_PI) - np.pi     # (tiled along the row: host generation stays cheap)
    x = np.ascontiguousarray(np.resize(tile, (rows, n)) if n <= 4096 else np.tile(tile, (1, -(-n // 4096)))[:, :n])
    return x.astype(dtype)


def mat_op(m, op, dtype):
    if op == "unwrap":
        return m.unwrap(dtype(TWO_PI))
    return getattr(m, op)()


def vec_op(v, op, dtype):
    if op == "unwrap":
        return v.unwrap(dtype(TWO_PI))
    return getattr(v, op)()


def run_time(out):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    w = lambda s: (print(s, flush=True), out.append(s))
    w("# Per-row unwrap / cum_sum / diff of a matrix (mat_scan.hip) on one MI355X: tools/mat_scan_bench.py --mode time")
    w("# batched = one DspMat call; loop = get_row -> DspVec op -> set_row per row (diff: no set_row, the row got shorter),")
    w("# timed on the first rows of the same data (%d rows; 8 for the rows of a million points) in the same process," % LOOP_ROWS)
    w("# alternating with the batched call: two rounds each, the smaller mean is shown.")
    w("# Every figure: fresh wrapped input copied on the device (untimed), then the call(s) and a device synchronisation")
    w("# inside the timed window; windows repeated until they add up to >= %.1f s; every shape warmed first." % WINDOW)
    w("# The window holds one synchronisation per call (diff: per 4 calls): a few us of host latency are part of each figure.")
    w("# bytes = rows x row_len x sizeof(T) read + the same written (diff: one point per row less written);")
    w("# %8TB = bytes / batched time over 8 TB/s (unwrap is bound by its serial chain, not by bandwidth: no share shown)")
    w("%-22s %-8s %12s %14s %10s %8s %14s" % ("shape", "op", "batched us", "loop us / row", "GB/s", "%8TB", "loop/batched*"))
    for rows, n in SHAPES:
        for dtype in (np.float32, np.float64):
            x = build(np, bd, rows, n, dtype)
            esz = x.dtype.itemsize
            lrows = min(rows, LOOP_ROWS, max(1, (8 << 20) // n))
            master, smaster = bd.DspMat(x), bd.DspMat(x[:lrows])

            def fresh(src, r):
                m = bd.DspMat(rows=r, row_len=n, dtype=dtype)
                m.add(src)
                return m
            for op in OPS:
                def loop(ms):
                    for r in range(lrows):
                        v = ms.get_row(r)
                        vec_op(v, op, dtype)
                        if op != "diff":
                            ms.set_row(r, v)
                tb, tl = [], []
                for _ in range(2):
                    tb.append(burst_time(bd, lambda: fresh(master, rows), lambda m: mat_op(m, op, dtype), 4 if op == "diff" else 1))
                    tl.append(burst_time(bd, lambda: fresh(smaster, lrows), loop, 1) / lrows)
                b, l = min(tb), min(tl)
                nbytes = rows * n * esz + rows * (n - (1 if op == "diff" else 0)) * esz
                bw = nbytes / b
                share = "%8.3f" % (bw / HBM_PEAK) if op != "unwrap" else "%8s" % "-"
                w("%-22s %-8s %12.1f %14.2f %10.1f %s %14.0f" % ("%s %dx%d" % (x.dtype.name, rows, n), op, b * 1e6, l * 1e6,
                                                            bw / 1e9, share, l * rows / b))
            del master, smaster
    w("# * loop/batched: the per-row loop time times the row count, over the batched call -- an extrapolation from the")
    w("#   timed slice, not a measurement of the whole loop.")


def run_prof(out_path):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    seq = []
    shapes = SHAPES + [(300, 3000), (16, 100000)]  # + one workgroup per row, + the three-step cum_sum
    for rows, n in shapes:
        for dtype in (np.float32, np.float64):
            x = build(np, bd, rows, n, dtype)
            for op in OPS:
                for _ in range(3):
                    m = bd.DspMat(x)
                    mat_op(m, op, dtype)
                    sync(bd)
                seq.append({"shape": "%s %dx%d" % (x.dtype.name, rows, n), "op": op, "calls": 3})
    json.dump(seq, open(out_path, "w"), indent=1)


def run_counts(seq_path, trace_dir):
    seq = json.load(open(seq_path))
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = [r for r in csv.DictReader(open(path)) if "k_ms_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    print("# kernels per call from rocprofv3 --kernel-trace (a run of its own), k_ms_* kernels only; us = last of 3 calls")
    print("%-22s %-8s %8s %10s  %s" % ("shape", "op", "launches", "kernel us", "kernels"))
    i = 0
    for s in seq:
        per = {"unwrap": 1, "diff": 1}.get(s["op"])
        if per is None:  # cum_sum: one launch, or sums -> offsets -> apply
            per = 3 if "k_ms_scan_sums" in rows[i]["Kernel_Name"] else 1
        grp = rows[i:i + per * s["calls"]]
        i += per * s["calls"]
        last = grp[-per:]
        names = [r["Kernel_Name"].replace("void ", "").replace("bdsp::", "").split("(")[0] for r in last]
        want = {"unwrap": "k_ms_unwrap", "diff": "k_ms_diff", "cum_sum": "k_ms_scan"}[s["op"]]
        assert all(want in n for n in names), (s, names)
        us = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in last) * 1e-3
        print("%-22s %-8s %8d %10.1f  %s" % (s["shape"], s["op"], per, us, " + ".join(names)))
    assert i == len(rows), (i, len(rows))
    print("# every k_ms_* dispatch of the run is accounted for: %d dispatches in %d calls" % (len(rows), sum(s["calls"] for s in seq)))


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
