"""DspMat.correlate (mat_correlate.hip) against what a user could do before it existed -> profiles/mat_correlate.txt.

  compose  the public composition zero_pad(L, Surround) -> plain_fft -> mul / mul_vector -> plain_ifft -> scale(1/L) ->
           swap_halves on the whole matrix
  loop     get_row + DspVec.correlate for LOOP_ROWS rows, extrapolated to the row count (labelled as such)

Modes, so that kernel times come from a profiled run of their own:
  --mode time    call times: host clock around the call(s) and the stream synchronisation that ends them; every
                 repeat runs on a fresh matrix (correlate grows the rows), the variants alternate within one process,
                 each is warmed up per shape; median and range of REPS repeats; outputs compared at the timed size
  --mode prof    a few calls per shape for `rocprofv3 --kernel-trace --stats`, each between two marker launches
                 (a per-row sum of a tiny matrix: the only k_mr_stats kernels of the run); logs the segment labels
  --mode report  (CPU) joins the time JSON, the segment log and the kernel-trace CSV into the text report
"""
import argparse
import csv
import glob
import json
import os
import statistics as pystats
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s
REPS, LOOP_ROWS = 5, 256
SURROUND = 1
# (name, rows, p, L, dtype, argument kind)
SHAPES = [("f32 16384x1000->2048 vector (fused)", 16384, 1000, 2048, "f32", "vector"),
          ("f32 4096x4095->4096 matrix (fused)", 4096, 4095, 4096, "f32", "matrix"),
          ("f32 16384x1013->2025 vector (general, smooth)", 16384, 1013, 2025, "f32", "vector"),
          ("f32 4096x1000->1999 vector (general, Bluestein)", 4096, 1000, 1999, "f32", "vector"),
          ("f64 8192x1000->2048 vector (fused)", 8192, 1000, 2048, "f64", "vector"),
          ("f32 65536x100->256 matrix (fused)", 65536, 100, 256, "f32", "matrix")]
# the general path's launch count must not depend on the row count: the same lengths at 16 rows
PROF_EXTRA = [("f32 16x1013->2025 vector (general, smooth)", 16, 1013, 2025, "f32", "vector"),
              ("f32 16x1000->1999 vector (general, Bluestein)", 16, 1000, 1999, "f32", "vector")]


def sync(bd):
    bd._lib.check(bd._lib.lib.bdsp_hip_synchronize(None), "synchronize")


def host_data(np, rows, p, l, dt, kind):
    dtype = np.float32 if dt == "f32" else np.float64
    rng = np.random.default_rng(rows * 31 + p)
    base = rng.uniform(-10, 10, (1 << 20) + 7).astype(dtype)  # (tiled: host generation stays cheap)
    x = np.resize(base, rows * 2 * p).reshape(rows, 2 * p)
    arows = rows if kind == "matrix" else 1
    y = np.resize(base[::-1], arows * 2 * p).reshape(arows, 2 * p)
    return x, y


def argument(bd, y, l, kind):
    a = bd.DspMat(y, is_complex=True) if kind == "matrix" else bd.DspVec(y[0], is_complex=True)
    p = y.shape[1] // 2
    if l == 2 * p - 1:
        assert a.prepare_argument_padded() == 0
    else:
        assert a.zero_pad(l, SURROUND) == 0 and a.prepare_argument() == 0
    return a


def v_correlate(m, arg, l):
    assert m.correlate(arg) == 0


def v_compose(m, arg, l):
    assert m.zero_pad(l, SURROUND) == 0 and m.plain_fft() == 0 and m.mul(arg) == 0 and m.plain_ifft() == 0
    assert m.scale(1.0 / l) == 0 and m.swap_halves() == 0


def v_loop(m, arg, kind, n):
    out = []
    for r in range(n):
        v = m.get_row(r)
        assert v.correlate(arg.get_row(r) if kind == "matrix" else arg) == 0
        out.append(v)
    return out


def rel_l2_rows(np, a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)))


def run_time(out_path):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    res = []
    for name, rows, p, l, dt, kind in SHAPES:
        x, y = host_data(np, rows, p, l, dt, kind)
        arg = argument(bd, y, l, kind)
        rec = {"case": name, "rows": rows, "p": p, "L": l, "dtype": dt, "kind": kind}
        # warm-up of every variant at this shape, and the outputs against each other
        ma, mb = bd.DspMat(x, is_complex=True), bd.DspMat(x, is_complex=True)
        v_correlate(ma, arg, l)
        v_compose(mb, arg, l)
        n = min(LOOP_ROWS, rows)
        vs = v_loop(bd.DspMat(x[:n], is_complex=True), arg, kind, n)
        sync(bd)
        a, b = ma.data(), mb.data()
        rec["max row rel-L2 correlate vs compose"] = rel_l2_rows(np, a, b)
        rec["max row rel-L2 correlate vs loop"] = rel_l2_rows(np, a[:n], np.stack([v.data() for v in vs]))
        del ma, mb, vs, a, b
        ta, tb = [], []
        for _ in range(REPS):  # alternating, each on a fresh matrix
            for fn, ts in ((v_correlate, ta), (v_compose, tb)):
                m = bd.DspMat(x, is_complex=True)
                sync(bd)
                t0 = time.perf_counter()
                fn(m, arg, l)
                sync(bd)
                ts.append(time.perf_counter() - t0)
                del m
        rec["correlate"], rec["compose"] = ta, tb
        tl = []
        for _ in range(3):
            m = bd.DspMat(x[:n], is_complex=True)
            sync(bd)
            t0 = time.perf_counter()
            vs = v_loop(m, arg, kind, n)
            sync(bd)
            tl.append(time.perf_counter() - t0)
            del m, vs
        rec["loop"], rec["loop_rows"] = tl, n
        res.append(rec)
        del arg
        print(name, "done: correlate %.0f us, compose %.0f us" % (pystats.median(ta) * 1e6, pystats.median(tb) * 1e6),
              flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def run_prof(out_path):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    tiny = bd.DspMat(np.ones((2, 8), np.float32))
    seq = []

    def mark(label):  # the segment that ENDS at this marker
        tiny.sum()
        seq.append(label)

    for name, rows, p, l, dt, kind in SHAPES + PROF_EXTRA:
        x, y = host_data(np, rows, p, l, dt, kind)
        arg = argument(bd, y, l, kind)
        ms = [bd.DspMat(x, is_complex=True) for _ in range(5)]
        v_correlate(ms[0], arg, l)  # warm-up
        sync(bd)
        mark("setup")
        for m in ms[1:4]:
            v_correlate(m, arg, l)
            sync(bd)
            mark("correlate|" + name)
        if rows <= 4096:
            v_compose(ms[4], arg, l)
            sync(bd)
            mark("compose|" + name)
        del ms, arg
    with open(out_path, "w") as f:
        json.dump(seq, f, indent=1)


def short(k):
    k = k.replace("void ", "").replace("bdsp::", "")
    return k[:k.index("(")] if "(" in k else k


def segments(trace_dir):
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    segs, cur, in_mark = [], [], False
    for r in rows:
        k = r["Kernel_Name"]
        if "k_mr_stats" in k or "k_mr_fold" in k:  # (k_mr_wg & co. are the mixed-radix transforms)
            if not in_mark:
                segs.append(cur)
                cur, in_mark = [], True
            continue
        in_mark = False
        cur.append((short(k), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    return segs


def spread(ts):
    return "%9.1f [%8.1f .. %8.1f]" % (pystats.median(ts) * 1e6, min(ts) * 1e6, max(ts) * 1e6)


def report(time_path, seq_path, trace_dir):
    L = []
    w = L.append
    w("# DspMat.correlate on one MI355X: tools/mat_correlate_bench.py")
    w("# call us = host clock around the call(s) and the stream synchronisation, median [min .. max] of %d repeats after a" % REPS)
    w("# warm-up, variants alternating in one process, every repeat on a fresh matrix: each variant's first call on a")
    w("# matrix also pays the reallocation of its two buffers to the longer rows and the copy of the old rows")
    w("# compose = zero_pad(L, Surround), plain_fft, mul / mul_vector, plain_ifft, scale(1/L), swap_halves")
    w("# loop = get_row + DspVec.correlate over %d rows, EXTRAPOLATED linearly to the row count" % LOOP_ROWS)
    w("")
    if time_path:
        for r in json.load(open(time_path)):
            c, b = pystats.median(r["correlate"]), pystats.median(r["compose"])
            lp = pystats.median(r["loop"]) * r["rows"] / r["loop_rows"]
            w("%s" % r["case"])
            w("  correlate   %s us" % spread(r["correlate"]))
            w("  compose     %s us   = %.2fx correlate" % (spread(r["compose"]), b / c))
            w("  loop        %9.1f us for %d rows -> extrapolated %.1f ms = %.0fx correlate" % (
                pystats.median(r["loop"]) * 1e6, r["loop_rows"], lp * 1e3, lp / c))
            w("  outputs     max row rel-L2: correlate vs compose %.2e, vs loop %.2e" % (
                r["max row rel-L2 correlate vs compose"], r["max row rel-L2 correlate vs loop"]))
        w("")
    if seq_path and trace_dir:
        seq = json.load(open(seq_path))
        segs = segments(trace_dir)
        assert len(segs) >= len(seq), (len(segs), len(seq))
        shapes = {s[0]: s for s in SHAPES + PROF_EXTRA}
        w("# kernels per call: rocprofv3 --kernel-trace in a run of its own; a call's kernels are those between two marker")
        w("# launches; need = rows (p + L) 2 sizeof(T) + the argument, over 8 TB/s")
        seen = {}
        for label, seg in zip(seq, segs):
            if label == "setup":
                continue
            seen.setdefault(label, []).append(seg)
        for label, calls in seen.items():
            what, name = label.split("|", 1)
            _, rows, p, l, dt, kind = shapes[name]
            esz = 4 if dt == "f32" else 8
            need = rows * (p + l) * 2 * esz + (rows if kind == "matrix" else 1) * l * 2 * esz
            counts = sorted(set(len(c) for c in calls))
            tot = pystats.median([sum(ns for _, ns in c) for c in calls]) * 1e-9
            names = {}
            for k, ns in calls[-1]:
                c = names.setdefault(k, [0, 0])
                c[0] += 1
                c[1] += ns
            w("%-10s %-52s launches %s  kernel time %9.1f us  need %7.1f MB = %6.1f us at 8 TB/s (%.2f of it)" % (
                what, name, "/".join(map(str, counts)), tot * 1e6, need / 1e6, need / HBM_PEAK * 1e6,
                need / HBM_PEAK / tot if tot else 0))
            for k, c in names.items():
                if k.startswith("k_mc_correlate"):
                    w("           %s alone: %.1f us = %.2f of 8 TB/s on the bytes it must move" % (
                        k, c[1] * 1e-3, need / HBM_PEAK / (c[1] * 1e-9)))
            w("           " + ", ".join("%s%s %.1f us" % (k, " x%d" % c[0] if c[0] > 1 else "", c[1] * 1e-3)
                                        for k, c in names.items())[:600])
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("time", "prof", "report"), required=True)
    ap.add_argument("--out")
    ap.add_argument("--time")
    ap.add_argument("--seq")
    ap.add_argument("--trace")
    a = ap.parse_args()
    if a.mode == "report":
        text = report(a.time, a.seq, a.trace)
        if a.out:
            open(a.out, "w").write(text)
        sys.stdout.write(text)
    elif a.mode == "time":
        run_time(a.out)
    else:
        run_prof(a.out)


if __name__ == "__main__":
    main()
