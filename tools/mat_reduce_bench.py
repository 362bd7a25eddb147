"""Per-row matrix reductions (DspMat.statistics / sum / dot_product, mat_reduce.hip) against the flat single-vector
kernels on the same bytes and against the per-row get_row + vector-facade loop -> profiles/r07_mat_reduce.txt.

Three modes, so that kernel times come from a profiled run of their own:
  --mode time    call times (host clock around each call, which ends in its stream synchronisation) -> JSON
  --mode prof    the same calls, a few repetitions each, for `rocprofv3 --kernel-trace`; logs the call order -> JSON
  --mode report  (CPU) joins the time JSON, the call log and the kernel-trace CSV into the text report
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

HBM_PEAK, COPY_CEIL = 8.0e12, 6.29e12  # B/s: MI355X HBM3E peak; a float4 copy measured on this part
M = 1 << 20
SHAPES = [(65536, 128), (16384, 1000), (2048, 65536), (64, M), (4, 16 * M)]
SWEEP = [8, 16, 64, 256, 1024, 4096, 65536, M, 16 * M]  # points per row at 128 MiB of complex f32
LOOP_ROWS = 1024


def cases():
    """(name, rows, scalars per row, dtype name, complex, sweep point)"""
    out = []
    for rows, pts in SHAPES:
        out.append(("c32 %dx%d" % (rows, pts), rows, 2 * pts, "f32", True, False))
        out.append(("c64 %dx%d" % (rows, pts), rows, 2 * pts, "f64", True, False))
        out.append(("r32 %dx%d" % (rows, pts + 1), rows, pts + 1, "f32", False, False))
    for pts in SWEEP:
        rows = (128 * M // 8) // pts
        out.append(("sweep c32 %dx%d" % (rows, pts), rows, 2 * pts, "f32", True, True))
    return out


def stat_bytes(dt, cplx):
    return {("f32", False): 56, ("f64", False): 64, ("f32", True): 64, ("f64", True): 104}[(dt, cplx)]


def build(np, bd, rows, rl, dt, cplx):
    dtype = np.float32 if dt == "f32" else np.float64
    rng = np.random.default_rng(rows * 31 + rl)
    x = np.resize(rng.standard_normal(M + 7, dtype=dtype), rows * rl)  # (tiled: host generation stays cheap)
    m = bd.DspMat(x.reshape(rows, rl), is_complex=cplx)
    flat = bd.DspVec(x, is_complex=cplx)
    y = bd.DspVec(rng.standard_normal(rl, dtype=dtype), is_complex=cplx)
    return m, flat, y


def ops(m, flat, y):
    """what each case runs: matrix calls and their flat single-vector counterparts on the same bytes"""
    return [("mat statistics", lambda: m.statistics()),
            ("mat sum", lambda: m.sum()),
            ("mat dot(vector)", lambda: m.dot_product(y)),
            ("flat statistics", lambda: flat.statistics()),
            ("flat sum", lambda: flat.sum()),
            ("flat dot", lambda: flat.dot_product(flat))]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return pystats.median(ts)


def run(mode, out_path):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    res, seq = [], []
    for name, rows, rl, dt, cplx, sweep in cases():
        m, flat, y = build(np, bd, rows, rl, dt, cplx)
        rec = {"case": name, "rows": rows, "row_len": rl, "dtype": dt, "complex": cplx, "sweep": sweep}
        for op, fn in ops(m, flat, y):
            if mode == "time":
                rec[op] = timed(fn, 10)
            else:
                fn()  # warm-up (not logged separately: the report takes the last `reps` calls of each op)
                for _ in range(3):
                    fn()
                seq.append({"case": name, "op": op, "calls": 4})
        if mode == "time" and rows >= LOOP_ROWS and not sweep:
            n = LOOP_ROWS  # the per-row loop a user writes today: get_row (a device copy) + the vector facade
            for op, call in (("loop statistics", lambda v: v.statistics()), ("loop sum", lambda v: v.sum()),
                             ("loop dot(vector)", lambda v: v.dot_product(y))):
                call(m.get_row(0))
                t0 = time.perf_counter()
                for r in range(n):
                    call(m.get_row(r))
                rec[op + " (%d rows)" % n] = time.perf_counter() - t0
        res.append(rec)
        del m, flat, y
        print(name, "done", flush=True)
    with open(out_path, "w") as f:
        json.dump(res if mode == "time" else seq, f, indent=1)


PRIMARY = ("k_stats_contig", "k_dot<", "k_mr_stats", "k_mr_dot")
SECONDARY = ("k_stats_final", "k_mr_fold")


def kernel_calls(trace_dir):
    """kernel-trace CSV -> list of (kernel names, ns) per library call, in dispatch order"""
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        k = r["Kernel_Name"]
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if any(p in k for p in PRIMARY):
            calls.append([[k], ns])
        elif any(s in k for s in SECONDARY) and calls:
            calls[-1][0].append(k)
            calls[-1][1] += ns
    return calls


def short(k):
    k = k.replace("void ", "").replace("bdsp::", "")
    return k[:k.index("(")] if "(" in k else k


def report(time_path, seq_path, trace_dir):
    times = {r["case"]: r for r in json.load(open(time_path))}
    seq = json.load(open(seq_path))
    calls = kernel_calls(trace_dir)
    need = sum(s["calls"] for s in seq)
    assert len(calls) == need, (len(calls), need)
    kt, names, i = {}, {}, 0
    for s in seq:
        grp = calls[i:i + s["calls"]]
        i += s["calls"]
        kt[(s["case"], s["op"])] = pystats.median([g[1] for g in grp[1:]]) * 1e-9
        names[(s["case"], s["op"])] = " + ".join(short(k) for k in grp[-1][0])
    L = []
    w = L.append
    w("# Per-row matrix reductions (mat_reduce.hip) on one MI355X: tools/mat_reduce_bench.py")
    w("# call = host clock around the Python call (ends in the call's stream synchronisation), median of 10 after warm-up")
    w("# kernel = rocprofv3 --kernel-trace in a run of its own, median of 3 after warm-up, all kernels of the call summed")
    w("# read = input bytes (mat dot: the matrix + one broadcast vector), written = result bytes")
    w("# %8TB = read / kernel over 8 TB/s; %copy = over 6.29 TB/s (float4 copy on this part); flat = the single-vector")
    w("# kernels (k_stats_contig / k_dot + final) on a vector of the same bytes, same process; ratio = mat / flat kernel")
    w("")
    hdr = "%-30s %-16s %9s %9s %8s %6s %6s %9s %6s  %s" % ("case", "op", "call us", "kern us", "RW GB/s", "%8TB",
                                                         "%copy", "flat us", "ratio", "kernels")
    for sweep in (False, True):
        w("## " + ("row-length sweep, 128 MiB complex f32 (L < 64: RW GB/s counts bytes read + written)" if sweep
                   else "shapes"))
        w(hdr)
        for case, r in times.items():
            if r["sweep"] != sweep:
                continue
            esz = 4 if r["dtype"] == "f32" else 8
            rd = r["rows"] * r["row_len"] * esz
            for op, flat in (("mat statistics", "flat statistics"), ("mat sum", "flat sum"),
                             ("mat dot(vector)", "flat dot")):
                k, fk = kt[(case, op)], kt[(case, flat)]
                if op == "mat statistics":
                    wr = r["rows"] * stat_bytes(r["dtype"], r["complex"])
                else:
                    wr = r["rows"] * esz * (2 if r["complex"] else 1)
                rbytes = rd + (r["row_len"] * esz if "dot" in op else 0)
                w("%-30s %-16s %9.1f %9.1f %8.0f %6.3f %6.3f %9.1f %6.2f  %s" % (
                    case, op, r[op] * 1e6, k * 1e6, (rbytes + wr) / k / 1e9, rbytes / k / HBM_PEAK,
                    rbytes / k / COPY_CEIL, fk * 1e6, k / fk,
                    names[(case, op)]))
            for key in sorted(x for x in r if x.startswith("loop ")):
                op, n = key.rsplit(" (", 1)
                n = int(n.split()[0])
                w("%-30s %-16s %9.0f us for %d rows; extrapolated to %d rows: %.1f ms = %.0fx the batched call" % (
                    case, op, r[key] * 1e6, n, r["rows"], r[key] * r["rows"] / n * 1e3,
                    r[key] * r["rows"] / n / r["mat " + op[5:]]))
        w("")
    w("# flat dot = the vector with itself (k_dot reads the same bytes through both operands)")
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
    else:
        run(a.mode, a.out)


if __name__ == "__main__":
    main()
