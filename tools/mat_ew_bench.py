"""The row-aware elementwise operations of a matrix (mat_ew.hip) on 16 384 x 2048 complex rows, f32 and f64:
  * DspMat.multiply_complex_exponential (k_mw_cexp: one phasor per position, reused down the rows) against
      (a) DspVec.multiply_complex_exponential on ONE vector of the same total size -- the same bytes moved, one
          double-precision sincos per element: the yardstick for whether sharing the phasor pays;
      (b) the get_row -> vector call -> set_row loop, timed on LOOP_ROWS rows, per row;
  * DspMat.reverse and DspMat.mul_smaller (a vector operand of 16 points) against the row loop;
  * DspMat.log(10) against DspVec.log(10) of the same size (the same kernel: expected equal)
-> profiles/mat_ew.txt.

  python tools/mat_ew_bench.py --out profiles/mat_ew.txt

Timing: every case is warmed; a figure is the mean over windows that add up to at least 0.3 s, each window a burst of
BURST calls on the same data and one device synchronisation (the library's calls are asynchronous), divided by BURST.
The mixer multiplies by unit phasors, reverse moves and mul_smaller multiplies by ones, so a burst runs on one matrix.
The matrix mixer and the vector mixer alternate in one process, ROUNDS rounds each; the smallest mean is shown with the
spread (largest - smallest) / smallest of each side's rounds, and the matrix kernel counts as faster only beyond the
larger spread.  log changes its data, so each of its calls gets a fresh copy (made on the device, untimed).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, POINTS = 16384, 2048
LOOP_ROWS = 256
WINDOW = 0.3
BURST = 10
ROUNDS = 3
A, B = 0.02, 0.3


def sync(bd):
    bd.lib.bdsp_hip_synchronize(None)


def burst_time(bd, fn, min_time=WINDOW):
    """mean seconds per call of fn over bursts of BURST calls"""
    for _ in range(3):
        fn()
    sync(bd)
    total, count = 0.0, 0
    while total < min_time:
        t0 = time.perf_counter()
        for _ in range(BURST):
            fn()
        sync(bd)
        total += time.perf_counter() - t0
        count += BURST
    return total / count


def single_time(bd, make, fn, min_time=WINDOW):
    """mean seconds per call: fresh input from make() (untimed), one call and a synchronisation in the window"""
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


def noise(np, rows, width, dtype):
    rng = np.random.default_rng(rows + width)
    tile = rng.uniform(0.5, 1.5, (min(rows, 512), width))
    return np.ascontiguousarray(np.resize(tile, (rows, width))).astype(dtype)


def ok(code):
    assert code == 0, code


def run(out):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# math family, reverse, mixer and *_smaller of the rows of a matrix (mat_ew.hip) on one MI355X: tools/mat_ew_bench.py.")
    w("# %d x %d complex rows.  A figure: bursts of %d calls and one device synchronisation per window, windows adding up" % (ROWS, POINTS, BURST))
    w("# to >= %.1f s, per call; every case warmed.  matrix = k_mw_cexp (one phasor per position, reused down the rows)," % WINDOW)
    w("# vector = DspVec.multiply_complex_exponential on one vector of rows * points (one sincos per element); the two")
    w("# alternate in one process, %d rounds each: smallest mean, spread = (largest - smallest) / smallest of the rounds." % ROUNDS)
    w("# The vector's phase a * k + b runs up to a * rows * points; a third measurement gives it a / rows, so that the size")
    w("# of the sincos argument is the matrix's.")
    w("%-8s %12s %8s %12s %8s %10s %9s" % ("mixer", "matrix us", "spread", "vector us", "spread", "vec / mat", "GB/s mat"))
    verdicts = []
    for dtype in (np.float32, np.float64):
        name = np.dtype(dtype).name
        x = noise(np, ROWS, 2 * POINTS, dtype)
        m = bd.DspMat(x, is_complex=True)
        v = bd.DspVec(x.reshape(-1), is_complex=True)
        del x
        tm, tv, ts = [], [], []
        for _ in range(ROUNDS):
            tm.append(burst_time(bd, lambda: ok(m.multiply_complex_exponential(A, B))))
            tv.append(burst_time(bd, lambda: ok(v.multiply_complex_exponential(A, B))))
            ts.append(burst_time(bd, lambda: ok(v.multiply_complex_exponential(A / ROWS, B))))
        sm, sv = (max(tm) - min(tm)) / min(tm), (max(tv) - min(tv)) / min(tv)
        ratio = min(tv) / min(tm)
        nbytes = 2.0 * ROWS * POINTS * 2 * np.dtype(dtype).itemsize  # read + write
        w("%-8s %12.1f %7.1f%% %12.1f %7.1f%% %10.2f %9.0f" % (name, min(tm) * 1e6, sm * 100, min(tv) * 1e6, sv * 100, ratio,
                                                           nbytes / min(tm) / 1e9))
        w("%-8s the vector call with a / %d, its phases within the matrix's range (a * %d): %.1f us" % (name, ROWS, POINTS, min(ts) * 1e6))
        verdicts.append((name, ratio, max(sm, sv)))

        # the row loop, LOOP_ROWS rows, per row; the batched calls on the whole matrix, per call
        ms = bd.DspMat(noise(np, LOOP_ROWS, 2 * POINTS, dtype), is_complex=True)
        ones = bd.DspVec(np.tile(np.array([1.0, 0.0], dtype), 16), is_complex=True)

        def loop(call):
            def run_loop():
                for r in range(LOOP_ROWS):
                    row = ms.get_row(r)
                    ok(call(row))
                    ok(ms.set_row(r, row))
            return burst_time(bd, run_loop, min_time=2 * WINDOW) / LOOP_ROWS
        rows_out = []
        rows_out.append(("multiply_complex_exponential", min(tm), loop(lambda row: row.multiply_complex_exponential(A, B))))
        rows_out.append(("reverse", burst_time(bd, lambda: ok(m.reverse())), loop(lambda row: row.reverse())))
        rows_out.append(("mul_smaller (16-point vector)", burst_time(bd, lambda: ok(m.mul_smaller(ones))),
                         loop(lambda row: row.mul_smaller(ones))))
        w("# %s: the batched call on %d rows, per call, beside the get_row -> DspVec call -> set_row loop on %d rows, per row" % (name, ROWS, LOOP_ROWS))
        w("%-8s %-32s %12s %14s" % ("", "call", "batched us", "loop us / row"))
        for what, tb, tl in rows_out:
            w("%-8s %-32s %12.1f %14.2f" % (name, what, tb * 1e6, tl * 1e6))
        del ms

        # log(10): the flat vector kernel under both; fresh data for every call
        master_m, master_v = m, v

        def fresh_m():
            f = bd.DspMat(rows=ROWS, row_len=2 * POINTS, is_complex=True, dtype=dtype)
            ok(f.add(master_m))
            return f

        def fresh_v():
            f = bd.DspVec(dtype=dtype, length=ROWS * 2 * POINTS, is_complex=True)
            ok(f.add(master_v))
            return f
        tlm = min(single_time(bd, fresh_m, lambda f: ok(f.log(10.0))) for _ in range(2))
        tlv = min(single_time(bd, fresh_v, lambda f: ok(f.log(10.0))) for _ in range(2))
        w("%-8s %-32s %12.1f %14s" % (name, "log(10), complex", tlm * 1e6, "vector call of the same size: %.1f us" % (tlv * 1e6)))
        del m, v, master_m, master_v
    w("# decision: the shared-phasor kernel stays only if it is faster than the vector kernel beyond the spread of the rounds")
    for name, ratio, spread in verdicts:
        faster = ratio > 1.0 + spread
        w("# %s: vector / matrix = %.2f, spread %.1f%% -> %s" % (name, ratio, spread * 100,
                                                               "k_mw_cexp is faster: kept" if faster else
                                                               "not faster beyond the spread: the flat ROWS variant of OpMulCexp is the simpler choice"))


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
