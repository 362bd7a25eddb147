"""Time-domain convolution of the rows of a matrix with an impulse-response function (DspMat.convolve, mat_interp.hip):
the direct kernel against the batched block convolution at 9 .. 257 taps -> the crossover MAT_CONV_DIRECT_MAX_TAPS
(capi.cpp); the get_row -> vector call -> set_row loop for comparison; the call times of interpolate_lin and
interpolate_hermite -> profiles/mat_interp.txt.

  python tools/mat_interp_bench.py --out profiles/mat_interp.txt

Timing: every case is warmed; a figure is the mean over windows that add up to at least 0.3 s, each window a burst of
BURST calls on the same matrix and one device synchronisation (the library's calls are asynchronous), divided by BURST.
convolve leaves the row length alone, so a burst runs on one matrix; between windows its values are scaled back by the
sum of the weights, untimed.  The two paths are forced through bdsp_hip_mat_convolve_ex and
alternate in one process, two rounds each; the smaller mean is shown.  An interpolation changes the row length, so each
of its calls gets a fresh matrix (copied on the device, untimed) and the figure includes growing the matrix's buffers, as
a user's first call does.  The row loop is timed on LOOP_ROWS rows and reported per row.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOOP_ROWS = 256
WINDOW = 0.3
BURST = 10
TAPS = (9, 17, 33, 65, 129, 257)
SHAPES = ((16384, 1000), (256, 65536))  # rows x complex f32 points
RATIO = 0.25
SINC = 0
BLOCK, DIRECT = 0, 1


def sync(bd):
    bd.lib.bdsp_hip_synchronize(None)


def burst_time(bd, fn, after, min_time=WINDOW):
    """mean seconds per call of fn over bursts of BURST calls; after() runs untimed between the windows"""
    for _ in range(3):
        fn()
    after(3)
    sync(bd)
    total, count = 0.0, 0
    while total < min_time:
        t0 = time.perf_counter()
        for _ in range(BURST):
            fn()
        sync(bd)
        total += time.perf_counter() - t0
        count += BURST
        after(BURST)
        sync(bd)
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
    tile = rng.uniform(-1.0, 1.0, (min(rows, 512), width))
    return np.ascontiguousarray(np.resize(tile, (rows, width))).astype(dtype)


def conv_gain(np, L):
    """what one convolve call multiplies a constant row by: the sum of the 2L + 1 weights"""
    return float(sum(np.sinc(RATIO * k) for k in range(-L, L + 1)))


def run(out):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# convolve(function) and interpolate_lin / interpolate_hermite of the rows of a matrix (mat_interp.hip) on one MI355X:")
    w("# tools/mat_interp_bench.py.  direct = k_mt_conv_direct, block = the batched 4096-point block convolution, both forced")
    w("# through bdsp_hip_mat_convolve_ex on the same matrix, alternating in one process, two rounds each, the smaller mean")
    w("# shown.  A figure: bursts of %d calls and one device synchronisation per window, windows adding up to >= %.1f s," % (BURST, WINDOW))
    w("# per call; every case warmed.  The call includes the launch that tabulates the weights.")
    w("%-28s %5s %11s %10s %8s" % ("complex f32 rows x points", "taps", "direct us", "block us", "faster"))
    faster_at = {t: [] for t in TAPS}
    for rows, points in SHAPES:
        m = bd.DspMat(noise(np, rows, 2 * points, np.float32), is_complex=True)
        for taps in TAPS:
            L = (taps - 1) // 2
            gain = conv_gain(np, L)

            def call(path):
                code = bd.lib.bdsp_hip_mat_convolve_ex32(m._h, SINC, 0.0, RATIO, L, path)
                assert code == 0, (taps, path, code)

            def after(n):
                assert m.scale(gain ** -n) == 0
            t = {BLOCK: [], DIRECT: []}
            for _ in range(2):
                for path in (DIRECT, BLOCK):
                    t[path].append(burst_time(bd, lambda: call(path), after))
            d, b = min(t[DIRECT]), min(t[BLOCK])
            faster_at[taps].append(d < b)
            w("%-28s %5d %11.1f %10.1f %8s" % ("%d x %d" % (rows, points), taps, d * 1e6, b * 1e6, "direct" if d < b else "block"))
        del m
    best = [t for t in TAPS if all(faster_at[t])]
    ok = [t for t in best if all(all(faster_at[u]) for u in TAPS if u <= t)]
    w("# crossover: the largest of these tap counts at which the direct kernel is faster at both shapes (and at every smaller")
    w("# count): %s" % (max(ok) if ok else "none"))

    w("# the row loop: get_row -> DspVec.convolve -> set_row, %d rows, 25 taps, per row; beside DspMat.convolve on the" % LOOP_ROWS)
    w("# same rows, per call")
    w("%-28s %14s %14s" % ("complex f32 rows x points", "loop us / row", "batched us"))
    for _, points in SHAPES:
        m = bd.DspMat(noise(np, LOOP_ROWS, 2 * points, np.float32), is_complex=True)

        def loop():
            for r in range(LOOP_ROWS):
                v = m.get_row(r)
                assert v.convolve(SINC, RATIO, 12) == 0
                assert m.set_row(r, v) == 0
        after = lambda n: m.scale(conv_gain(np, 12) ** -n)  # noqa: E731
        tl = burst_time(bd, loop, after, min_time=2 * WINDOW) / LOOP_ROWS
        tb = burst_time(bd, lambda: m.convolve(SINC, RATIO, 12), after)
        w("%-28s %14.2f %14.1f" % ("%d x %d" % (LOOP_ROWS, points), tl * 1e6, tb * 1e6))
        del m

    w("# interpolate_lin / interpolate_hermite, factor 2.5, real f32 rows: one call on a fresh matrix (copied on the device,")
    w("# untimed) and a device synchronisation per window; the call grows the matrix's buffers to the new row length")
    w("%-28s %-20s %10s %12s" % ("real f32 rows x points", "call", "call us", "loop us/row"))
    for rows, points in SHAPES:
        x = noise(np, rows, points, np.float32)
        master, smaster = bd.DspMat(x), bd.DspMat(x[:LOOP_ROWS])
        del x

        def fresh(src, r):
            f = bd.DspMat(rows=r, row_len=points, dtype=np.float32)
            f.add(src)
            return f
        for name in ("interpolate_lin", "interpolate_hermite"):
            def call(mm):
                assert getattr(mm, name)(2.5) == 0

            def loop(ms):
                probe = ms.get_row(0)
                call(probe)
                dst = bd.DspMat(rows=LOOP_ROWS, row_len=len(probe), dtype=np.float32)
                for r in range(LOOP_ROWS):
                    v = ms.get_row(r)
                    call(v)
                    assert dst.set_row(r, v) == 0, (len(v), dst.row_len())
            tb = min(single_time(bd, lambda: fresh(master, rows), call) for _ in range(2))
            tl = single_time(bd, lambda: fresh(smaster, LOOP_ROWS), loop) / LOOP_ROWS
            w("%-28s %-20s %10.1f %12.2f" % ("%d x %d" % (rows, points), name, tb * 1e6, tl * 1e6))
        del master, smaster


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
