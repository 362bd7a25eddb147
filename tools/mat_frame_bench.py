"""The vector <-> matrix moves and the batched index moves of a matrix (mat_frame.hip), complex f32, on one MI355X:
  * DspMat.from_frames and DspMat.overlap_add of a 16M-point vector at (frame, hop) = (1024, 256) and (1024, 1024);
  * DspMat.from_vectors of 16 384 vectors of 1000 points;
  * DspMat.zero_pad 16 384 x 1000 -> 1024 and DspMat.swap_halves 16 384 x 1024, and the same two moves at rows = 1, for
    this build and for the parent commit's library (one launch per row there), alternating in one run
-> profiles/mat_frame.txt.

  tools/build_baseline.sh <parent commit>      # -> tools/lab/old_lib/libbasic_dsp_hip_B.so
  python tools/mat_frame_bench.py --out profiles/mat_frame.txt

Timing: every case is warmed; a figure is the mean over windows that add up to at least 0.3 s, each window ending in
one device synchronisation (the library's calls are asynchronous).  The new calls allocate their result, so their
figure includes the allocation and the release of the result, as a caller sees them.  zero_pad changes the shape, so
each of its calls gets a fresh matrix (made on the device, untimed) and a synchronisation of its own; swap_halves runs
in bursts on one matrix.  A process loads one library, chosen by BDSP_HIP_LIBRARY, and the parent commit's library
lacks the symbols the package binds on import, so the two builds run in worker processes of this tool that bind the
handful of entry points they need by hand -- one after the other, ROUNDS rounds each, alternating; the smallest mean
of a build's rounds is shown with their spread (largest - smallest) / smallest.  Beside every time of this build: the
bytes the move has to read and write once (algorithmic bytes) per second.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGNAL = 1 << 24
FRAMES = ((1024, 256), (1024, 1024))
ROWS, POINTS, PADDED = 16384, 1000, 1024
WINDOW = 0.3
BURST = 10
ROUNDS = 3
ELEM = 8  # bytes of a complex f32 point
BASELINE = os.path.join(ROOT, "tools", "lab", "old_lib", "libbasic_dsp_hip_B.so")


def sync(bd):
    bd.lib.bdsp_hip_synchronize(None)


def burst_time(bd, fn, burst=BURST, min_time=WINDOW):
    """mean seconds per call of fn over bursts of `burst` calls and one synchronisation"""
    for _ in range(3):
        fn()
    sync(bd)
    total, count = 0.0, 0
    while total < min_time:
        t0 = time.perf_counter()
        for _ in range(burst):
            fn()
        sync(bd)
        total += time.perf_counter() - t0
        count += burst
    return total / count


def ok(code):
    assert code == 0, code


def noise(np, scalars):
    tile = np.random.default_rng(scalars).uniform(-1.0, 1.0, min(scalars, 1 << 20)).astype(np.float32)
    return np.resize(tile, scalars)


class RawLib:
    """The few entry points the batched moves need, bound by hand: a worker also loads the parent commit's library,
    which lacks the symbols the package binds when it is imported."""

    def __init__(self, path):
        import ctypes as C
        self.C = C
        self.lib = lib = C.CDLL(path)
        P, SZ, I32 = C.c_void_p, C.c_size_t, C.c_int32
        for name, res, args in (("bdsp_hip_mat_new32", P, (I32, I32, SZ, SZ, C.c_float)), ("bdsp_hip_mat_delete32", None, (P,)),
                                ("bdsp_hip_mat_upload32", I32, (P, P, SZ)), ("bdsp_hip_mat_add32", I32, (P, P)),
                                ("bdsp_hip_mat_zero_pad32", I32, (P, SZ, I32)), ("bdsp_hip_mat_swap_halves32", I32, (P,)),
                                ("bdsp_hip_mat_row_points32", SZ, (P,)), ("bdsp_hip_synchronize", C.c_int, (P,)),
                                ("bdsp_hip_has_gpu_support_f32", C.c_int, ())):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, list(args)
        assert lib.bdsp_hip_has_gpu_support_f32(), "no GPU"

    def new(self, rows, points, data=None):
        m = self.lib.bdsp_hip_mat_new32(1, 0, rows, 2 * points, 1.0)
        assert m
        if data is not None:
            ok(self.lib.bdsp_hip_mat_upload32(m, data.ctypes.data_as(self.C.c_void_p), data.size))
        return m


def moves(raw, np):
    """the four figures a worker measures: zero_pad and swap_halves at ROWS rows and at one row"""
    lib = raw.lib
    sync = lambda: lib.bdsp_hip_synchronize(None)  # noqa: E731
    res = {}
    for rows in (ROWS, 1):
        master = raw.new(rows, POINTS, noise(np, rows * 2 * POINTS))
        # zero_pad changes the shape: a fresh copy of the master (made on the device, untimed) for every call
        total, count, warm = 0.0, 0, 3
        while total < WINDOW:
            f = raw.new(rows, POINTS)
            ok(lib.bdsp_hip_mat_add32(f, master))
            sync()
            t0 = time.perf_counter()
            ok(lib.bdsp_hip_mat_zero_pad32(f, PADDED, 0))
            sync()
            dt = time.perf_counter() - t0
            assert lib.bdsp_hip_mat_row_points32(f) == PADDED
            lib.bdsp_hip_mat_delete32(f)
            if warm:
                warm -= 1
                continue
            total += dt
            count += 1
        res["zero_pad %d" % rows] = total / count
        lib.bdsp_hip_mat_delete32(master)
        m = raw.new(rows, PADDED, noise(np, rows * 2 * PADDED))
        burst = BURST if rows > 1 else 10 * BURST
        for _ in range(3):
            ok(lib.bdsp_hip_mat_swap_halves32(m))
        sync()
        total, count = 0.0, 0
        while total < WINDOW:
            t0 = time.perf_counter()
            for _ in range(burst):
                ok(lib.bdsp_hip_mat_swap_halves32(m))
            sync()
            total += time.perf_counter() - t0
            count += burst
        res["swap_halves %d" % rows] = total / count
        lib.bdsp_hip_mat_delete32(m)
    return res


def worker():
    import numpy as np
    print("RESULT " + json.dumps(moves(RawLib(os.environ["BDSP_HIP_LIBRARY"]), np)), flush=True)


def run_worker(library):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=dict(os.environ, BDSP_HIP_LIBRARY=library),
                       capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError("worker failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    return json.loads(lines[-1][7:])


def run(out, baseline):
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# vector <-> matrix moves and batched index moves of a matrix (mat_frame.hip) on one MI355X: tools/mat_frame_bench.py.")
    w("# complex f32.  A figure: windows adding up to >= %.1f s, each ending in one device synchronisation, per call; every" % WINDOW)
    w("# case warmed.  from_frames, overlap_add and from_vectors allocate their result: allocation and release are in the")
    w("# figure.  GB/s = the bytes the move reads once and writes once (algorithmic bytes) over the time.")
    w("%-44s %12s %10s" % ("call", "us", "GB/s"))
    v = bd.DspVec(noise(np, 2 * SIGNAL), is_complex=True)
    for F, H in FRAMES:
        def frames():
            code, m = bd.DspMat.from_frames(v, F, H)
            ok(code)
            return m
        m = frames()
        rows = m.rows()
        t = burst_time(bd, frames, burst=2)
        nbytes = (SIGNAL + rows * F) * ELEM
        w("%-44s %12.1f %10.0f" % ("from_frames 16M points (%d, %d): %d rows" % (F, H, rows), t * 1e6, nbytes / t / 1e9))

        def ola():
            code, y = m.overlap_add(H)
            ok(code)
            return y
        n = ola().points()
        t = burst_time(bd, ola, burst=2)
        nbytes = (rows * F + n) * ELEM
        w("%-44s %12.1f %10.0f" % ("overlap_add %d x %d, hop %d: %d points" % (rows, F, H, n), t * 1e6, nbytes / t / 1e9))
        del m
    del v
    src = bd.DspMat(noise(np, ROWS * 2 * POINTS).reshape(ROWS, 2 * POINTS), is_complex=True)
    vs = [src.get_row(r) for r in range(ROWS)]
    del src

    def stack():
        code, m = bd.DspMat.from_vectors(vs)
        ok(code)
    t = burst_time(bd, stack, burst=2)
    w("%-44s %12.1f %10.0f" % ("from_vectors %d x %d points" % (ROWS, POINTS), t * 1e6, 2 * ROWS * POINTS * ELEM / t / 1e9))
    # the method builds a table of ROWS handles in Python on every call; the library call alone, the table built once:
    import ctypes as C
    table, handle = (C.c_void_p * ROWS)(*[v._h for v in vs]), C.c_void_p()

    def stack_c():
        ok(bd.lib.bdsp_hip_mat_from_vectors32(table, ROWS, C.byref(handle)))
        bd.lib.bdsp_hip_mat_delete32(handle)
    t = burst_time(bd, stack_c, burst=2)
    w("%-44s %12.1f %10.0f" % ("  bdsp_hip_mat_from_vectors32 alone", t * 1e6, 2 * ROWS * POINTS * ELEM / t / 1e9))
    del vs
    sync(bd)

    # the batched moves: this build and the parent commit's library, alternating, ROUNDS rounds each
    w("# zero_pad %d -> %d points (End) and swap_halves of %d points per row: this build (one launch) and the parent" % (POINTS, PADDED, PADDED))
    w("# commit's library (one launch per row), in worker processes that alternate, %d rounds each: smallest mean," % ROUNDS)
    w("# spread = (largest - smallest) / smallest of the rounds.")
    have_old = bool(baseline) and os.path.exists(baseline)
    new, old = [], []
    for _ in range(ROUNDS):
        new.append(run_worker(bd.LIB_PATH))
        if have_old:
            old.append(run_worker(baseline))
    algo = {"zero_pad": lambda rows: rows * (POINTS + PADDED) * ELEM, "swap_halves": lambda rows: 2 * rows * PADDED * ELEM}
    w("%-20s %12s %8s %10s %12s %8s %12s" % ("call", "new us", "spread", "new GB/s", "parent us", "spread", "parent / new"))
    verdicts = []
    for rows in (ROWS, 1):
        for name in ("zero_pad", "swap_halves"):
            key = "%s %d" % (name, rows)
            tn = [r[key] for r in new]
            sn = (max(tn) - min(tn)) / min(tn)
            line = "%-20s %12.1f %7.1f%% %10.1f" % ("%s, %d rows" % (name, rows), min(tn) * 1e6, sn * 100, algo[name](rows) / min(tn) / 1e9)
            if have_old:
                to = [r[key] for r in old]
                so = (max(to) - min(to)) / min(to)
                line += " %12.1f %7.1f%% %12.2f" % (min(to) * 1e6, so * 100, min(to) / min(tn))
                if rows == 1:
                    verdicts.append((name, min(tn), min(to), max(sn, so)))
            else:
                line += " %12s %8s %12s" % ("not measured", "", "")
            w(line)
    w("# condition: at rows = 1, where both builds launch once, this build is no slower than the parent beyond the larger")
    w("# spread of the two builds' rounds")
    if not have_old:
        w("# parent commit's library not found (tools/build_baseline.sh): not measured")
    for name, tn, to, spread in verdicts:
        w("# %s, 1 row: new / parent = %.3f, spread %.1f%% -> %s" % (name, tn / to, spread * 100,
                                                                  "holds" if tn <= to * (1.0 + spread) else "DOES NOT HOLD"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--baseline", default=BASELINE, help="the parent commit's library (tools/build_baseline.sh)")
    ap.add_argument("--worker", action="store_true", help="measure the batched moves of the library BDSP_HIP_LIBRARY names")
    a = ap.parse_args()
    if a.worker:
        worker()
        return
    lines = []
    run(lines, a.baseline)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
