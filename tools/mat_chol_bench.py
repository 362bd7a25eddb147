"""cholesky / cholesky_solve (mat_chol.hip) on one MI355X beside torch on the same device, a plain device copy and the
download - numpy - upload path they replace -> profiles/mat_chol.txt.

  (a) cholesky N = 64        (b) cholesky N = 256        (c) cholesky N = 1024                      complex f32
  (d) forward 64 x 2^20      complex f32: whitening of 64 channels x 1M samples, the hot path
  (e) forward 64 x 2^20      complex f64
  (f) forward 256 x 65536    complex f32
  (g) both 64 x 64           complex f32

  python tools/mat_chol_bench.py --out profiles/mat_chol.txt

Timing as in tools/mat_mul_bench.py: device events around ONE call -- the library's on its own stream, torch's on torch's;
the call allocates its result, which is inside the window.  Every leg is warmed and then repeated until the timed calls
add up to at least 0.2 s (at most 2000 calls); a figure is the mean of a leg.  The legs alternate torch, ours, torch,
ours, torch; the torch legs give the spread (largest - smallest) / smallest, and the smallest mean of each kind is shown.
torch = torch.linalg.cholesky / torch.linalg.solve_triangular (twice for "both"); if the build lacks either, the column
says absent, and if torch's call fails the column says so -- nothing is substituted.  copy = tensor.clone() of the
right-hand side's bytes (read once, written once).  host = download, numpy.linalg.cholesky / numpy.linalg.solve, upload:
wall-clock around the three steps, mean of 3; not run where N x P exceeds 2^24 elements (seconds per call).
No figure is a gate.  A row where ours is slower than torch is marked in bold (**...**).
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("a", "cholesky", 64, 0, "float32"), ("b", "cholesky", 256, 0, "float32"), ("c", "cholesky", 1024, 0, "float32"),
         ("d", "forward", 64, 1 << 20, "float32"), ("e", "forward", 64, 1 << 20, "float64"),
         ("f", "forward", 256, 65536, "float32"), ("g", "both", 64, 64, "float32"))
MIN_TIME = 0.2
MAX_CALLS = 2000
WARM = 3
PEAK_BYTES = 8.0e12


def ok(code):
    assert code == 0, code


def leg(timed_call):
    for _ in range(WARM):
        timed_call()
    total, count = 0.0, 0
    while total < MIN_TIME and count < MAX_CALLS:
        total += timed_call()
        count += 1
    return total / count


def run(out, only):
    import numpy as np
    import torch
    import basic_dsp_amd as bd
    bd.require_gpu()
    lib = bd.lib
    e0, e1 = C.c_void_p(lib.bdsp_hip_event_create()), C.c_void_p(lib.bdsp_hip_event_create())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = C.c_float()
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    has_chol = hasattr(torch.linalg, "cholesky")
    has_tri = hasattr(torch.linalg, "solve_triangular")
    w("# cholesky / cholesky_solve (mat_chol.hip) on one MI355X: tools/mat_chol_bench.py.  Device events around one call; every")
    w("# leg warmed, calls adding up to >= %.1f s (at most %d); legs alternate torch, ours, torch, ours, torch.  Shown: the smallest" % (MIN_TIME, MAX_CALLS))
    w("# mean of a kind of leg; spread of the torch legs.  copy: tensor.clone() of the right-hand side.  host: download, numpy,")
    w("# upload (wall clock).  of 8TB/s: (B read + X written) over the call time.  ** ours slower than torch **")
    w("%-5s %-9s %-4s %-14s %10s %9s %10s %7s %12s %10s %12s" % ("case", "call", "kind", "N x P", "ours us", "of 8TB/s", "torch us",
                                                                   "spread", "ours / torch", "copy us", "host us"))
    rng = np.random.default_rng(20240611)
    for name, what, N, P, dtype in CASES:
        if only and name not in only:
            continue
        tdt = torch.complex64 if dtype == "float32" else torch.complex128
        cdt = np.complex64 if dtype == "float32" else np.complex128
        elem = np.dtype(dtype).itemsize * 2
        G = (rng.standard_normal((N, 2 * N)) + 1j * rng.standard_normal((N, 2 * N)))
        A = (G @ G.conj().T / (2.0 * N) + 0.1 * np.eye(N)).astype(cdt)
        ha = np.ascontiguousarray(A).view(dtype)
        da = bd.DspMat(ha, is_complex=True)
        ta = torch.from_numpy(A).cuda()
        code, dl = bd.cholesky(da)
        ok(code)
        tl = torch.linalg.cholesky(ta) if has_chol else None
        db = tb = hb = None
        if what != "cholesky":
            hb = rng.standard_normal((N, 2 * P), dtype=np.float32).astype(dtype)
            db = bd.DspMat(hb, is_complex=True)
            tb = torch.from_numpy(hb.view(cdt)).cuda()

        def ours():
            ok(lib.bdsp_hip_event_record(e0, None))
            if what == "cholesky":
                code, y = bd.cholesky(da)
            else:
                code, y = bd.cholesky_solve(dl, db, part=what)
            ok(lib.bdsp_hip_event_record(e1, None))
            ok(code)
            ok(lib.bdsp_hip_synchronize(None))
            ok(lib.bdsp_hip_event_elapsed_ms(e0, e1, C.byref(ms)))
            del y
            return ms.value * 1e-3

        def theirs():
            t0.record()
            if what == "cholesky":
                z = torch.linalg.cholesky(ta)
            else:
                z = torch.linalg.solve_triangular(tl, tb, upper=False)
                if what == "both":
                    z = torch.linalg.solve_triangular(tl.mH, z, upper=True)
            t1.record()
            torch.cuda.synchronize()
            del z
            return t0.elapsed_time(t1) * 1e-3

        def copy():
            t0.record()
            z = tb.clone()
            t1.record()
            torch.cuda.synchronize()
            del z
            return t0.elapsed_time(t1) * 1e-3

        def host():
            t = time.perf_counter()
            if what == "cholesky":
                y = bd.DspMat(np.ascontiguousarray(np.linalg.cholesky(da.data().view(cdt))).view(dtype), is_complex=True)
            else:
                l = np.tril(dl.data().view(cdt))
                x = np.linalg.solve(l, db.data().view(cdt))
                if what == "both":
                    x = np.linalg.solve(l.conj().T, x)
                y = bd.DspMat(np.ascontiguousarray(x).view(dtype), is_complex=True)
            ok(lib.bdsp_hip_synchronize(None))
            del y
            return time.perf_counter() - t

        absent = (what == "cholesky" and not has_chol) or (what != "cholesky" and not (has_tri and has_chol))
        failed = ""
        tt, to = [], []
        if not absent:
            try:
                tt.append(leg(theirs))
            except RuntimeError as e:  # torch's own failure (its BLAS could not allocate, say): reported, nothing substituted
                absent, failed = True, "torch failed: " + str(e).split(" when calling")[0][:60]
        to.append(leg(ours))
        if not absent:
            tt.append(leg(theirs))
        to.append(leg(ours))
        if not absent:
            tt.append(leg(theirs))
        tm = min(to)
        tcopy = leg(copy) if (what != "cholesky" and P >= (1 << 16)) else None
        thost = sum(host() for _ in range(3)) / 3.0 if N * max(P, N) <= (1 << 24) else None
        nbytes = 2 * N * P * elem if what != "cholesky" else N * N * elem * 1.5
        if absent:
            tor, spr, rat = (failed or "absent"), "-", "-"
        else:
            th = min(tt)
            spread = (max(tt) - min(tt)) / min(tt)
            tor, spr = "%.1f" % (th * 1e6), "%.1f%%" % (spread * 100)
            rat = "%.2f" % (tm / th)
            if tm > th * (1.0 + spread):
                rat = "**%s**" % rat
        w("%-5s %-9s %-4s %-14s %10.1f %8.1f%% %10s %7s %12s %10s %12s" % (
            "(%s)" % name, what, "c32" if dtype == "float32" else "c64", "%d x %d" % (N, P if what != "cholesky" else N), tm * 1e6,
            100 * nbytes / tm / PEAK_BYTES, tor, spr, rat, "-" if tcopy is None else "%.1f" % (tcopy * 1e6),
            "-" if thost is None else "%.1f" % (thost * 1e6)))
        del da, dl, db, ta, tb, tl
        torch.cuda.empty_cache()
    lib.bdsp_hip_event_destroy(e0)
    lib.bdsp_hip_event_destroy(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", default="", help="case letters, e.g. adg")
    a = ap.parse_args()
    lines = []
    run(lines, a.only)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
