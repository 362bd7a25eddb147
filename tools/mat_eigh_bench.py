"""eigh (mat_eigh.hip) on one MI355X beside torch.linalg.eigh on the same device and the download - numpy - upload path it
replaces -> profiles/mat_eigh.txt.

  N = 8, 64, 256, 1024 in complex f32 (a .. d) and complex f64 (e .. h); A = G G^H / 2N + 0.1 I, G random N x 2N

  python tools/mat_eigh_bench.py --out profiles/mat_eigh.txt

Timing as in tools/mat_chol_bench.py: device events around ONE call -- the library's on its own stream, torch's on torch's;
the call allocates its results and reads its status back (once for N <= 64, once per sweep above), all of which is inside
the window.  Every leg is warmed and then repeated until the timed calls add up to at least 0.2 s (at most 2000 calls); a
figure is the mean of a leg.  The legs alternate torch, ours, torch, ours, torch; the torch legs give the spread
(largest - smallest) / smallest, and the smallest mean of each kind is shown.  If torch's call fails the column says so --
nothing is substituted.  host = download, numpy.linalg.eigh, upload of w and v: wall-clock around the three steps, mean of
3.  sweeps and launches are those of the call (je_launches of mat_eigh_core.h: 1 for N <= 64, else 3 + 3 sweeps times the
block steps of a sweep).  No figure is a gate.  A row where ours is slower than torch is marked in bold (**...**).
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("a", 8, "float32"), ("b", 64, "float32"), ("c", 256, "float32"), ("d", 1024, "float32"),
         ("e", 8, "float64"), ("f", 64, "float64"), ("g", 256, "float64"), ("h", 1024, "float64"))
MIN_TIME = 0.2
MAX_CALLS = 2000
WARM = 2


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


def launches(N, sweeps):
    if N <= 64:
        return 1
    nb = (N + 31) // 32
    return 3 + sweeps * 3 * (nb if nb % 2 else nb - 1)


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
    w("# eigh (mat_eigh.hip) on one MI355X: tools/mat_eigh_bench.py.  Device events around one call; every leg warmed, calls")
    w("# adding up to >= %.1f s (at most %d); legs alternate torch, ours, torch, ours, torch.  Shown: the smallest mean of a kind" % (MIN_TIME, MAX_CALLS))
    w("# of leg; spread of the torch legs.  host: download, numpy.linalg.eigh, upload (wall clock).  ** ours slower than torch **")
    w("%-5s %-4s %-12s %12s %7s %9s %12s %7s %12s %12s" % ("case", "kind", "N", "ours us", "sweeps", "launches", "torch us", "spread",
                                                          "ours / torch", "host us"))
    rng = np.random.default_rng(20240612)
    for name, N, dtype in CASES:
        if only and name not in only:
            continue
        cdt = np.complex64 if dtype == "float32" else np.complex128
        G = (rng.standard_normal((N, 2 * N)) + 1j * rng.standard_normal((N, 2 * N)))
        A = (G @ G.conj().T / (2.0 * N) + 0.1 * np.eye(N)).astype(cdt)
        da = bd.DspMat(np.ascontiguousarray(A).view(dtype), is_complex=True)
        ta = torch.from_numpy(A).cuda()
        code, _, _, sweeps = bd.eigh(da, return_sweeps=True)
        ok(code)

        def ours():
            ok(lib.bdsp_hip_event_record(e0, None))
            code, y, z = bd.eigh(da)
            ok(lib.bdsp_hip_event_record(e1, None))
            ok(code)
            ok(lib.bdsp_hip_synchronize(None))
            ok(lib.bdsp_hip_event_elapsed_ms(e0, e1, C.byref(ms)))
            del y, z
            return ms.value * 1e-3

        def theirs():
            t0.record()
            z = torch.linalg.eigh(ta)
            t1.record()
            torch.cuda.synchronize()
            del z
            return t0.elapsed_time(t1) * 1e-3

        def host():
            t = time.perf_counter()
            lam, vec = np.linalg.eigh(da.data().view(cdt))
            y = bd.DspMat(np.ascontiguousarray(lam.astype(dtype))[None, :], is_complex=False)
            z = bd.DspMat(np.ascontiguousarray(vec.conj().T).view(dtype), is_complex=True)
            ok(lib.bdsp_hip_synchronize(None))
            del y, z
            return time.perf_counter() - t

        failed = ""
        tt, to = [], []
        try:
            tt.append(leg(theirs))
        except RuntimeError as e:  # torch's own failure: reported, nothing substituted
            failed = "torch failed: " + str(e).split(" when calling")[0][:60]
        to.append(leg(ours))
        if not failed:
            tt.append(leg(theirs))
        to.append(leg(ours))
        if not failed:
            tt.append(leg(theirs))
        tm = min(to)
        thost = sum(host() for _ in range(3)) / 3.0
        if failed:
            tor, spr, rat = failed, "-", "-"
        else:
            th = min(tt)
            spread = (max(tt) - min(tt)) / min(tt)
            tor, spr = "%.1f" % (th * 1e6), "%.1f%%" % (spread * 100)
            rat = "%.2f" % (tm / th)
            if tm > th * (1.0 + spread):
                rat = "**%s**" % rat
        w("%-5s %-4s %-12s %12.1f %7d %9d %12s %7s %12s %12.1f" % (
            "(%s)" % name, "c32" if dtype == "float32" else "c64", "%d x %d" % (N, N), tm * 1e6, sweeps, launches(N, sweeps), tor, spr,
            rat, thost * 1e6))
        del da, ta
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
