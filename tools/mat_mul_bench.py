"""matmul (mat_mul.hip) on one MI355X beside torch.matmul on the same device, for the shapes
  (a) 8 x 8 x 2^20 plain          few channels -> few beams (memory-bound: 4 flop per byte in complex f32)
  (b) 64 x 64 x 2^20 plain        64 beams from 64 channels (32 flop per byte)
  (c) 256 x 256 x 65536 plain
  (d) 64 x 2^20 x 64 transposed   the covariance of 64 channels x 1M points
  (e) 256 x 65536 x 256 transposed
(M x K x N) in complex f32, and (b) and (d) in complex f64 as well -> profiles/mat_mul.txt.

  python tools/mat_mul_bench.py --out profiles/mat_mul.txt

Timing: device events around ONE call -- the library's on its own stream, torch's on torch's.  The call allocates its
result (from the library's block cache once warm), which is inside the window, as it is for a caller.  Every leg is warmed
and then repeated until the timed calls add up to at least 0.2 s (at most 2000 calls); a figure is the mean of a leg.  The
legs alternate torch, matmul, torch, matmul, torch: the torch leg's three repeats give the run-to-run spread (largest -
smallest) / smallest, and the smallest mean of each kind of leg is shown.

Derived columns: the path is mm_dispatch's rule (mat_mul_core.h), evaluated here from the constants of that header.
bytes = (M K + K N + M N) elements read or written once (the algorithmic bytes), flops = 8 M N K (a complex multiply-add
is 8 real operations); "of 8 TB/s" and "of peak" are those over the call time against 8.0 TB/s and against 157.3 TFLOP/s
(f32) or 78.6 TFLOP/s (f64, the vector rate).  No time is fixed in advance; where matmul is slower than torch the row says
so.  For the shapes with at most 2^20 outputs the two results are compared: max |ours - torch| / max |torch|.
"""
import argparse
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("a", 8, 8, 1 << 20, False), ("b", 64, 64, 1 << 20, False), ("c", 256, 256, 65536, False),
          ("d", 64, 1 << 20, 64, True), ("e", 256, 65536, 256, True))
F64_TOO = ("b", "d")
MIN_TIME = 0.2
MAX_CALLS = 2000
WARM = 3
PEAK_BYTES = 8.0e12
PEAK_FLOPS = {"float32": 157.3e12, "float64": 78.6e12}


def constants():
    with open(os.path.join(ROOT, "basic_dsp_amd", "csrc", "mat_mul_core.h")) as f:
        src = f.read()
    return {k: int(v) for k, v in re.findall(r"constexpr (?:size_t|int) (MM_[A-Z_]+) = (\d+);", src)}


def path_of(M, N, K, trans, c):
    tiles = -(-M // c["MM_TM"]) * -(-N // c["MM_TN"])
    if not trans and M <= c["MM_STREAM_MAX_M"] and K <= c["MM_STREAM_MAX_K"]:
        return "stream"
    if K >= c["MM_SPLIT_MIN_K"] and tiles <= c["MM_SPLIT_MAX_TILES"]:
        return "split"
    return "tiled"


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


def run(out):
    import numpy as np
    import torch
    import basic_dsp_amd as bd
    bd.require_gpu()
    lib = bd.lib
    consts = constants()
    e0, e1 = C.c_void_p(lib.bdsp_hip_event_create()), C.c_void_p(lib.bdsp_hip_event_create())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = C.c_float()
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# matmul (mat_mul.hip) on one MI355X: tools/mat_mul_bench.py.  Device events around one call; every leg warmed, calls")
    w("# adding up to >= %.1f s (at most %d); legs alternate torch, matmul, torch, matmul, torch.  Shown: the smallest mean of a" % (MIN_TIME, MAX_CALLS))
    w("# kind of leg; spread = (largest - smallest) / smallest of the three torch legs.  torch = torch.matmul on tensors of the")
    w("# same shape and dtype (a @ b, or x @ x.mH).  bytes = (M K + K N + M N) elements once; flops = 8 M N K; of 8 TB/s and of")
    w("# peak (157.3 TFLOP/s f32, 78.6 TFLOP/s f64): those over the call time.  Seeded normal data.")
    w("%-5s %-4s %-22s %-6s %-6s %10s %9s %8s %10s %7s %11s  %s" % ("shape", "kind", "M x K x N", "form", "path", "matmul us",
                                                                      "of 8TB/s", "of peak", "torch us", "spread", "mm / torch", "note"))
    rng = np.random.default_rng(20240607)
    for dtype in ("float32", "float64"):
        tdt = torch.complex64 if dtype == "float32" else torch.complex128
        cdt = np.complex64 if dtype == "float32" else np.complex128
        elem = np.dtype(dtype).itemsize * 2
        for name, M, K, N, trans in SHAPES:
            if dtype == "float64" and name not in F64_TOO:
                continue
            same = trans and M == N
            ha = rng.standard_normal((M, 2 * K), dtype=np.float32).astype(dtype)
            hb = ha if same else rng.standard_normal((N, 2 * K) if trans else (K, 2 * N), dtype=np.float32).astype(dtype)
            da = bd.DspMat(ha, is_complex=True)
            db = da if same else bd.DspMat(hb, is_complex=True)
            ta = torch.from_numpy(ha.view(cdt)).cuda()
            tb = ta if same else torch.from_numpy(hb.view(cdt)).cuda()
            del ha, hb

            def ours():
                ok(lib.bdsp_hip_event_record(e0, None))
                code, y = bd.matmul(da, db, conj_transpose=trans)
                ok(lib.bdsp_hip_event_record(e1, None))
                ok(code)
                ok(lib.bdsp_hip_synchronize(None))
                ok(lib.bdsp_hip_event_elapsed_ms(e0, e1, C.byref(ms)))
                del y
                return ms.value * 1e-3

            def theirs():
                t0.record()
                z = torch.matmul(ta, tb.mH if trans else tb)
                t1.record()
                torch.cuda.synchronize()
                del z
                return t0.elapsed_time(t1) * 1e-3

            tt, to = [], []
            tt.append(leg(theirs))
            to.append(leg(ours))
            tt.append(leg(theirs))
            to.append(leg(ours))
            tt.append(leg(theirs))
            spread = (max(tt) - min(tt)) / min(tt)
            tm, th = min(to), min(tt)
            note = "" if tm <= th * (1.0 + spread) else "SLOWER than torch"
            if M * N <= (1 << 20):
                code, y = bd.matmul(da, db, conj_transpose=trans)
                ok(code)
                mine = y.data().view(cdt)
                ref = torch.matmul(ta, tb.mH if trans else tb).cpu().numpy()
                note = (note + "; " if note else "") + "max |ours - torch| / max |torch| = %.1e" % (np.abs(mine - ref).max() / np.abs(ref).max())
                del y, mine, ref
            nbytes = (M * K + K * N + M * N) * elem
            flops = 8.0 * M * N * K
            w("%-5s %-4s %-22s %-6s %-6s %10.1f %8.1f%% %7.1f%% %10.1f %6.1f%% %11.2f  %s" % (
                "(%s)" % name, "c32" if dtype == "float32" else "c64", "%d x %d x %d" % (M, K, N), "trans" if trans else "plain",
                path_of(M, N, K, trans, consts), tm * 1e6, 100 * nbytes / tm / PEAK_BYTES, 100 * flops / tm / PEAK_FLOPS[dtype],
                th * 1e6, spread * 100, tm / th, note))
            del da, db, ta, tb
            torch.cuda.empty_cache()
    lib.bdsp_hip_event_destroy(e0)
    lib.bdsp_hip_event_destroy(e1)


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
