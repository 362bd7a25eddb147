"""Run by tests/test_gpu_launch_helper.py in a process of its own: the FIRST four library calls of a process, in an order
that a launcher which raises the dynamic-LDS limit of another instantiation than the one it launches cannot survive.

Three register-resident lengths whose workgroups need more than 64 KiB of LDS (k_mr_reg3, mixed_radix_reg3.h; f32 4000 =
20 20 10 is one of the five 512-thread lengths and has a plain-only instantiation besides the one with the fused options):

    1. inverse plain transform,    f32, 4000 points, batch 1   (plain-only instantiation, inverse, before any forward one)
    2. forward windowed transform, f32, 4000 points, batch 3   (option instantiation, forward)
    3. inverse plain transform,    f64, 2000 points, batch 1   (inverse before forward)
    4. forward shifted transform,  f64,  640 points, batch 2   (option path, forward)

Each goes through bdsp_hip_dev_fft on torch-owned memory, must return BDSP_OK (0) and is held to the oracle at the bound of
test_register_resident_three_stage_batches (tests/test_gpu_parity.py): rel-L2 1e-6 (f32) / 1e-12 (f64).  Prints one line
per call and "ok" last."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle_lib as orc  # noqa: E402

HAMMING, HAMMING_ORACLE, HAMMING_ALPHA = 1, 1, 0.54  # the facade's id, the oracle's id and its alpha

CALLS = (  # dtype, points, batch, inverse, what
    (np.float32, 4000, 1, True, "plain"),
    (np.float32, 4000, 3, False, "windowed"),
    (np.float64, 2000, 1, True, "plain"),
    (np.float64, 640, 2, False, "shifted"),
)


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def reference(row, inverse, what):
    row = row.astype(np.float64)
    if what == "windowed":
        row = orc.apply_window(row, True, HAMMING_ORACLE, HAMMING_ALPHA)
    out = orc.fft(row, inverse)
    return orc.swap_halves(out, True, True) if what == "shifted" else out


def main():
    import torch
    import basic_dsp_amd as bd
    L = bd._lib
    worst = 0.0
    for k, (dtype, n, batch, inverse, what) in enumerate(CALLS):
        x = orc.fill_uniform(2 * n * batch, 4100 + k, -10, 10, dtype).reshape(batch, 2 * n)
        d = torch.from_numpy(x).cuda()
        s = torch.empty_like(d)
        flags = (L.FFT_INVERSE if inverse else 0) | (L.FFT_SHIFT_OUT if what == "shifted" else 0)
        window = HAMMING if what == "windowed" else -1
        in_scratch = C.c_int(0)
        code = L.lib.bdsp_hip_dev_fft(0 if dtype == np.float32 else 1, d.data_ptr(), s.data_ptr(), n, batch, flags, 1.0, window,
                                      HAMMING_ALPHA if window >= 0 else 0.0, C.byref(in_scratch), L.torch_stream_arg())
        if code != 0:
            print("call %d returned %d: %s" % (k + 1, code, L.last_error()))
            return 1
        torch.cuda.synchronize()
        got = (s if in_scratch.value else d).cpu().numpy()
        tol = 1e-6 if dtype == np.float32 else 1e-12
        for r in range(batch):
            err = rel_l2(got[r], reference(x[r], inverse, what))
            worst = max(worst, err / tol)
            print("call %d %s %s %s n=%d row %d/%d: rel-L2 %.3e (bound %.0e)" % (k + 1, np.dtype(dtype).name, "inverse" if inverse else "forward",
                                                                                what, n, r, batch, err, tol))
            if not err < tol:
                print("call %d row %d misses the bound" % (k + 1, r))
                return 1
    print("ok (worst rel-L2 / bound %.3f)" % worst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
