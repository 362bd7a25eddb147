"""GPU tests (-m gpu) of the routes through the block convolution kernel (k_overlap_save_v2) that the parity suite
leaves alone: the prepared spectrum with the delay applied as a phase, for every R0 and in both precisions; the per-call
dispatch-group shares, which must not change a bit of the result; partial runs (first_block / nblocks, the pipelined
gpu_convolve_vector) in f64; batched real rows with a short last block and an odd number of real blocks.  The tap counts
and the share overrides come from tests/conv_v2_shapes.txt, which the host simulation (tests/test_conv_v2_abi.py) reads
too.

Oracle: orc.convolve_direct in f64, on the whole vector where n <= 3 * 4096, else on three windows of 300 points (both
ends and the middle).  Tolerances: tol_for(dtype), rel-L2 1e-6 (f32) / 1e-12 (f64), as in test_gpu_parity.py."""
import functools

import numpy as np
import pytest

import oracle_lib as orc
from test_conv_v2_abi import read_shapes

pytestmark = pytest.mark.gpu

bd = pytest.importorskip("basic_dsp_amd")
from basic_dsp_amd import DspMat, DspVec  # noqa: E402
from basic_dsp_amd import vector as V  # noqa: E402

TAPS, _, SHARES = read_shapes()
ELEM = {np.float32: 0, np.float64: 1}  # include/basic_dsp_hip.h: `elem` = 0 for f32, 1 for f64
BLOCK = 4096


def rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300)


def tol_for(dtype):   # test_gpu_parity.py: rel-L2 of one f32 / f64 convolution against the f64 oracle
    return 1e-6 if dtype == np.float32 else 1e-12


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == np.float32 else torch.float64


def _windows(n):
    """(first, count) pieces of a vector of n points that the oracle computes."""
    if n <= 3 * BLOCK:
        return [(0, n)]
    return [(0, 300), (n // 2 - 150, 300), (n - 300, 300)]


def _check_against_oracle(got, x, h, cplx, tol, what):
    e = 2 if cplx else 1
    n = x.size // e
    for first, count in _windows(n):
        ref = orc.convolve_direct(x.astype(np.float64), h.astype(np.float64), cplx, first, count)
        err = rel_l2(got[e * first: e * (first + count)], ref)
        assert err < tol, (what, first, err)


# ------------------------------------------------------------------ prepared spectrum, every R0, both precisions
PREP_N, PREP_BATCH = 2 * BLOCK + 17, 2


@functools.lru_cache(maxsize=None)
def _prepared_case(taps):
    """Rows, filter and oracle result of one tap count; f32 values, so both precisions share them."""
    rows = np.stack([orc.fill_uniform(2 * PREP_N, 41 + r + taps, -10, 10, np.float32) for r in range(PREP_BATCH)])
    h = orc.fill_uniform(2 * taps, 91 + taps, -1, 1, np.float32) / np.float32(taps)
    ref = np.stack([orc.convolve_direct(r.astype(np.float64), h.astype(np.float64), True) for r in rows])
    for a in (rows, h, ref):
        a.setflags(write=False)
    return rows, h, ref


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r0", range(1, 13))
def test_prepared_spectrum_every_r0(r0, dtype):
    """bdsp_hip_dev_conv_prepare + bdsp_hip_dev_convolve_prepared: the kernel's hs_is_taps == 0 branch delays the spectrum
    by the phase wtab[(k d) & 4095].  For every R0 the tap counts with d = 0 and d = 255; the spectrum buffer is reused
    for the two tap vectors in turn.  Against the oracle, and against bdsp_hip_dev_convolve on the same data.
    Measured on MI355X, worst over all R0: prepared 2.4e-7 (f32) / 1.8e-15 (f64), prepared against taps 2.3e-7 / 4.8e-16."""
    import torch
    lib, sp, elem, tol = bd.lib, bd._lib.torch_stream_arg(), ELEM[dtype], tol_for(dtype)
    mine = [(m, d) for m, r, d in TAPS if r == r0 and m in (256 * r0 + 1, 256 * (r0 - 1) + 2)]
    assert sorted(d for _, d in mine) == [0, 255]
    spec = torch.full((2 * lib.bdsp_hip_conv_spectrum_points(),), float("nan"), device="cuda", dtype=_torch_dtype(dtype))
    for taps, d in mine:
        rows, h, ref = _prepared_case(taps)
        dx, dh = torch.from_numpy(rows.astype(dtype)).cuda(), torch.from_numpy(h.astype(dtype)).cuda()
        dy = torch.full_like(dx, float("nan"))
        assert lib.bdsp_hip_dev_conv_prepare(elem, dh.data_ptr(), taps, spec.data_ptr(), sp) == 0
        assert lib.bdsp_hip_dev_convolve_prepared(elem, dx.data_ptr(), dy.data_ptr(), PREP_N, PREP_BATCH, spec.data_ptr(), taps, sp) == 0
        got = dy.cpu().numpy()
        dy.fill_(float("nan"))
        assert lib.bdsp_hip_dev_convolve(elem, dx.data_ptr(), dy.data_ptr(), PREP_N, PREP_BATCH, dh.data_ptr(), taps, sp) == 0
        plain = dy.cpu().numpy()
        for r in range(PREP_BATCH):
            e_prep, e_plain, e_both = rel_l2(got[r], ref[r]), rel_l2(plain[r], ref[r]), rel_l2(got[r], plain[r])
            print("R0 %d taps %d d %d row %d %s: prepared %.3e, taps %.3e, prepared vs taps %.3e" % (r0, taps, d, r, dtype.__name__, e_prep, e_plain, e_both))
            assert e_prep < tol and e_plain < tol and e_both < tol, (taps, r, e_prep, e_plain, e_both)


# ------------------------------------------------------------------ results do not depend on the shares
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("batch", [1, 64])
def test_result_does_not_depend_on_the_shares(batch, dtype):
    """bdsp_hip_dev_convolve_ex moves blocks between workgroups and nothing else: with every override of
    tests/conv_v2_shapes.txt the output is bit-identical to the default call's.  n = 30 V + 5 at 1024 taps: one vector
    is a shrunk grid of at most 3 rounds, 64 vectors are about 2.5 rounds of a full grid at 256 CUs.  The output
    buffer is NaN before each call, so a block nobody took shows."""
    import torch
    lib, sp, elem = bd.lib, bd._lib.torch_stream_arg(), ELEM[dtype]
    taps = 1024
    n = 30 * (BLOCK - 256 * 4) + 5
    g = torch.Generator(device="cuda")
    g.manual_seed(11 + batch)
    dx = torch.rand((batch, 2 * n), generator=g, device="cuda", dtype=_torch_dtype(dtype)) * 20 - 10
    dh = (torch.rand(2 * taps, generator=g, device="cuda", dtype=_torch_dtype(dtype)) * 2 - 1) / taps
    dy = torch.full_like(dx, float("nan"))
    assert lib.bdsp_hip_dev_convolve(elem, dx.data_ptr(), dy.data_ptr(), n, batch, dh.data_ptr(), taps, sp) == 0
    want = dy.cpu().numpy()
    assert not np.isnan(want).any()
    h = dh.cpu().numpy()
    for r in sorted({0, batch // 2, batch - 1}):
        _check_against_oracle(want[r], dx[r].cpu().numpy(), h, True, tol_for(dtype), ("default", batch, r))
    assert len(SHARES) == 4
    for first, second in [(-1, -1)] + SHARES:
        dy.fill_(float("nan"))
        assert lib.bdsp_hip_dev_convolve_ex(elem, dx.data_ptr(), dy.data_ptr(), n, batch, dh.data_ptr(), taps, first, second, sp) == 0
        assert np.array_equal(dy.cpu().numpy(), want), (first, second)


# ------------------------------------------------------------------ partial runs in f64
@pytest.mark.parametrize("n,m", [((1 << 20) + 12345, 257), ((1 << 20) + 5, 2500)])
def test_pipelined_convolve_vector_f64(n, m):
    """Above 2^20 complex points gpu_convolve_vector runs the blocks in chunks (first_block / nblocks): in f64 too the
    result equals the device-resident path bit for bit, and the oracle on three windows."""
    x = orc.fill_uniform(2 * n, 77 + n, -10, 10, np.float64)
    h = orc.fill_uniform(2 * m, 78, -1, 1, np.float64) / m
    y, rng = V.gpu_convolve_vector(x, h, True)
    assert rng == (0, 2 * n)
    v = DspVec(x, is_complex=True)
    assert v.convolve_signal(DspVec(h, is_complex=True)) == 0
    assert np.array_equal(y, v.data()), (n, m)
    _check_against_oracle(y, x, h, True, tol_for(np.float64), (n, m))


# ------------------------------------------------------------------ batched real rows
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("blocks", [3, 2])
def test_matrix_convolve_signal_real_rows_with_a_short_last_block(blocks, rows, dtype):
    """DspMat.convolve_signal on real rows: pairs of real blocks, batched.  At 200 taps (V = 3840) n = 3 V + 1 is four real
    blocks in two pairs per row, the last block of one sample; n = 2 V + 1 is three real blocks, so the last pair is half
    empty.  Every row against its own oracle.
    (test_matrix_batched_ops_equal_per_row_vector_ops has real rows of 2048 and 1001 points at 33 taps: one block.)"""
    taps = 200
    n = blocks * (BLOCK - 256) + 1
    a = np.stack([orc.fill_uniform(n, 300 + r + n, -10, 10, dtype) for r in range(rows)])
    h = orc.fill_uniform(taps, 9, -1, 1, dtype) / dtype(taps)
    m = DspMat(a, is_complex=False)
    assert m.convolve_signal(DspVec(h)) == 0 and not m.is_complex()
    got = m.data()
    assert got.shape == a.shape
    for r in range(rows):
        ref = orc.convolve_direct(a[r].astype(np.float64), h.astype(np.float64), False)
        err = rel_l2(got[r], ref)
        print("real rows %d row %d %s: %.3e" % (rows, r, dtype.__name__, err))
        assert err < tol_for(dtype), (rows, r, err)
