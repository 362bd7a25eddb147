"""A vector is a matrix of one row: DspVec's swap_halves / fft_shift / ifft_shift, zero_pad, reverse, mirror, cum_sum,
unwrap and *_smaller launch the matrix kernels with one row, so a matrix row compared with the vector call no longer
checks two implementations there (diff / diff_with_start and multiply_complex_exponential keep a vector kernel, which
measured faster for one long row).  This file holds the vector's independent references for all nine operations at the
shapes where a one-row launch of a row-carrying kernel can go wrong:
  * points 1, 2, 3, 255, 256, 257, 511, 512, 513: the lane groups of the short-row scan end at MS_SCAN_SHORT = 512, a
    workgroup's tile of the mixer at 256;
  * SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1: one workgroup per row ends and the three-step scan begins;
  * L + 1 and 2 L + 3, L = compute units x 8 x 256 = one grid stride of the flat kernels: above it a lane carries its
    (row, position) over a stride that is longer than the row, and the last lanes run one trip fewer.
Real and complex data, f32 and f64.  A vector owns its (aligned) device buffer, so the only offset the API allows is the
host array's: every upload comes from an address that is not 16-byte aligned.

References and bounds:
  * the movers against tests/vec_model.py (VecModel, index arithmetic only) and diff against oracle_lib: bit-equal;
  * unwrap (a sequential recurrence) and *_smaller (one rounding per operation) against oracle_lib: bit-equal, as in
    tests/test_gpu_parity.py; operand lengths 1, points / 3 (where 3 divides points) and points;
  * cum_sum with test_gpu_parity's bound: max |got - prefix sum| / (max |prefix sum| + 1) < 2e-7 (f32), 1e-13 (f64),
    and oracle_lib's sequential sum in T within its own error bound of that prefix sum;
  * multiply_complex_exponential with test_gpu_parity's bounds: rel-L2 < 2e-7 (f32), 1e-14 (f64) against the exact
    phasor exp(j (a k + b)) in double, and against oracle_lib's running product < 5e-5 (f32), 1e-11 (f64) for up to
    3000 points.  The running product's own error grows with the index (measured against the exact phasor on the CPU:
    1.6e-5 at 3000 points, 2.6e-3 at 524289, 5.3e-3 at 1048579 in f32; 2.6e-14, 4.4e-12, 8.7e-12 in f64 -- linear in
    the length), so above 3000 points that bound grows by points / 3000, which keeps test_gpu_parity's margin over the
    reference's own error.
"""
import numpy as np
import pytest

import oracle_lib as orc
from vec_model import PAD_CENTER, PAD_END, PAD_SURROUND, VecModel

pytestmark = pytest.mark.gpu

bd = pytest.importorskip("basic_dsp_amd")
from basic_dsp_amd import DspVec  # noqa: E402
from basic_dsp_amd import vector as V  # noqa: E402

MS_SCAN_SHORT = 512    # mat_scan.hip
SCAN_CHUNK = 4096      # mat_scan_core.h
FLAT_WG, FLAT_WG_PER_CU = 256, 8   # mf_grid / mw_grid / sy_grid: at most 8 workgroups of 256 lanes per compute unit


def _shapes():
    cus = bd.lib.bdsp_hip_compute_units()
    assert cus > 0, bd.last_error()
    stride = cus * FLAT_WG_PER_CU * FLAT_WG
    return [1, 2, 3, 255, 256, 257, MS_SCAN_SHORT - 1, MS_SCAN_SHORT, MS_SCAN_SHORT + 1, SCAN_CHUNK - 1, SCAN_CHUNK,
            SCAN_CHUNK + 1, stride + 1, 2 * stride + 3]


_CACHE = {}


def unaligned(a):
    """a copy of `a` whose first byte is not 16-byte aligned (one scalar into a fresh buffer)"""
    a = np.asarray(a)
    buf = np.empty(a.size + 5, a.dtype)
    start = next(k for k in range(1, 5) if (buf.ctypes.data + k * a.itemsize) % 16)
    out = buf[start:start + a.size]
    out[:] = a
    assert out.ctypes.data % 16 != 0
    return out


def signal(points, cplx, dtype, seed=0):
    """the shared, read-only input of one (points, number space, precision): computed once"""
    key = (points, cplx, np.dtype(dtype).name, seed)
    if key not in _CACHE:
        x = unaligned(orc.fill_uniform(points * (2 if cplx else 1), 20261019 + 7 * seed + points % 1000, -10, 10, dtype))
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(bits(got), bits(ref))


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300)


CASES = [(c, d) for c in (False, True) for d in (np.float32, np.float64)]
IDS = ["%s-%s" % ("complex" if c else "real", np.dtype(d).name) for c, d in CASES]


@pytest.fixture(scope="module")
def shapes():
    bd.require_gpu()
    return _shapes()


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_movers_bit_equal_to_the_model(shapes, cplx, dtype):
    """swap_halves, fft_shift, ifft_shift, reverse, zero_pad (End, Surround, Center; to one point more and to 2 p + 3)
    and mirror: code, length and every bit as VecModel's gather"""
    for p in shapes:
        x = signal(p, cplx, dtype)
        steps = [("swap_halves", ()), ("fft_shift", ()), ("ifft_shift", ()), ("reverse", ())]
        steps += [("zero_pad", (q, o)) for q in (p + 1, 2 * p + 3) for o in (PAD_END, PAD_SURROUND, PAD_CENTER)]
        if cplx:
            steps.append(("mirror", ()))
        for name, args in steps:
            v = DspVec(x, is_complex=cplx, domain=V.FREQ)
            m = VecModel(x, is_complex=cplx, domain=V.FREQ)
            assert getattr(v, name)(*args) == getattr(m, name)(*args) == 0, (name, args, p)
            assert len(v) == len(m) and v.is_complex() == m.is_complex(), (name, args, p)
            assert same_bits(v.data(), m.data()), (name, args, p)
        # two movers in a row: the second reads what the first left in the trade buffer
        v, m = DspVec(x, is_complex=cplx), VecModel(x, is_complex=cplx)
        assert v.reverse() == m.reverse() == 0 and v.ifft_shift() == m.ifft_shift() == 0
        assert same_bits(v.data(), m.data()), p


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_diff_bit_equal_to_the_oracle(shapes, cplx, dtype):
    e = 2 if cplx else 1
    for p in shapes:
        x = signal(p, cplx, dtype)
        for with_start in (False, True):
            v = DspVec(x, is_complex=cplx)
            assert (v.diff_with_start() if with_start else v.diff()) == 0
            ref = orc.diff(np.array(x), cplx, with_start)
            assert len(v) == ref.size == (p if with_start else p - 1) * e, (p, with_start)
            assert same_bits(v.data(), ref), (p, with_start)


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_cum_sum_against_the_prefix_sum(shapes, cplx, dtype):
    e = 2 if cplx else 1
    for p in shapes:
        x = signal(p, cplx, dtype)
        v = DspVec(x, is_complex=cplx)
        assert v.cum_sum() == 0 and len(v) == p * e
        # the prefix sum in extended precision: at 10^6 points a sequential f64 sum's own error is no longer far below 1e-13
        ref = np.cumsum(x.astype(np.longdouble).reshape(-1, e), axis=0).reshape(-1)
        scale = np.max(np.abs(ref)) + 1.0
        err = np.max(np.abs(v.data() - ref)) / scale
        assert err < (2e-7 if dtype == np.float32 else 1e-13), (p, err)
        seq = orc.cum_sum(np.array(x), cplx)
        assert np.max(np.abs(seq - ref)) / scale < (p * 1e-7 if dtype == np.float32 else p * 1e-16), p


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_unwrap_bit_equal_to_the_oracle(shapes, dtype):
    """a phase ramp wrapped into (-pi, pi] (every tile carries the previous tile's unwrapped end) and random data with
    a divisor that makes most steps take the remainder; a complex vector is poisoned"""
    for p in shapes:
        ramp = unaligned(np.angle(np.exp(1j * np.arange(p, dtype=np.float64) * 0.37)).astype(dtype))
        for data, div in ((ramp, 2 * np.pi), (signal(p, False, dtype, seed=1), 7.0)):
            v = DspVec(data)
            assert v.unwrap(dtype(div)) == 0 and len(v) == p
            assert same_bits(v.data(), orc.unwrap(np.array(data), dtype(div))), (p, div)
    c = DspVec(signal(3, True, dtype), is_complex=True)
    assert c.unwrap(dtype(1.0)) == -1 and c.is_erroneous()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_multiply_complex_exponential_against_the_exact_phasor_and_the_oracle(shapes, dtype):
    for p in shapes:
        x = signal(p, True, dtype)
        v = DspVec(x, is_complex=True, delta=0.5)
        assert v.multiply_complex_exponential(0.02, 0.3) == 0 and len(v) == 2 * p
        got = v.data()
        # a and b are multiplied by delta in T first (complex_ops.rs:83-84)
        a, b = float(dtype(0.02) * dtype(0.5)), float(dtype(0.3) * dtype(0.5))
        exact = x.astype(np.float64).view(np.complex128) * np.exp(1j * (a * np.arange(p) + b))
        err = rel_l2(got, exact.view(np.float64))
        assert err < (2e-7 if dtype == np.float32 else 1e-14), (p, err)
        running = orc.multiply_complex_exponential(np.array(x), 0.02, 0.3, 0.5)
        err = rel_l2(got, running)
        assert err < (5e-5 if dtype == np.float32 else 1e-11) * max(1.0, p / 3000.0), (p, err)
    r = DspVec(signal(3, False, dtype))
    assert r.multiply_complex_exponential(0.02, 0.3) == -1 and r.is_erroneous()


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_smaller_bit_equal_to_the_oracle(shapes, cplx, dtype):
    """operand lengths 1, points / 3 and points; an operand whose length does not divide the vector's: code 7"""
    e = 2 if cplx else 1
    for p in shapes:
        x = signal(p, cplx, dtype)
        for yp in sorted({1, p // 3 if p % 3 == 0 else p, p}):
            y = unaligned(orc.fill_uniform(yp * e, 77 + yp % 1000, 1, 10, dtype))
            tiled = np.tile(y.reshape(yp, e), (p // yp, 1)).reshape(-1)
            for op, name in enumerate(("add_smaller", "sub_smaller", "mul_smaller", "div_smaller")):
                v = DspVec(x, is_complex=cplx)
                assert getattr(v, name)(DspVec(y, is_complex=cplx)) == 0, (p, yp, name)
                code, ref = orc.binary(np.array(x), tiled, cplx, op)
                assert code == 0 and len(v) == p * e
                assert same_bits(v.data(), ref), (p, yp, name)
        if p > 2:
            v = DspVec(x, is_complex=cplx)
            assert v.add_smaller(DspVec(np.ones((p - 1) * e, dtype), is_complex=cplx)) == 7
            assert same_bits(v.data(), np.array(x)), p
