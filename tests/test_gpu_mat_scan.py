"""DspMat.diff / diff_with_start / cum_sum / wrap / unwrap: every row against the CPU oracle and against the vector
path on that row, in every regime of mat_scan.hip and at its boundaries, plus row isolation, codes and state, and the
chain correlate -> phase -> unwrap -> diff on a batch of chirps."""
import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
SCAN_CHUNK = 4096      # mat_scan_core.h
SCAN_SHORT = 512       # mat_scan.hip MS_SCAN_SHORT: a lane group per row up to here, then a workgroup per row
TILE_BYTES = 16384     # mat_scan_core.h MS_TILE_BYTES


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def _shapes(bd, dtype):
    """(rows, points per row).  The regime list of test_gpu_mat_reductions.py with rows capped at 300 000 points (one
    lane walks an unwrap row), plus this unit's boundaries +- 1: the unwrap tile widths of the four tile shapes, the
    row counts at which the tile shape changes (4 workgroups per CU of 1, 4, 16 rows) and around the 64 lanes of a
    workgroup, SCAN_CHUNK, the lane-group / workgroup-per-row threshold of cum_sum and its lane-group sizes."""
    s = [(1, 1), (7, 1), (65536, 3), (4097, 17), (4096, 64), (2049, 100), (1000, 1000), (333, 4097), (64, 65537),
         (8, 300000), (513, 5), (129, 31), (1, 300000), (1, 77), (5, 0), (0, 9)]
    elems = TILE_BYTES // np.dtype(dtype).itemsize
    cus = bd.lib.bdsp_hip_compute_units()
    for d in (-1, 0, 1):
        s += [(4 * cus * 16 + 1, elems // 64 + d),  # 64 rows per workgroup: W = 64 f32 / 32 f64
              (4 * cus * 4 + 1, elems // 16 + d), (4 * cus + 1, elems // 4 + d), (3, elems + d),
              (37, SCAN_CHUNK + d), (19, 2 * SCAN_CHUNK + d), (301, SCAN_SHORT + d), (1001, 8 + d), (1001, 64 + d),
              (63 + d, 130), (4 * cus + d, 9), (4 * cus * 4 + d, 9), (4 * cus * 16 + d, 9), (4 * cus * 16 + 64 + d, 70)]
    return s


def _mat(bd, x, cplx=False):
    return bd.DspMat(x, is_complex=cplx)


def _sample(rows, n=3):
    return sorted(set(np.linspace(0, rows - 1, min(rows, n)).astype(int).tolist())) if rows else []


def _ulp(v, dtype):
    return np.spacing(np.abs(np.asarray(v, dtype=dtype))).astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", (False, True))
def test_diff_rows_equal_the_oracle(bd, dtype, cplx):
    e = 2 if cplx else 1
    for k, (rows, pts) in enumerate(_shapes(bd, dtype)):
        x = orc.fill_uniform(rows * pts * e, 300 + k, -10, 10, dtype).reshape(rows, pts * e)
        for with_start in (False, True):
            m = _mat(bd, x, cplx)
            assert (m.diff_with_start() if with_start else m.diff()) == 0
            new_len = pts * e if with_start else max(pts - 1, 0) * e
            assert m.rows() == rows and m.row_len() == (new_len if rows else 0), (rows, pts, with_start)
            assert m.is_complex() == cplx and m.domain() == 0 and m.delta() == 1.0
            got = m.data()
            if rows * pts == 0:
                continue
            # diff's arithmetic is one subtraction per element: the oracle's, vectorised over the rows ...
            ref = x.copy() if with_start else x[:, e:] - x[:, :-e]
            if with_start:
                ref[:, e:] = x[:, e:] - x[:, :-e]
            assert np.array_equal(got, ref), (rows, pts, with_start)
            for r in _sample(rows, 5):  # ... and the oracle itself on sampled rows
                assert np.array_equal(got[r], orc.diff(x[r], cplx, with_start)), (rows, pts, r, with_start)


def _unwrap_inputs(rows, n, dtype, seed):
    """(name, data, divisor).  Ramps: slopes in [1, 2.9] rad / sample, a different one per row: eight samples travel at
    least 7 rad, more than a turn, so every row of eight or more samples wraps at least once."""
    t = np.arange(n, dtype=np.float64)[None, :] * np.linspace(1.0, 2.9, rows)[:, None] + np.arange(rows)[:, None] * 0.7
    ramp = (np.mod(t + np.pi, 2 * np.pi) - np.pi).astype(dtype)
    uni = orc.fill_uniform(rows * n, seed, -30, 30, dtype).reshape(rows, n)
    big = (orc.fill_uniform(rows * n, seed + 1, -1, 1, dtype) * dtype(1e6)).astype(dtype)
    flat = big.reshape(-1)
    flat[::7] = np.round(flat[::7] / 3) * 3
    big = flat.reshape(rows, n)
    wide = orc.fill_uniform(rows * n, seed + 2, -100, 100, dtype).reshape(rows, n)
    return [("ramp", ramp, 2 * np.pi), ("uniform", uni, 7.0), ("big / 3", big, 3.0), ("big / 1e-3", big, 1e-3),
            ("wide / 0.1", wide, 0.1), ("negative divisor", uni, -7.0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwrap_rows_equal_the_oracle_bit_for_bit(bd, dtype):
    for k, (rows, n) in enumerate(_shapes(bd, dtype)):
        if rows * n == 0:
            m = bd.DspMat(rows=rows, row_len=n, dtype=dtype)
            assert m.unwrap(7.0) == 0 and m.rows() == rows and m.row_len() == (n if rows else 0)
            continue
        for name, x, div in _unwrap_inputs(rows, n, dtype, 500 + 3 * k):
            ref = np.stack([orc.unwrap(x[r], dtype(div)) for r in range(rows)])
            if n >= 8:  # from the oracle alone, before the device is asked: an identity kernel cannot pass
                changed = np.any(ref.view(np.uint8) != x.view(np.uint8), axis=1)
                assert changed.mean() >= 0.9, (name, rows, n, changed.mean())
            m = _mat(bd, x)
            assert m.unwrap(dtype(div)) == 0
            assert m.rows() == rows and m.row_len() == n and not m.is_complex() and m.domain() == 0 and m.delta() == 1.0
            got = m.data()
            assert np.array_equal(got, ref, equal_nan=True), (name, rows, n, np.argwhere(got != ref)[:4])
            for r in _sample(rows):
                v = bd.DspVec(x[r])
                assert v.unwrap(dtype(div)) == 0
                assert np.array_equal(v.data(), got[r], equal_nan=True), (name, rows, n, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_equals_the_oracle_on_the_flat_data(bd, dtype):
    for k, (rows, n) in enumerate(((1, 1), (7, 1), (1000, 1000), (65536, 3), (3, 100001), (5, 0), (0, 4))):
        x = orc.fill_uniform(rows * n, 40 + k, -100, 100, dtype).reshape(rows, n)
        for div in (7.0, 2 * np.pi, -3.0, 0.1):
            m = _mat(bd, x) if x.size else bd.DspMat(rows=rows, row_len=n, dtype=dtype)
            assert m.wrap(dtype(div)) == 0
            assert m.rows() == rows and m.row_len() == (n if rows else 0)
            if x.size:
                assert np.array_equal(m.data().reshape(-1), orc.math(x.reshape(-1), False, "wrap", dtype(div))), (rows, n, div)


def _chain(n):
    """Longest chain of double additions between an input and an output of the three-step scan (mat_scan.hip's long
    rows, and a long vector), counted from the code: chunk sums 16 per thread + 8 tree levels;
    offsets 2 * ceil(nchunks / 256) per thread + the 256-step serial scan; apply 16 thread total + 8 Hillis-Steele
    + 1 offset + 16 running.  mat_scan.hip's one-pass regimes are shorter (lane groups: 6 shuffle steps + at most 8
    carries; workgroup per row: the 41 of apply), so the same count bounds them."""
    per = -(-(-(-n // SCAN_CHUNK)) // 256)
    return 24 + 2 * per + 256 + 41


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", (False, True))
def test_cum_sum_rows(bd, dtype, cplx):
    e = 2 if cplx else 1
    bound = 2e-7 if dtype == np.float32 else 1e-13   # test_gpu_parity.py::test_diff_cum_sum_wrap_unwrap
    differing = sampled = 0
    for k, (rows, pts) in enumerate(_shapes(bd, dtype)):
        x = orc.fill_uniform(rows * pts * e, 700 + k, -10, 10, dtype).reshape(rows, pts * e)
        m = _mat(bd, x, cplx) if x.size else bd.DspMat(rows=rows, row_len=pts * e, is_complex=cplx, dtype=dtype)
        assert m.cum_sum() == 0
        assert m.rows() == rows and m.row_len() == (pts * e if rows else 0) and m.is_complex() == cplx
        assert m.domain() == 0 and m.delta() == 1.0
        if not x.size:
            continue
        got = m.data().astype(np.float64).reshape(rows, pts, e)
        ref = np.cumsum(x.astype(np.float64).reshape(rows, pts, e), axis=1)
        scale = np.max(np.abs(ref), axis=(1, 2)) + 1.0
        err = np.max(np.abs(got - ref), axis=(1, 2)) / scale
        print("cum_sum %s cplx=%d %d x %d: max err / (max |prefix| + 1) = %.3e" % (np.dtype(dtype).name, cplx, rows, pts, err.max()))
        assert err.max() < bound, (rows, pts, err.max())
        # against the vector path: both round the same exact prefix once to T, each after its own double chain
        D = 2 * _chain(pts)
        for r in _sample(rows):
            v = bd.DspVec(x[r], is_complex=cplx)
            assert v.cum_sum() == 0
            vec = v.data()
            mass = np.sum(np.abs(x[r].astype(np.float64)))
            diff = np.abs(got[r].reshape(-1) - vec.astype(np.float64))
            assert np.all(diff <= _ulp(vec, dtype) + D * 2.0 ** -53 * mass), (rows, pts, r, diff.max())
            differing += int(np.count_nonzero(diff))
            sampled += diff.size
    print("cum_sum %s cplx=%d: %d of %d sampled elements differ from the vector path" % (np.dtype(dtype).name, cplx, differing, sampled))
    # (reported, not asserted: two double prefixes round to different f32 values only when an f32 tie lies between them)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_isolated(bd, dtype):
    """NaN, +-inf and 1e30 in one row: every other row bit-identical to the call on the clean matrix, the affected row
    as the vector path on that row."""
    for rows, n in ((70, 300), (70, 3000), (70, 9000), (1100, 40)):
        x = orc.fill_uniform(rows * n, 11, -30, 30, dtype).reshape(rows, n)
        bad = x.copy()
        r0 = rows // 2 + 1
        bad[r0, n // 30], bad[r0, n // 2], bad[r0, n // 2 + n // 10], bad[r0, n - n // 6] = 1e30, np.inf, -np.inf, np.nan
        others = np.arange(rows) != r0
        for op in ("cum_sum", "unwrap"):
            res = []
            for data in (x, bad):
                m = _mat(bd, data)
                assert (m.cum_sum() if op == "cum_sum" else m.unwrap(dtype(7.0))) == 0
                res.append(m.data())
            clean, got = res
            assert clean[others].tobytes() == got[others].tobytes(), (op, rows, n)
            v = bd.DspVec(bad[r0])
            assert (v.cum_sum() if op == "cum_sum" else v.unwrap(dtype(7.0))) == 0
            vec = v.data()
            if op == "unwrap":
                assert np.array_equal(got[r0], vec, equal_nan=True), (rows, n)
                continue
            # cum_sum: the same non-finite pattern; finite values within the two schemes' rounding (test_cum_sum_rows)
            assert np.array_equal(np.isnan(got[r0]), np.isnan(vec)) and np.isnan(vec).any()
            inf = np.isinf(vec)
            assert np.array_equal(np.isinf(got[r0]), inf) and np.array_equal(got[r0][inf], vec[inf]) and inf.any()
            fin = np.isfinite(vec)
            mass = np.sum(np.abs(bad[r0].astype(np.float64))[: n // 2])
            d = np.abs(got[r0][fin].astype(np.float64) - vec[fin].astype(np.float64))
            assert np.all(d <= _ulp(vec[fin], dtype) + 2 * _chain(n) * 2.0 ** -53 * mass), (rows, n, d.max())


def _poisoned(m):
    return m.row_len() == 0 and np.isnan(m.delta())


@pytest.mark.parametrize("dtype", DTYPES)
def test_codes_and_state(bd, dtype):
    x = orc.fill_uniform(6 * 40, 3, -10, 10, dtype).reshape(6, 40)
    # complex wrap / unwrap: -1, poisoned afterwards, and every later call reports -1
    for op in ("wrap", "unwrap"):
        m = _mat(bd, x, True)
        assert getattr(m, op)(dtype(3.0)) == -1 and _poisoned(m) and m.rows() == 6 and m.is_complex()
        assert m.diff() == -1 and m.diff_with_start() == -1 and m.cum_sum() == -1
        assert m.wrap(dtype(3.0)) == -1 and m.unwrap(dtype(3.0)) == -1 and _poisoned(m)
    # poisoned by another call (multiply_frequency_response on a time-domain matrix)
    m = _mat(bd, x)
    assert m.multiply_frequency_response(0, 0.5) == -1
    assert m.diff() == -1 and m.diff_with_start() == -1 and m.cum_sum() == -1
    assert m.wrap(dtype(3.0)) == -1 and m.unwrap(dtype(3.0)) == -1 and _poisoned(m)
    # no rows, empty rows: 0, shape untouched
    for cplx in (False, True):
        for rows, rl in ((0, 8), (5, 0)):
            m = bd.DspMat(rows=rows, row_len=rl, is_complex=cplx, dtype=dtype)
            assert m.diff() == 0 and m.diff_with_start() == 0 and m.cum_sum() == 0
            if not cplx:
                assert m.wrap(dtype(3.0)) == 0 and m.unwrap(dtype(3.0)) == 0
            assert m.rows() == rows and m.row_len() == 0 and m.is_complex() == cplx and not np.isnan(m.delta())
    # domain, delta and number space stay
    for cplx in (False, True):
        m = bd.DspMat(x, is_complex=cplx, domain=1, delta=0.25)
        ops = [m.diff, m.diff_with_start, m.cum_sum] + ([] if cplx else [lambda: m.wrap(dtype(3.0)), lambda: m.unwrap(dtype(3.0))])
        for f in ops:
            assert f() == 0 and m.domain() == 1 and m.delta() == 0.25 and m.is_complex() == cplx and m.rows() == 6
    # diff until the rows are empty, then once more
    for cplx in (False, True):
        e = 2 if cplx else 1
        m = _mat(bd, x[:, :4 * e].copy(), cplx)
        ref = x[:, :4 * e].copy()
        for left in (3, 2, 1, 0, 0):
            assert m.diff() == 0 and m.rows() == 6 and m.row_len() == left * e and not np.isnan(m.delta())
            ref = ref[:, e:] - ref[:, :-e] if ref.shape[1] else ref
            assert np.array_equal(m.data(), ref)
        assert m.diff_with_start() == 0 and m.cum_sum() == 0 and m.row_len() == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_chirp_slopes_from_correlate_phase_unwrap_diff(bd, dtype):
    """The README chain on linear chirps z[n] = exp(i pi k n^2): correlated with a unit impulse at the centre of the
    argument every row comes back in one piece inside its padding, phase -> unwrap(2 pi) -> diff is the instantaneous
    frequency pi k (2n + 1), whose slope per sample is 2 pi k.
    Tolerance, from the number formats.  An unwrapped phase moves at most pi per sample, so |y| <= pi (L + 1) over the L
    points of a row; a stored y carries at most one ulp_T(pi (L + 1)) of rounding (cur - prev and prev + diff, half an
    ulp each; nothing accumulates, since prev + diff is cur minus a whole number of divisors).  The phase of a
    unit-magnitude sample after the two length-L transforms of correlate (L = 2048: 2 x 11 butterfly stages of at most
    one eps_T each, the product with the argument, atan2 within 2 ulp) is off by at most eps_noise = 64 eps_T.  A
    difference of neighbours is then off by at most e = 2 ulp_T(pi (L + 1)) + 2 eps_noise, and the least-squares slope
    sum w_n f[n], w_n = (n - mean) / sum (n - mean)^2, over N samples by at most e * sum |w_n| <= 3 e / N."""
    p, rows, L = 1000, 32, 2048
    ks = (0.1 + 0.3 * np.arange(rows) / rows) / p           # pi k (2n + 1) < pi / 2 for n < p: no aliasing
    nn = np.arange(p, dtype=np.float64)
    z = np.exp(1j * np.pi * ks[:, None] * nn[None, :] ** 2)
    x = np.empty((rows, 2 * p), dtype)
    x[:, 0::2], x[:, 1::2] = z.real, z.imag
    imp = np.zeros(2 * L, dtype)
    imp[2 * (L // 2)] = 1.0                                 # the impulse at the centre: zero lag, the rows come back in one piece
    # where the oracle (float64, row 0) puts the signal, and that it is not conjugated
    code, ref_arg = orc.prepare_argument(imp.astype(np.float64), False)
    assert code == 0
    code, c = orc.correlate(x[0].astype(np.float64), ref_arg)
    assert code == 0
    cz = c[0::2] + 1j * c[1::2]
    assert cz.size == L
    on = np.flatnonzero(np.abs(cz) > 0.5)
    assert on.size == p and on[-1] - on[0] == p - 1
    lo, hi = on[0] + 2, on[-1] - 2                          # diff[j] = y[j + 1] - y[j], j in [lo, hi)
    N = hi - lo
    w = np.arange(N, dtype=np.float64) - (N - 1) / 2.0
    w /= np.sum(w * w)
    assert np.sum(np.abs(w)) <= 3.0 / N
    f_ref = np.diff(np.unwrap(np.angle(cz)))[lo:hi]
    assert abs(np.dot(w, f_ref) - 2 * np.pi * ks[0]) < 1e-9
    arg = bd.DspVec(imp, is_complex=True)
    assert arg.prepare_argument() == 0
    m = bd.DspMat(x, is_complex=True)
    assert m.correlate(arg) == 0 and m.phase() == 0 and m.unwrap(dtype(2 * np.pi)) == 0 and m.diff() == 0
    assert m.rows() == rows and m.row_len() == L - 1 and not m.is_complex()
    f = m.data().astype(np.float64)
    eps = float(np.finfo(dtype).eps)
    e = 2 * float(np.spacing(dtype(np.pi * (L + 1)))) + 2 * 64 * eps
    tol = 3 * e / N
    slopes = f[:, lo:hi] @ w
    print("chirp slopes %s: max |slope - 2 pi k| = %.3e, tolerance %.3e" % (np.dtype(dtype).name, np.max(np.abs(slopes - 2 * np.pi * ks)), tol))
    assert np.all(np.abs(slopes - 2 * np.pi * ks) <= tol), (np.max(np.abs(slopes - 2 * np.pi * ks)), tol)
