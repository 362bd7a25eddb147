"""Per-row statistics, sums and dot products of DspMat (one batched device pass) against the vector path row by row,
against the CPU oracle, and at the edges (ties, NaN / inf, empty, poisoned, split lengths, error codes)."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
KEYS = ("sum", "count", "average", "rms", "min", "min_index", "max", "max_index")


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def _epp(dtype, cplx):
    return 16 // np.dtype(dtype).itemsize // (2 if cplx else 1)


def _shapes(dtype, cplx):
    """(rows, points per row): every regime and its boundaries +- 1 point, odd real row lengths included."""
    s = [(1, 1), (7, 1), (65536, 3), (4097, 17), (4096, 64), (2049, 100), (1000, 1000), (333, 4097), (64, 65537),
         (8, 1000003), (513, 5), (129, 31)]
    e = _epp(dtype, cplx)
    for d in (-1, 0, 1):
        # mat_reduce.hip: MR_SHORT_MAX_PK (1024 packets), the long-row chunks (8192), lane groups 4 -> 8 and 32 -> 64
        s += [(37, 1024 * e + d), (3, 8192 * e + d), (11, 64 * e + d), (11, 512 * e + d)]
    return s


def _matrix(bd, rows, pts, dtype, cplx, seed):
    e = 2 if cplx else 1
    x = orc.fill_uniform(rows * pts * e, seed, -10, 10, dtype).reshape(rows, pts * e)
    return x, bd.DspMat(x, is_complex=cplx)


def _ulp(v, dtype):
    return float(np.spacing(np.asarray(abs(v), dtype=dtype)))


def _close(got, ref, mass, dtype):
    """|mat - vec| <= 1 ulp_T(|vec|) + 8 * 2^-53 * mass, real and imaginary part each"""
    for g, r in ((np.real(got), np.real(ref)), (np.imag(got), np.imag(ref))):
        if np.isnan(r):
            assert np.isnan(g)
            continue
        assert abs(float(g) - float(r)) <= _ulp(r, dtype) + 8 * 2.0 ** -53 * mass, (got, ref, mass)


def _sample(rows):
    if rows <= 64:
        return range(rows)
    return sorted(set(np.linspace(0, rows - 1, 64).astype(int).tolist()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", (False, True))
def test_rows_equal_the_vector_path(bd, dtype, cplx):
    for k, (rows, pts) in enumerate(_shapes(dtype, cplx)):
        x, m = _matrix(bd, rows, pts, dtype, cplx, 1000 + k)
        st, stp = m.statistics(), m.statistics(prec=True)
        s, sq, sp, sqp = m.sum(), m.sum_sq(), m.sum(prec=True), m.sum_sq(prec=True)
        y = orc.fill_uniform(pts * (2 if cplx else 1), 77 + k, -1, 1, dtype)
        yv = bd.DspVec(y, is_complex=cplx)
        dc, d = m.dot_product(yv)
        assert dc == 0
        for r in _sample(rows):
            v = bd.DspVec(x[r], is_complex=cplx)
            xr = x[r].astype(np.float64)
            z = xr[0::2] + 1j * xr[1::2] if cplx else xr
            m1, m2 = float(np.sum(np.abs(z))), float(np.sum(np.abs(z) ** 2))
            for got, ref, T in ((st, v.statistics(), dtype), (stp, v.statistics(prec=True), np.float64)):
                for key in ("count", "min", "max", "min_index", "max_index"):
                    assert got[key][r] == ref[key], (rows, pts, r, key, got[key][r], ref[key])
                _close(got["sum"][r], ref["sum"], m1, T)
                _close(got["average"][r], ref["average"], m1, T)
                _close(got["rms"][r], ref["rms"], m2, T)
            _close(s[r], v.sum(), m1, dtype)
            _close(sp[r], v.sum(prec=True), m1, np.float64)
            _close(sq[r], v.sum_sq(), m2, dtype)
            _close(sqp[r], v.sum_sq(prec=True), m2, np.float64)
            vc, vd = v.dot_product(yv)
            assert vc == 0
            _close(d[r], vd, m1, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", (False, True))
def test_rows_against_the_oracle(bd, dtype, cplx):
    tol = 2e-5 if dtype == np.float32 else 1e-12
    e = 2 if cplx else 1
    stats = orc.complex_statistics if cplx else orc.real_statistics
    for k, (rows, pts) in enumerate(((300, 1000), (17, 40000), (4, 300001), (2000, 7))):
        x = orc.fill_uniform(rows * pts * e, 31 + k, -10, 10, dtype).reshape(rows, pts * e)
        for r in range(rows):  # a unique maximum and minimum at row-dependent positions
            imx, imn = (r * 7919 + 3) % pts, (r * 104729 + 11) % pts
            if imn == imx:
                imn = (imn + 1) % pts
            if cplx:
                x[r, 2 * imx:2 * imx + 2] = 77.0
                x[r, 2 * imn:2 * imn + 2] = 0.0
            else:
                x[r, imx], x[r, imn] = 77.0, -88.0
        m = bd.DspMat(x, is_complex=cplx)
        st = m.statistics()
        s, sq = m.sum(), m.sum_sq()
        y = orc.fill_uniform(rows * pts * e, 9 + k, -1, 1, dtype).reshape(rows, pts * e)
        code, d = m.dot_product(bd.DspMat(y, is_complex=cplx))
        assert code == 0
        code, parts = m.statistics_split(3)
        assert code == 0
        for r in _sample(rows):
            x64 = x[r].astype(np.float64)
            ref = stats(x64)
            assert st["count"][r] == ref["count"] == pts
            for key in ("min", "max", "min_index", "max_index"):
                assert st[key][r] == ref[key], (rows, pts, r, key)
            for key in ("sum", "average", "rms"):
                assert abs(st[key][r] - ref[key]) <= tol * max(1.0, abs(ref[key])) * 50, (key, st[key][r], ref[key])
            rs, rq = orc.vec_sum(x64, cplx), orc.vec_sum(x64, cplx, True)
            assert abs(s[r] - rs) <= tol * 50 * max(1.0, abs(rs)) and abs(sq[r] - rq) <= tol * 50 * abs(rq)
            rd = orc.dot(x64, y[r].astype(np.float64), cplx)
            assert abs(d[r] - rd) <= tol * 50 * max(1.0, abs(rd))
            for b in range(3):
                rb = stats(x64, b, 3)
                assert parts["count"][r, b] == rb["count"]
                assert parts["max_index"][r, b] == rb["max_index"] and parts["min_index"][r, b] == rb["min_index"]
                assert abs(parts["sum"][r, b] - rb["sum"]) <= tol * 50 * max(1.0, abs(rb["sum"]))


@pytest.mark.parametrize("cplx", (False, True))
def test_ties_nan_and_inf(bd, cplx):
    dtype = np.float32
    e = 2 if cplx else 1
    # a tied maximum and minimum in one short, one medium and one chunked row length: the first occurrence wins
    for pts, a, b in ((40, 3, 30), (5000, 100, 4000), (300000, 5000, 200000)):
        x = orc.fill_uniform(2 * pts * e, 5, -1, 1, dtype).reshape(2, pts * e)
        x[:, a * e:(a + 1) * e] = 9.0
        x[:, b * e:(b + 1) * e] = 9.0
        x[:, (a + 1) * e:(a + 2) * e] = -9.0 if not cplx else 0.0
        x[:, (b + 1) * e:(b + 2) * e] = -9.0 if not cplx else 0.0
        st = bd.DspMat(x, is_complex=cplx).statistics()
        assert list(st["max_index"]) == [a, a] and list(st["min_index"]) == [a + 1, a + 1]
    # NaN never wins a comparison, sums propagate NaN / inf; the same bits as the vector path
    x = orc.fill_uniform(6 * 64 * e, 6, -1, 1, dtype).reshape(6, 64 * e)
    x[0, 5] = np.nan
    x[1, 0] = np.nan
    x[2, 7] = np.inf
    x[3, 9], x[3, 20] = np.inf, -np.inf
    x[4, :] = np.nan
    x[5, 3] = -np.inf
    st = bd.DspMat(x, is_complex=cplx).statistics()
    for r in range(6):
        ref = bd.DspVec(x[r], is_complex=cplx).statistics()
        for key in KEYS:
            for g, f in ((np.real(st[key][r]), np.real(ref[key])), (np.imag(st[key][r]), np.imag(ref[key]))):
                if key in ("sum", "average", "rms") and np.isfinite(f):  # finite sums: added in another order
                    assert abs(float(g) - float(f)) <= 1e-5 * max(1.0, abs(float(f))), (r, key, g, f)
                else:
                    assert g == f or (np.isnan(g) and np.isnan(f)), (r, key, g, f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_rows_and_poisoned(bd, dtype):
    for cplx in (False, True):
        m0 = bd.DspMat(rows=0, row_len=8, is_complex=cplx, dtype=dtype)
        assert m0.statistics()["count"].size == 0 and m0.sum().size == 0
        me = bd.DspMat(rows=5, row_len=0, is_complex=cplx, dtype=dtype)
        st = me.statistics()
        assert list(st["count"]) == [0] * 5 and np.all(np.isnan(st["average"]))
        if cplx:
            assert np.all(st["min"] == complex(np.inf, np.inf)) and np.all(st["max"] == 0)
        else:
            assert np.all(st["min"] == np.inf) and np.all(st["max"] == -np.inf)
        assert np.all(me.sum() == 0)
    # poisoned: multiply_frequency_response on a time-domain matrix; every call reports -1, results still written
    m = bd.DspMat(orc.fill_uniform(4 * 32, 3, -1, 1, dtype).reshape(4, 32), dtype=dtype)
    assert m.multiply_frequency_response(0, 0.5) == -1
    sfx = "32" if dtype == np.float32 else "64"
    St = bd._lib.Statistics32 if sfx == "32" else bd._lib.Statistics64
    out = (St * 4)()
    assert getattr(bd.lib, "bdsp_hip_mat_real_statistics" + sfx)(m._h, out, 4) == -1
    assert [out[i].count for i in range(4)] == [0] * 4
    code, parts = m.statistics_split(2)
    assert code == -1 and parts["count"].shape == (4, 2)
    assert m.dot_product(bd.DspVec(np.ones(32, dtype)))[0] == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_lengths_and_error_codes(bd, dtype):
    sfx = "32" if dtype == np.float32 else "64"
    for cplx in (False, True):
        e = 2 if cplx else 1
        x = orc.fill_uniform(9 * 50 * e, 8, -5, 5, dtype).reshape(9, 50 * e)
        m = bd.DspMat(x, is_complex=cplx)
        for ln in (1, 2, 3, 16):
            code, parts = m.statistics_split(ln)
            assert code == 0 and parts["count"].shape == (9, ln)
            for r in (0, 8):
                code, ref = bd.DspVec(x[r], is_complex=cplx).statistics_split(ln)
                for b in range(ln):
                    for key in ("count", "min", "max", "min_index", "max_index"):
                        assert parts[key][r, b] == ref[b][key]
        assert m.statistics_split(17)[0] == 7
        code, parts = m.statistics_split(0)
        assert code == 0 and parts["count"].shape == (9, 0)
        # wrong output lengths
        St = bd._lib.Statistics32 if sfx == "32" else bd._lib.Statistics64
        out = (St * 20)()
        assert getattr(bd.lib, "bdsp_hip_mat_real_statistics" + sfx)(m._h, out, 8) == 7
        assert getattr(bd.lib, "bdsp_hip_mat_real_statistics_split" + sfx)(m._h, out, 17, 2) == 7
        vals = (C.c_double * 20)()
        assert getattr(bd.lib, "bdsp_hip_mat_real_sum_prec" + sfx)(m._h, vals, 10) == 7
    r = bd.DspMat(orc.fill_uniform(4 * 10, 1, -1, 1, dtype).reshape(4, 10), dtype=dtype)
    c = bd.DspMat(orc.fill_uniform(4 * 10, 2, -1, 1, dtype).reshape(4, 10), is_complex=True, dtype=dtype)
    cf = bd.DspMat(orc.fill_uniform(4 * 10, 2, -1, 1, dtype).reshape(4, 10), is_complex=True, domain=1, dtype=dtype)
    assert c.dot_product(r)[0] == 2 and c.dot_product(cf)[0] == 2 and c.dot_product(bd.DspVec(np.ones(10, dtype)))[0] == 2
    assert r.dot_product(c)[0] == 0  # real_* walks the scalars, the operand's number space is not checked (as dot)
    vals = (C.c_double * 8)()
    assert getattr(bd.lib, "bdsp_hip_mat_real_dot_product_prec" + sfx)(c._h, r._h, vals, 4) == 4
    assert getattr(bd.lib, "bdsp_hip_mat_complex_dot_product_prec" + sfx)(r._h, c._h, (bd._lib.Complex64 * 4)(), 4) == 3
    r5 = bd.DspMat(orc.fill_uniform(5 * 10, 3, -1, 1, dtype).reshape(5, 10), dtype=dtype)
    assert r.dot_product(r5)[0] == 7
    assert getattr(bd.lib, "bdsp_hip_mat_real_dot_product_prec" + sfx)(r._h, r._h, vals, 3) == 7
    # a broadcast vector shorter than the row: min(row length, vector length) elements per row
    for cplx, m in ((False, r), (True, c)):
        y = orc.fill_uniform(6, 4, -1, 1, dtype)
        code, d = m.dot_product(bd.DspVec(y, is_complex=cplx))
        assert code == 0
        xs = m.data().astype(np.float64)
        for i in range(4):
            ref = orc.dot(xs[i, :6], y.astype(np.float64), cplx)
            assert abs(d[i] - ref) <= 1e-5 * max(1.0, abs(ref))
    # real_* on a complex matrix walks every scalar, as the vector facade
    got = np.zeros(4)
    assert getattr(bd.lib, "bdsp_hip_mat_real_sum_prec" + sfx)(c._h, got.ctypes.data_as(C.POINTER(C.c_double)), 4) == 0
    xs = c.data()
    for i in range(4):
        v = bd.DspVec(xs[i])
        assert abs(got[i] - v.sum(prec=True)) <= 1e-12 * max(1.0, float(np.sum(np.abs(xs[i]))))


def test_repeated_calls_are_bit_identical(bd):
    for rows, pts in ((8192, 24), (700, 3000), (4, 400000)):
        x, m = _matrix(bd, rows, pts, np.float32, True, 99)
        a, b = m.statistics(), m.statistics()
        for key in KEYS:
            assert a[key].tobytes() == b[key].tobytes(), (rows, pts, key)
        y = bd.DspVec(orc.fill_uniform(pts * 2, 98, -1, 1, np.float32), is_complex=True)
        assert m.dot_product(y)[1].tobytes() == m.dot_product(y)[1].tobytes()
        assert m.sum_sq(prec=True).tobytes() == m.sum_sq(prec=True).tobytes()


def test_statistics_is_one_batched_call(bd):
    """65 536 rows x 16 complex f32 points: a per-row launch-and-sync loop cannot return within 20 ms."""
    x, m = _matrix(bd, 65536, 16, np.float32, True, 7)
    for _ in range(3):
        m.statistics()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        st = m.statistics()
        best = min(best, time.perf_counter() - t0)
    assert st["count"].shape == (65536,) and np.all(st["count"] == 16)
    assert best < 0.020, best
