"""DspMat.plain_sfft / sfft / windowed_sfft / plain_sifft / sifft / windowed_sifft / mirror / to_complex: every sampled
row against the float64 CPU oracle and against the vector path; row isolation, determinism, the rejection of a row whose
first bin is not real, the other codes, and end to end in front of a peak search.

Tolerances are the ones the project holds the vector family to (test_gpu_parity.py, test_symmetric_fft_family and
test_shifted_and_windowed_symmetric_transforms_against_oracle), tol = 1e-6 (f32) / 1e-12 (f64): forward transforms
rel-L2 < 2 tol, the round trip plain_sfft -> plain_sifft / N < 4 tol, sifft < 2 tol (plain_sifft on a given half spectrum
is the same transform without the exact scale and the index move: 2 tol as well), windowed_sifft < 4 tol; against the
vector path twice the respective bound; mirror and to_complex bit-equal."""
import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
TIME, FREQ = 0, 1
TRIANGULAR, HAMMING, BLACKMAN_HARRIS, HANN = 0, 1, 2, 4
# (window id of the library, window id and alpha of the oracle)
WINDOWS = ((HAMMING, 1, 0.54), (HANN, 1, 0.5), (TRIANGULAR, 0, 0.0), (BLACKMAN_HARRIS, 2, 0.0))
# N = real points of a row: 1, 3 (p = 1, 2: the edges of the mirror and of the first-bin rule); 9, 45, 225 (the
# register-resident mixed-radix kernels); 1001 (f32 real rows unaligned for every other row, p = 501 odd); 255 and 4097
# (chirp-z, factors 17 and 17 * 241: computed noise in the first bin)
POINTS = (1, 3, 9, 45, 225, 1001, 255, 4097)
ROWS = (1, 2, 3, 257, 1003)
SHAPES = [(n, r) for n in POINTS for r in ROWS] + [(3, 70001)]  # + grid dimensions and batch above 65 535


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def tol_of(dtype):
    return 1e-6 if dtype == np.float32 else 1e-12


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    # a window of ONE point is 0/0 in the reference (cos(2 pi n / (N - 1))): where the reference has NaN the result must
    # have NaN, and the distance is taken over the rest
    nan = np.isnan(ref)
    if nan.any():
        assert np.array_equal(np.isnan(got), nan), (got, ref)
        got, ref = got[~nan], ref[~nan]
        if not ref.size:
            return 0.0
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def sample_rows(rows):
    """at most 64 rows: the first, the last, the rest spread evenly"""
    if rows <= 64:
        return list(range(rows))
    return sorted({0, rows - 1} | set(np.linspace(0, rows - 1, 62).astype(int).tolist()))


def same_meta(m, v, what):
    assert m.is_complex() == v.is_complex() and m.domain() == v.domain(), what
    assert m.row_len() == len(v), what
    dm, dv = m.delta(), v.delta()
    assert dm == dv or (np.isnan(dm) and np.isnan(dv)), (what, dm, dv)


_inputs = {}


def real_rows(n, rows, dtype):
    """the time-domain matrix of a shape, made once and never changed"""
    key = ("t", n, rows, dtype)
    if key not in _inputs:
        x = orc.fill_uniform(rows * n, 20161018 + 31 * n + rows, -10, 10, dtype).reshape(rows, n)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def half_spectra(n, rows, dtype, tested):
    """random half spectra of p = n // 2 + 1 bins per row whose scalar `tested` (an imaginary part) is 0 in every row"""
    p = n // 2 + 1
    key = ("f", n, rows, dtype, tested)
    if key not in _inputs:
        h = orc.fill_uniform(rows * 2 * p, 77 + 13 * n + rows, -10, 10, dtype).reshape(rows, 2 * p)
        h[:, tested] = 0
        h.setflags(write=False)
        _inputs[key] = h
    return _inputs[key]


_refs = {}


def forward_ref(n, rows, dtype, r, kind):
    """float64 reference of row r: kind "plain", "shift" or a window of WINDOWS"""
    key = (n, rows, dtype, r, kind)
    if key not in _refs:
        p = n // 2 + 1
        xd = real_rows(n, rows, dtype)[r].astype(np.float64)
        if kind == "plain":
            ref = np.fft.fft(xd)[:p].view(np.float64)
        else:
            c = orc.zero_interleave(xd, False, 2)
            if kind != "shift":
                c = orc.apply_window(c, True, kind[1], kind[2])
            ref = orc.swap_halves(orc.fft(c), True, True)[:2 * p]
        _refs[key] = ref
    return _refs[key]


def oracle_sifft(hd, p, shifted):
    y = hd
    if shifted:
        y = orc.swap_halves(orc.complex_scale(hd, 1.0 / p, 0.0), True, False)
    return orc.fft(orc.mirror(y), inverse=True)[0::2]


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,rows", SHAPES)
def test_forward_forms_against_oracle_and_vector(bd, n, rows, dtype):
    tol, p = tol_of(dtype), n // 2 + 1
    x = real_rows(n, rows, dtype)
    sample = sample_rows(rows)
    ops = [("plain", "plain_sfft", ()), ("shift", "sfft", ())] + [(w, "windowed_sfft", (w[0],)) for w in WINDOWS]
    for kind, name, args in ops:
        m = bd.DspMat(x, delta=0.5)
        assert getattr(m, name)(*args) == 0, name
        assert m.is_complex() and m.domain() == FREQ and m.rows() == rows and m.row_points() == p
        assert m.delta() == dtype(0.5) * dtype(n)
        got = m.data()
        for r in sample:
            e = rel_l2(got[r], forward_ref(n, rows, dtype, r, kind))
            assert e < 2 * tol, (name, args, r, e)
            v = bd.DspVec(x[r], delta=0.5)
            assert getattr(v, name)(*args) == 0
            same_meta(m, v, name)
            e = rel_l2(got[r], v.data())
            assert e < 4 * tol, (name, args, r, e)


# ------------------------------------------------------------------ inverse
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,rows", SHAPES)
def test_inverse_forms_against_oracle_and_vector(bd, n, rows, dtype):
    tol, p = tol_of(dtype), n // 2 + 1
    sample = sample_rows(rows)
    # the round trip through a COMPUTED half spectrum (rounding noise in the first bin must pass the rule)
    x = real_rows(n, rows, dtype)
    m = bd.DspMat(x)
    assert m.plain_sfft() == 0 and m.plain_sifft() == 0
    assert not m.is_complex() and m.domain() == TIME and m.row_len() == n and m.rows() == rows
    got = m.data()
    for r in sample:
        e = rel_l2(got[r].astype(np.float64) / n, x[r])
        assert e < 4 * tol, ("round trip", r, e)
    # given half spectra: (method, arguments, shifted, bound against the oracle)
    for name, args, shifted, bound in (("plain_sifft", (), False, 2 * tol), ("sifft", (), True, 2 * tol),
                                       ("windowed_sifft", (HAMMING,), True, 4 * tol)):
        h = half_spectra(n, rows, dtype, 2 * (p // 2) + 1 if shifted else 1)
        m = bd.DspMat(h, is_complex=True, domain=FREQ, delta=0.25)
        assert getattr(m, name)(*args) == 0, name
        assert not m.is_complex() and m.domain() == TIME and m.row_len() == n and m.rows() == rows
        assert m.delta() == dtype(0.25) * dtype(n)
        got = m.data()
        for r in sample:
            ref = oracle_sifft(h[r].astype(np.float64), p, shifted)
            if args:
                ref = orc.apply_window(ref, False, 1, 0.54, unapply=True)
            e = rel_l2(got[r], ref)
            assert e < bound, (name, r, e)
            v = bd.DspVec(h[r], is_complex=True, domain=FREQ, delta=0.25)
            assert getattr(v, name)(*args) == 0
            same_meta(m, v, name)
            e = rel_l2(got[r], v.data())
            assert e < 2 * bound, (name, "vector", r, e)


# ------------------------------------------------------------------ mirror, to_complex
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,rows", SHAPES)
def test_mirror_and_to_complex_are_bit_exact(bd, n, rows, dtype):
    p = n // 2 + 1
    h = half_spectra(n, rows, dtype, 1)
    m = bd.DspMat(h, is_complex=True, domain=FREQ, delta=0.25)
    assert m.mirror() == 0
    assert m.is_complex() and m.domain() == FREQ and m.row_points() == 2 * p - 1 and m.delta() == dtype(0.25)
    got = m.data()
    for r in sample_rows(rows):
        assert np.array_equal(got[r], orc.mirror(h[r])), r
    v = bd.DspVec(h[rows - 1], is_complex=True, domain=FREQ, delta=0.25)
    assert v.mirror() == 0
    same_meta(m, v, "mirror")
    assert np.array_equal(got[rows - 1], v.data())
    # a complex TIME matrix is mirrored as well (only real time data is refused, freq.rs:56-59)
    m = bd.DspMat(h[:1], is_complex=True)
    assert m.mirror() == 0 and m.domain() == TIME and np.array_equal(m.data()[0], orc.mirror(h[0]))

    x = real_rows(n, rows, dtype)
    m = bd.DspMat(x, delta=0.5)
    assert m.to_complex() == 0
    assert m.is_complex() and m.domain() == TIME and m.row_points() == n and m.rows() == rows and m.delta() == dtype(0.5)
    got = m.data()
    for r in sample_rows(rows):
        assert np.array_equal(got[r], orc.zero_interleave(x[r], False, 2)), r


# ------------------------------------------------------------------ row isolation, determinism
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [45, 255, 1001])
def test_rows_do_not_see_each_other_and_calls_repeat(bd, n, dtype):
    rows, p = 257, n // 2 + 1
    x = real_rows(n, rows, dtype)
    h = half_spectra(n, rows, dtype, 2 * (p // 2) + 1)
    cases = (("sfft", (), x, {}), ("windowed_sfft", (HANN,), x, {}),
             ("sifft", (), h, dict(is_complex=True, domain=FREQ)),
             ("windowed_sifft", (HAMMING,), h, dict(is_complex=True, domain=FREQ)),
             ("mirror", (), h, dict(is_complex=True, domain=FREQ)))
    for name, args, a, kw in cases:
        def run(data):
            m = bd.DspMat(data, **kw)
            assert getattr(m, name)(*args) == 0, name
            return m.data()
        first = run(a)
        assert np.array_equal(first, run(a)), (name, "two calls on equal input differ")
        b = a.copy()
        changed = 101
        b[changed, 0::2] = -b[changed, 0::2] + 1  # real scalars (time rows) or real parts (half spectra)
        second = run(b)
        keep = np.arange(rows) != changed
        assert np.array_equal(first[keep], second[keep]), name
        assert not np.array_equal(first[changed], second[changed]), name


# ------------------------------------------------------------------ rejection: one row's first bin is not real
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad_row", [0, 1002, 500])
def test_one_bad_row_poisons_the_matrix(bd, bad_row, dtype):
    n, rows = 45, 1003
    p = n // 2 + 1
    for name, args, tested in (("plain_sifft", (), 1), ("sifft", (), 2 * (p // 2) + 1),
                               ("windowed_sifft", (HAMMING,), 2 * (p // 2) + 1)):
        bad = half_spectra(n, rows, dtype, tested).copy()
        bad[bad_row, tested] = 1.0
        m = bd.DspMat(bad, is_complex=True, domain=FREQ)
        assert getattr(m, name)(*args) == 8, name
        assert m.is_complex() and m.domain() == FREQ and m.row_len() == 0 and np.isnan(m.delta())
        assert getattr(m, name)(*args) == -1  # the next call on the poisoned matrix
        # the vector path on that row alone says the same
        assert getattr(bd.DspVec(bad[bad_row], is_complex=True, domain=FREQ), name)(*args) == 8


def test_first_bin_rule_edges(bd):
    """p = 1 (re1 = im1 = 0) and p = 2; 1e-11 passes whatever the scale, noise passes below 1e-3 * (|re0| + |re1| +
    |im1|) and fails above -- as the vector path on the same row"""
    for row, code in (([5.0, 0.0], 0), ([5.0, 1.0], 8), ([5.0, 4.0e-3], 0), ([0.0, 1e-11], 0), ([0.0, 1e-9], 8),
                      ([1000.0, 0.9, 50.0, -50.0], 0), ([1000.0, -1.2, 50.0, -50.0], 8), ([3.0, -0.0, 1.0, 2.0], 0)):
        h = np.array([[1.0, 0.0] * (len(row) // 2), row, [2.0, 0.0] * (len(row) // 2)], np.float64)
        m = bd.DspMat(h, is_complex=True, domain=FREQ)
        assert m.plain_sifft() == code, row
        assert bd.DspVec(h[1], is_complex=True, domain=FREQ).plain_sifft() == code, row


# ------------------------------------------------------------------ the other codes
@pytest.mark.parametrize("dtype", DTYPES)
def test_codes(bd, dtype):
    forward = (("plain_sfft", ()), ("sfft", ()), ("windowed_sfft", (HANN,)))
    inverse = (("plain_sifft", ()), ("sifft", ()), ("windowed_sifft", (HANN,)))
    z = np.zeros((3, 10), dtype)
    for name, args in forward:
        m = bd.DspMat(z)  # even N
        assert getattr(m, name)(*args) == 9 and m.is_complex() and m.domain() == FREQ and np.isnan(m.delta())
        assert getattr(m, name)(*args) == 5  # poisoned AND complex / frequency now: the domain check comes first
        m = bd.DspMat(rows=3, row_len=0, dtype=dtype)  # rows without points
        assert getattr(m, name)(*args) == 9
        m = bd.DspMat(z, is_complex=True)
        assert getattr(m, name)(*args) == 5 and m.is_complex() and m.domain() == FREQ and np.isnan(m.delta())
        m = bd.DspMat(z[:, :9], domain=FREQ)
        assert getattr(m, name)(*args) == 5
        m = bd.DspMat(rows=0, row_len=9, dtype=dtype)
        assert getattr(m, name)(*args) == 0 and m.is_complex() and m.domain() == FREQ and m.row_len() == 0
        # the vector codes in the same order
        assert getattr(bd.DspVec(z[0]), name)(*args) == 9
        assert getattr(bd.DspVec(z[0], is_complex=True), name)(*args) == 5
    for name, args in inverse:
        m = bd.DspMat(z, is_complex=True)  # time domain
        assert getattr(m, name)(*args) == 6 and m.is_complex() and m.domain() == FREQ and np.isnan(m.delta())
        m = bd.DspMat(z, domain=FREQ)  # real
        assert getattr(m, name)(*args) == 6
        m = bd.DspMat(rows=0, row_len=10, is_complex=True, domain=FREQ, dtype=dtype)
        assert getattr(m, name)(*args) == 0 and not m.is_complex() and m.domain() == TIME and m.row_len() == 0
        m = bd.DspMat(rows=3, row_len=0, is_complex=True, domain=FREQ, dtype=dtype)  # as the vector on an empty vector
        v = bd.DspVec(np.zeros(0, dtype), is_complex=True, domain=FREQ)
        assert getattr(m, name)(*args) == getattr(v, name)(*args) == 0
        assert m.is_complex() == v.is_complex() and m.domain() == v.domain() and m.row_len() == len(v) == 0
    m = bd.DspMat(z, is_complex=True)
    assert m.to_complex() == -1 and np.isnan(m.delta()) and m.row_len() == 0
    m = bd.DspMat(z)  # real time data has no spectrum to mirror
    assert m.mirror() == -1 and np.isnan(m.delta())
    for kw in (dict(rows=0, row_len=10), dict(rows=3, row_len=0)):
        m = bd.DspMat(is_complex=True, domain=FREQ, dtype=dtype, **kw)
        assert m.mirror() == 0 and m.row_len() == 0 and m.is_complex() and m.domain() == FREQ
        m = bd.DspMat(dtype=dtype, **kw)
        assert m.to_complex() == 0 and m.row_len() == 0 and m.is_complex()


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("dtype", DTYPES)
def test_windowed_sfft_magnitude_peak_per_row(bd, dtype):
    """windowed_sfft(HANN) -> magnitude -> statistics()["max_index"]: the peak bin of every sampled row equals the
    same chain on the vector path"""
    n, rows = 1001, 257
    x = real_rows(n, rows, dtype)
    m = bd.DspMat(x)
    assert m.windowed_sfft(HANN) == 0 and m.magnitude() == 0
    assert not m.is_complex() and m.row_len() == n // 2 + 1
    peaks = m.statistics()["max_index"]
    assert peaks.shape == (rows,)
    for r in sample_rows(rows):
        v = bd.DspVec(x[r])
        assert v.windowed_sfft(HANN) == 0 and v.magnitude() == 0
        assert peaks[r] == v.statistics()["max_index"], r
