"""DspMat.convolve (built-in impulse responses and Python callables), convolve_complex, interpolate_lin and
interpolate_hermite: sampled rows against the CPU oracle and against the vector path on the same row; row isolation,
determinism, the codes, and the README's pipeline snippet.

Tolerances.  convolve: the project's bound for this operation (test_gpu_parity.py, test_convolve_with_function), rel-L2
< 2e-6 (f32) / 1e-12 (f64) against the float64 oracle.  Plain ascending f32 summation of these inputs
(fill_uniform(-10, 10), at most 2 * 300 + 1 weights) stays at or below 7.2e-7 against the oracle on the CPU, so the bound
has a 2.7x margin; longer direct sums are not part of this file.  Against the vector path: twice the bound (each side is
within the bound of the same reference), and bit-equal where the vector path is a direct sum as well (2L + 1 > points:
the same expressions over ascending k, both objects built without FMA contraction).  The interpolations are bit-equal to
the oracle in the matrix's precision and to the vector path."""
import os
import re

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.float32, np.float64)
TIME, FREQ = 0, 1
SINC, RAISED_COSINE = 0, 1
FUNCTIONS = ((SINC, 0.0), (RAISED_COSINE, 0.35))
WG = 256  # lanes of a workgroup: rows shorter than this share one


def direct_max_taps():
    with open(os.path.join(ROOT, "basic_dsp_amd", "csrc", "capi.cpp")) as f:
        return int(re.search(r"constexpr size_t MAT_CONV_DIRECT_MAX_TAPS = (\d+);", f.read()).group(1))


K = direct_max_taps()
# (rows, points, L, ratio)
CONV_CASES = [(3, 1, 5, 0.3), (3, 2, 1, 0.3), (5, 7, 20, 0.3), (4, 8, 8, 0.25), (257, 100, 3, 0.25), (257, 100, 100, 0.25),
              (33, 255, 127, 0.25), (33, 257, 257, 0.05), (9, 1000, 12, 0.25), (9, 1000, 64, 0.25), (5, 1025, 300, 0.1),
              (70000, 3, 1, 0.3),
              (9, 1000, (K - 1) // 2, 0.25), (9, 1000, (K - 1) // 2 + 1, 0.25),  # the two sides of the crossover
              (3, 5000, 12, 0.25)]  # the vector path hands this one to the block kernel
# (rows, n, factor, delay)
INTERP_CASES = [(3, 1, 2.0, 0.0), (3, 2, 3.0, 0.0), (5, 3, 0.5, 0.0), (5, 7, 4.0, 0.0), (5, 7, 3.0, 0.0), (4, 5, 3.0, 0.25),
                (257, 100, 2.5, 0.0), (9, 513, 0.5, 0.0), (9, 1000, 2.5, 0.0), (5, 2000, 3.0, 0.25), (70000, 3, 2.0, 0.0)]


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def tol_of(dtype):
    return 2e-6 if dtype == np.float32 else 1e-12


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def sample_rows(rows, row_elems):
    """the first and the last row and the rows on both sides of workgroup boundaries: the first two and the last
    boundary between the row groups that share a workgroup (short rows), or between runs of 256 outputs"""
    if rows <= 9:
        return list(range(rows))
    per = max(1, WG // row_elems)
    s = {0, rows - 1}
    for b in (per, 2 * per, (rows - 1) // per * per):
        s |= {b - 1, b}
    return sorted(r for r in s if 0 <= r < rows)


_inputs = {}


def rows_of(rows, scalars, dtype):
    """the matrix of a shape, made once and never changed"""
    key = (rows, scalars, dtype)
    if key not in _inputs:
        x = orc.fill_uniform(rows * scalars, 20161018 + 31 * scalars + rows, -10, 10, dtype).reshape(rows, scalars)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


_refs = {}


def conv_ref(x, rows, points, L, ratio, cplx, dtype, fid, ro, r):
    key = (rows, points, L, ratio, cplx, dtype, fid, r)
    if key not in _refs:
        _refs[key] = orc.convolve_function(x[r].astype(np.float64), cplx, fid, ro, ratio, L)
    return _refs[key]


# ------------------------------------------------------------------ convolve with the built-in functions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("rows,points,L,ratio", CONV_CASES)
def test_convolve_against_oracle_and_vector(bd, rows, points, L, ratio, cplx, dtype):
    tol = tol_of(dtype)
    x = rows_of(rows, points * (2 if cplx else 1), dtype)
    vector_is_direct = 2 * min(L, points) + 1 > points
    for fid, ro in FUNCTIONS:
        m = bd.DspMat(x, is_complex=cplx, delta=0.5)
        assert m.convolve(fid, ratio, L, rolloff=ro) == 0
        assert m.is_complex() == cplx and m.domain() == TIME and m.rows() == rows and m.row_points() == points
        assert m.delta() == dtype(0.5)
        got = m.data()
        for r in sample_rows(rows, points):
            e = rel_l2(got[r], conv_ref(x, rows, points, L, ratio, cplx, dtype, fid, ro, r))
            print("convolve", rows, points, L, cplx, dtype.__name__, fid, "row", r, "rel-L2", e)
            assert e < tol, (fid, r, e)
            v = bd.DspVec(x[r], is_complex=cplx, delta=0.5)
            assert v.convolve(fid, ratio, L, rolloff=ro) == 0
            assert len(v) == m.row_len() and v.delta() == m.delta()
            if vector_is_direct:
                assert np.array_equal(got[r], v.data()), (fid, r)
            else:
                e = rel_l2(got[r], v.data())
                assert e < 2 * tol, (fid, r, "vector", e)


# ------------------------------------------------------------------ callback forms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("rows,points,L,ratio", [(5, 7, 20, 0.3), (9, 1000, 12, 0.25), (9, 1000, 64, 0.25)])
def test_python_sinc_equals_the_builtin(bd, rows, points, L, ratio, cplx, dtype):
    tol = tol_of(dtype)
    x = rows_of(rows, points * (2 if cplx else 1), dtype)
    calls = []

    def sinc(t):
        calls.append(t)
        return float(np.sinc(t))
    m = bd.DspMat(x, is_complex=cplx)
    assert m.convolve(sinc, ratio, L) == 0
    assert len(calls) == 2 * min(L, points) + 1  # sampled once for all rows
    b = bd.DspMat(x, is_complex=cplx)
    assert b.convolve(SINC, ratio, L) == 0
    got, builtin = m.data(), b.data()
    for r in range(rows):
        assert rel_l2(got[r], builtin[r]) < tol, r
        assert rel_l2(got[r], conv_ref(x, rows, points, L, ratio, cplx, dtype, SINC, 0.0, r)) < tol, r
    v = bd.DspVec(x[rows - 1], is_complex=cplx)
    assert v.convolve(lambda t: float(np.sinc(t)), ratio, L) == 0
    assert rel_l2(got[rows - 1], v.data()) < 2 * tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,points,L,ratio", [(5, 7, 20, 0.3), (257, 100, 3, 0.25), (9, 1000, 12, 0.25),
                                                 (9, 1000, 64, 0.25)])
def test_convolve_complex_callback(bd, rows, points, L, ratio, dtype):
    """f(x) = sinc(x) * (1 + 0.5j): (1 + 0.5j) times the result of the real function"""
    tol = tol_of(dtype)
    x = rows_of(rows, 2 * points, dtype)
    m = bd.DspMat(x, is_complex=True, delta=0.5)
    assert m.convolve_complex(lambda t: np.sinc(t) * (1 + 0.5j), ratio, L) == 0
    assert m.is_complex() and m.domain() == TIME and m.row_points() == points and m.delta() == dtype(0.5)
    got = m.data()
    for r in sample_rows(rows, points):
        ref = conv_ref(x, rows, points, L, ratio, True, dtype, SINC, 0.0, r).view(np.complex128) * (1 + 0.5j)
        e = rel_l2(got[r], ref.view(np.float64))
        print("convolve_complex", rows, points, L, dtype.__name__, "row", r, "rel-L2", e)
        assert e < tol, (r, e)
    v = bd.DspVec(x[rows - 1], is_complex=True)
    assert v.convolve_complex(lambda t: np.sinc(t) * (1 + 0.5j), ratio, L) == 0
    assert rel_l2(got[rows - 1], v.data()) < 2 * tol


# ------------------------------------------------------------------ interpolate_lin / interpolate_hermite
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,n,factor,delay", INTERP_CASES)
def test_interpolations_are_bit_equal(bd, rows, n, factor, delay, dtype):
    x = rows_of(rows, n, dtype)
    dest = orc.interpolate_real_len(n, factor, dtype)
    for name, oracle in (("interpolate_lin", orc.interpolate_lin), ("interpolate_hermite", orc.interpolate_hermite)):
        m = bd.DspMat(x, delta=0.5)
        assert getattr(m, name)(factor, delay) == 0, name
        assert not m.is_complex() and m.domain() == TIME and m.rows() == rows and m.delta() == dtype(0.5)
        assert m.row_len() == dest, name
        got = m.data()
        for r in sample_rows(rows, dest):
            ref = oracle(x[r], factor, delay)
            assert np.isfinite(ref).all()
            assert np.array_equal(got[r], ref), (name, r)
            v = bd.DspVec(x[r], delta=0.5)
            assert getattr(v, name)(factor, delay) == 0
            assert len(v) == dest and np.array_equal(got[r], v.data()), (name, r, "vector")


# ------------------------------------------------------------------ row isolation, determinism
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_see_each_other_and_calls_repeat(bd, dtype):
    cases = (("convolve", (RAISED_COSINE, 0.25, 3, 0.35), 257, 100, False), ("convolve", (SINC, 0.25, 100), 257, 100, True),
             ("convolve", (SINC, 0.25, 12), 33, 1000, True), ("convolve", (SINC, 0.25, 64), 33, 1000, True),
             ("interpolate_lin", (2.5, 0.0), 257, 100, False), ("interpolate_hermite", (2.5, 0.25), 257, 100, False))
    for name, args, rows, points, cplx in cases:
        a = rows_of(rows, points * (2 if cplx else 1), dtype)

        def run(data):
            m = bd.DspMat(data, is_complex=cplx)
            assert getattr(m, name)(*args) == 0, name
            return m.data()
        first = run(a)
        assert np.array_equal(first, run(a)), (name, "two calls on equal input differ")
        b = a.copy()
        changed = 17
        b[changed] = -b[changed] + 1
        second = run(b)
        keep = np.arange(rows) != changed
        assert np.array_equal(first[keep], second[keep]), name
        assert not np.array_equal(first[changed], second[changed]), name


# ------------------------------------------------------------------ codes
@pytest.mark.parametrize("dtype", DTYPES)
def test_codes(bd, dtype):
    z = np.ones((3, 10), dtype)
    cfn = lambda t: np.sinc(t) * (1 + 0.5j)  # noqa: E731
    rfn = lambda t: float(np.sinc(t))  # noqa: E731
    forms = (("convolve", (SINC, 0.25, 2)), ("convolve", (RAISED_COSINE, 0.25, 2, 0.35)), ("convolve", (rfn, 0.25, 2)),
             ("convolve_complex", (cfn, 0.25, 2)))
    for name, args in forms:
        m = bd.DspMat(z, is_complex=True, domain=FREQ)  # a frequency-domain matrix is poisoned by every form
        assert getattr(m, name)(*args) == -1, name
        assert m.row_len() == 0 and np.isnan(m.delta()) and m.domain() == FREQ
        assert getattr(m, name)(*args) == -1  # and stays poisoned
        for kw in (dict(rows=0, row_len=10), dict(rows=3, row_len=0)):
            m = bd.DspMat(is_complex=True, dtype=dtype, delta=0.5, **kw)
            assert getattr(m, name)(*args) == 0, (name, kw)
            assert m.row_len() == 0 and m.is_complex() and m.domain() == TIME and m.delta() == dtype(0.5)
    m = bd.DspMat(z, domain=FREQ)  # real and frequency domain
    assert m.convolve(SINC, 0.25, 2) == -1
    m = bd.DspMat(z)  # a real matrix is poisoned by convolve_complex, as the vector
    assert m.convolve_complex(cfn, 0.25, 2) == -1 and np.isnan(m.delta()) and m.row_len() == 0
    assert bd.DspVec(z[0]).convolve_complex(cfn, 0.25, 2) == -1
    m = bd.DspMat(z)  # ... but convolved by the real forms
    assert m.convolve(SINC, 0.25, 2) == 0 and m.convolve(rfn, 0.25, 2) == 0 and m.row_len() == 10
    for name in ("interpolate_lin", "interpolate_hermite"):
        m = bd.DspMat(z, is_complex=True)  # a complex matrix is poisoned by both interpolations
        assert getattr(m, name)(2.0) == -1 and np.isnan(m.delta()) and m.row_len() == 0, name
        assert getattr(m, name)(2.0) == -1
        assert getattr(bd.DspVec(z[0], is_complex=True), name)(2.0) == -1
        for kw in (dict(rows=0, row_len=10), dict(rows=3, row_len=0)):
            m = bd.DspMat(dtype=dtype, delta=0.5, **kw)
            assert getattr(m, name)(2.0) == 0 and m.row_len() == 0 and not m.is_complex() and m.delta() == dtype(0.5)
        m = bd.DspMat(z, domain=FREQ, delta=0.5)  # the domain is neither checked nor changed, as in the vector
        assert getattr(m, name)(2.0) == 0 and m.domain() == FREQ and m.row_len() == 19 and m.delta() == dtype(0.5)
    m = bd.DspMat(z, is_complex=True)
    assert m.to_complex() == -1  # poisoned by another call: every new method reports it and changes nothing
    for name, args in forms + (("interpolate_lin", (2.0,)), ("interpolate_hermite", (2.0,))):
        assert getattr(m, name)(*args) == -1 and m.row_len() == 0 and np.isnan(m.delta()), name


# ------------------------------------------------------------------ end to end
def test_readme_snippet_runs(bd):
    """the pipeline snippet of the README (correlate -> smooth -> phase -> unwrap -> diff -> resample), with 64 rows in
    place of 16 384"""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "interpolate_hermite" in b]
    assert len(blocks) == 1
    code = blocks[0]
    assert "16384" in code and "pulses.convolve(" in code
    env = {}
    exec("import numpy as np\nfrom basic_dsp_amd import DspVec, DspMat, vector as V\n" + code.replace("16384", "64"), env)
    pulses = env["pulses"]
    assert pulses.rows() == 64 and not pulses.is_complex() and pulses.row_len() > 0
    assert np.isfinite(pulses.data()).all()
