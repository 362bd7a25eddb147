"""DspMat's math family, reverse, multiply_complex_exponential, add / sub / mul / div_smaller (matrix or vector operand)
and the part getters / setters: every row against the CPU oracle and bit for bit against the vector path on that row
(get_row -> the DspVec method -> data()); the codes, empty and poisoned matrices, row isolation, determinism, and the
README's mixer snippet.

Tolerances are the ones the vector tests of the same operation in test_gpu_parity.py use:
  * math family (test_math_family): max |got - ref| / (|ref| + 1) < tol = 3e-6 (f32) / 1e-13 (f64) for the functions
    without an argument, 4 * tol for the ones with one; complex matrices rel-L2 < ctol = 2e-5 / 1e-12; the input ranges
    _MATH_DOMAINS, _MATH_ARGS and (-3, 3) for complex data are copied from there;
  * multiply_complex_exponential (test_multiply_complex_exponential): rel-L2 < 2e-7 / 1e-14 against the exact float64
    phase, here per row (the rows are shorter than that test's 3000 points);
  * magnitude, phase (test_complex_to_real_maps): 4 eps relative and absolute against the oracle in the matrix's precision;
  * get_mag_phase / set_mag_phase (test_pairs_split_merge_map): rel-L2 < tol = 2e-6 / 1e-14 for the magnitudes, 4 * tol
    absolute for the phases and rel-L2 < 4 * tol for set_mag_phase;
  * everything else is bit-exact."""
import os
import re

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.float32, np.float64)
TIME, FREQ = 0, 1

# test_gpu_parity.py, _MATH_DOMAINS / _MATH_ARGS: real input ranges that keep the function real-valued
_MATH_DOMAINS = {
    "sqrt": (0.0, 50.0), "square": (-10, 10), "ln": (1e-3, 50.0), "exp": (-10, 10), "sin": (-10, 10), "cos": (-10, 10),
    "tan": (-1.4, 1.4), "asin": (-0.99, 0.99), "acos": (-0.99, 0.99), "atan": (-10, 10), "sinh": (-8, 8),
    "cosh": (-8, 8), "tanh": (-8, 8), "asinh": (-10, 10), "acosh": (1.01, 50.0), "atanh": (-0.99, 0.99),
    "abs": (-10, 10), "ln_approx": (1e-3, 50.0), "exp_approx": (-10, 10), "sin_approx": (-10, 10),
    "cos_approx": (-10, 10)}
_MATH_ARGS = {"powf": ((0.1, 10.0), 2.5), "root": ((0.1, 10.0), 3.0), "log": ((1e-3, 50.0), 10.0),
              "expf": ((-3, 3), 10.0), "log_approx": ((1e-3, 50.0), 10.0),
              "expf_approx": ((-3, 3), 10.0), "powf_approx": ((0.1, 10.0), 2.5)}   # (wrap is not part of this family)
_COMPLEX_MATH0 = ("sqrt", "square", "ln", "exp", "sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh",
                  "asinh", "acosh", "atanh")
_COMPLEX_MATH1 = (("powf", 2.5), ("root", 3.0), ("log", 10.0), ("expf", 7.0))
_REAL_ONLY0 = ("abs", "ln_approx", "exp_approx", "sin_approx", "cos_approx")
_REAL_ONLY1 = ("log_approx", "expf_approx", "powf_approx")

MATH_REAL_SHAPES = [(3, 1), (3, 5), (5, 7), (257, 100), (5, 1025)]
MATH_COMPLEX_SHAPES = [(3, 3), (5, 1025)]
CEXP_SHAPES = [(3, 1), (3, 2), (5, 3), (4, 127), (4, 128), (4, 129), (4, 255), (4, 256), (4, 257), (257, 100), (9, 1025),
               (70000, 3)]
REVERSE_SHAPES = CEXP_SHAPES + [(1, 4097)]
# (rows, row points, operand points)
SMALLER_CASES = [(3, 6, 2), (3, 6, 3), (5, 12, 1), (5, 7, 7), (257, 100, 25), (9, 1024, 256), (70000, 4, 2)]
SMALLER = ("add_smaller", "sub_smaller", "mul_smaller", "div_smaller")
PART_SHAPES = [(3, 1), (5, 7), (257, 100), (5, 1025)]
GETTERS = (("get_real", 2), ("get_imag", 3), ("get_magnitude", 0), ("get_magnitude_squared", 1), ("get_phase", 4))


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def _oracle_math(x, cplx, name, arg):   # test_gpu_parity.py, _oracle_math
    key = {"ln_approx": "ln", "exp_approx": "exp", "sin_approx": "sin", "cos_approx": "cos", "log_approx": "log"}.get(name, name)
    if name == "root":
        key, arg = "powf", 1.0 / arg
    return orc.math(x.astype(np.float64), cplx, key, arg)


def _vector_path_rows(rows):
    """rows whose result is compared bit for bit with the vector path (test_gpu_mat_basic.py): every row up to 300
    rows, else the first 16, the last 16 and 16 spread in between"""
    if rows <= 300:
        return list(range(rows))
    return sorted(set(range(16)) | set(range(rows - 16, rows)) | set(np.linspace(0, rows - 1, 16).astype(int).tolist()))


def _fill(rows, scalars, seed, dtype, lo=-10, hi=10):
    x = orc.fill_uniform(rows * scalars, seed, lo, hi, dtype).reshape(rows, scalars)
    x.setflags(write=False)
    return x


def _seed(rows, pts, salt=0):
    return 20161018 + 977 * rows + 31 * pts + salt


def _mat(bd, x, cplx, **kw):
    if x.size == 0:
        return bd.DspMat(rows=x.shape[0], row_len=x.shape[1], is_complex=cplx, dtype=x.dtype, **kw)
    return bd.DspMat(x, is_complex=cplx, **kw)


def _dest(bd, dtype, cplx=False, delta=0.125):
    """a destination of another shape and delta than anything a getter produces"""
    return bd.DspMat(rows=2, row_len=4, is_complex=cplx, dtype=dtype, delta=delta)


def _poisoned(m):
    return m.row_len() == 0 and np.isnan(m.delta())


def _as_real(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return np.ascontiguousarray(a.astype(np.complex128)).view(np.float64)
    return a.astype(np.float64)


def rel_l2(got, ref):
    got, ref = _as_real(got).ravel(), _as_real(ref).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _vector_rows(bd, x, cplx, rows, call, **kw):
    """the vector path: row r as a DspVec, `call` on it, downloaded"""
    out = {}
    for r in rows:
        v = bd.DspVec(np.array(x[r]), is_complex=cplx, **kw)
        code = call(v)
        assert code == 0, (r, code)
        out[r] = v.data()
    return out


def _check_vector_path(bd, got, x, cplx, call, what, **kw):
    rows = _vector_path_rows(x.shape[0])
    ref = _vector_rows(bd, x, cplx, rows, call, **kw)
    bad = [r for r in rows if not _bits_equal(got[r], ref[r])]
    assert not bad, (what, "rows that differ from the vector path", bad[:8])


# ---------------------------------------------------------------------------------------------- math family
def _math_calls(cplx):
    if cplx:
        return [(n, None, False) for n in _COMPLEX_MATH0] + [(n, a, True) for n, a in _COMPLEX_MATH1]
    return [(n, None, False) for n in _MATH_DOMAINS] + [(n, a, True) for n, (_, a) in _MATH_ARGS.items()]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,pts,cplx", [s + (False,) for s in MATH_REAL_SHAPES] + [s + (True,) for s in MATH_COMPLEX_SHAPES])
def test_math_family_equals_the_vector_path_and_the_oracle(bd, rows, pts, cplx, dtype):
    tol = 3e-6 if dtype == np.float32 else 1e-13
    ctol = 2e-5 if dtype == np.float32 else 1e-12
    e = 2 if cplx else 1
    calls = _math_calls(cplx)
    assert len(calls) == (20 if cplx else 28)
    for k, (name, arg, has_arg) in enumerate(calls):
        if cplx:
            lo, hi = -3, 3
        else:
            lo, hi = _MATH_ARGS[name][0] if has_arg else _MATH_DOMAINS[name]
        x = _fill(rows, pts * e, _seed(rows, pts, 100 + k), dtype, lo, hi)
        args = (arg,) if has_arg else ()
        m = _mat(bd, x, cplx, delta=0.5)
        assert getattr(m, name)(*args) == 0, name
        assert m.is_complex() == cplx and m.rows() == rows and m.row_len() == pts * e and m.delta() == 0.5, name
        got = m.data()
        _check_vector_path(bd, got, x, cplx, lambda v: getattr(v, name)(*args), name)
        ref = _oracle_math(x.reshape(-1), cplx, name, arg if has_arg else 0.0).reshape(rows, pts * e)
        if cplx:
            err = rel_l2(got, ref)
            assert err < ctol, (name, err)
        else:
            err = float(np.max(np.abs(got - ref) / (np.abs(ref) + 1.0)))
            assert err < (tol * 4 if has_arg else tol), (name, err)


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_only_math_poisons_a_complex_matrix(bd, dtype):
    x = _fill(5, 14, 7, dtype, -3, 3)
    for name in _REAL_ONLY0 + _REAL_ONLY1:
        m = _mat(bd, x, True)
        args = (2.0,) if name in _REAL_ONLY1 else ()
        assert getattr(m, name)(*args) == -1, name
        assert _poisoned(m) and m.rows() == 5 and m.is_complex(), name
        assert getattr(m, name)(*args) == -1, name   # and stays poisoned


# ---------------------------------------------------------------------------------------------- multiply_complex_exponential
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("a", [0.02, -0.02])
@pytest.mark.parametrize("rows,pts", CEXP_SHAPES)
def test_multiply_complex_exponential(bd, rows, pts, a, dtype):
    b, delta = 0.3, 0.5
    x = _fill(rows, 2 * pts, _seed(rows, pts, 1), dtype)
    m = _mat(bd, x, True, delta=delta)
    assert m.multiply_complex_exponential(a, b) == 0
    assert m.is_complex() and m.rows() == rows and m.row_points() == pts and m.delta() == delta and m.domain() == TIME
    got = m.data()
    # a and b are multiplied by delta in T first (complex_ops.rs:83-84); the phase restarts in every row
    ad, bdl = float(dtype(a) * dtype(delta)), float(dtype(b) * dtype(delta))
    k = np.arange(pts)
    ref = x.astype(np.float64).view(np.complex128) * np.exp(1j * (ad * k + bdl))[None, :]
    diff = got.astype(np.float64).view(np.complex128) - ref
    err = np.linalg.norm(diff, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    worst = int(np.argmax(err))
    print("multiply_complex_exponential %s %dx%d a=%g: worst row %d rel-L2 %.3e" % (np.dtype(dtype).name, rows, pts, a, worst, err[worst]))
    assert err[worst] < (2e-7 if dtype == np.float32 else 1e-14), (worst, err[worst])
    _check_vector_path(bd, got, x, True, lambda v: v.multiply_complex_exponential(a, b), "multiply_complex_exponential",
                       delta=delta)


@pytest.mark.parametrize("dtype", DTYPES)
def test_multiply_complex_exponential_poisons_a_real_matrix(bd, dtype):
    m = _mat(bd, _fill(3, 8, 2, dtype), False)
    assert m.multiply_complex_exponential(0.02, 0.3) == -1 and _poisoned(m) and m.rows() == 3


# ---------------------------------------------------------------------------------------------- reverse
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("rows,pts", REVERSE_SHAPES)
def test_reverse(bd, rows, pts, cplx, dtype):
    e = 2 if cplx else 1
    x = _fill(rows, pts * e, _seed(rows, pts, 2), dtype)
    m = _mat(bd, x, cplx, delta=0.25, domain=FREQ)
    assert m.reverse() == 0
    assert m.is_complex() == cplx and m.rows() == rows and m.row_points() == pts
    assert m.delta() == 0.25 and m.domain() == FREQ
    got = m.data()
    ref = x.reshape(rows, pts, e)[:, ::-1, :].reshape(rows, pts * e)   # whole elements: pairs for complex rows
    assert _bits_equal(got, ref)
    assert m.reverse() == 0 and _bits_equal(m.data(), x)              # two reverses restore the input


# ---------------------------------------------------------------------------------------------- *_smaller
def _tiled_oracle(x, y_rows, cplx, op):
    """orc.binary(row, np.tile(operand_row, ...)) for every row; for the many-row shape on the flat data (the same
    arithmetic on the same elements, without 70 000 calls)"""
    rows, rl = x.shape
    reps = rl // y_rows.shape[1]
    tiled = np.tile(y_rows, (1, reps))
    if tiled.shape[0] == 1:
        tiled = np.broadcast_to(tiled, x.shape)
    if rows > 300:
        code, ref = orc.binary(x.reshape(-1), np.ascontiguousarray(tiled).reshape(-1), cplx, op)
        assert code == 0
        return ref.reshape(rows, rl)
    out = np.empty_like(x)
    for r in range(rows):
        code, out[r] = orc.binary(x[r], tiled[r], cplx, op)
        assert code == 0
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("rows,pts,ypts", SMALLER_CASES)
def test_smaller_with_a_matrix_and_with_a_vector_operand(bd, rows, pts, ypts, cplx, dtype):
    e = 2 if cplx else 1
    x = _fill(rows, pts * e, _seed(rows, pts, 3), dtype)
    ym = _fill(rows, ypts * e, _seed(rows, ypts, 4), dtype, 1, 10)   # operands from (1, 10): div stays tame
    yv = _fill(1, ypts * e, _seed(1, ypts, 5), dtype, 1, 10)
    assert rows == 1 or not np.array_equal(ym[0], ym[1])
    other = _mat(bd, ym, cplx)
    vec = bd.DspVec(np.array(yv[0]), is_complex=cplx)
    for op, name in enumerate(SMALLER):
        m = _mat(bd, x, cplx)
        assert getattr(m, name)(other) == 0, name
        assert m.rows() == rows and m.row_len() == pts * e and m.is_complex() == cplx
        got = m.data()
        assert _bits_equal(got, _tiled_oracle(x, ym, cplx, op)), (name, "matrix operand")
        sel = _vector_path_rows(rows)
        ref = {r: None for r in sel}
        for r in sel:
            v = bd.DspVec(np.array(x[r]), is_complex=cplx)
            assert getattr(v, name)(bd.DspVec(np.array(ym[r]), is_complex=cplx)) == 0
            ref[r] = v.data()
        assert not [r for r in sel if not _bits_equal(got[r], ref[r])], (name, "matrix operand, vector path")
        m = _mat(bd, x, cplx)
        assert getattr(m, name)(vec) == 0, name
        got = m.data()
        assert _bits_equal(got, _tiled_oracle(x, yv, cplx, op)), (name, "vector operand")
        _check_vector_path(bd, got, x, cplx, lambda v: getattr(v, name)(vec), name + " (vector operand)")
    assert _bits_equal(other.data(), ym) and _bits_equal(vec.data(), yv[0])   # the operands are only read


@pytest.mark.parametrize("dtype", DTYPES)
def test_smaller_codes(bd, dtype):
    x = _fill(2, 3, 11, dtype)
    for name in SMALLER:
        m = _mat(bd, x, False)
        # the period must divide the ROW: 2 rows x 3 points with a 2-point vector is 7 although 6 % 2 == 0
        assert getattr(m, name)(bd.DspVec(np.ones(2, dtype))) == 7, name
        assert getattr(m, name)(bd.DspVec(dtype=dtype, length=0)) == 7, name
        assert getattr(m, name)(_mat(bd, _fill(3, 3, 12, dtype, 1, 10), False)) == 7, name          # another row count
        assert getattr(m, name)(bd.DspMat(rows=2, row_len=0, dtype=dtype)) == 7, name                # empty operand rows
        assert getattr(m, name)(_mat(bd, _fill(2, 2, 13, dtype, 1, 10), False)) == 7, name          # 3 % 2 != 0
        assert _bits_equal(m.data(), x) and not _poisoned(m), name                                    # untouched
    # real against complex: the code add returns for the same pair (equal scalar lengths: the meta data check)
    xr = _fill(3, 6, 14, dtype)
    cm = _mat(bd, _fill(3, 6, 15, dtype, 1, 10), True)
    cv = bd.DspVec(np.array(_fill(1, 6, 16, dtype, 1, 10)[0]), is_complex=True)
    for name in SMALLER:
        m = _mat(bd, xr, False)
        want = _mat(bd, xr, False).add(cm)
        assert want == 2 and getattr(m, name)(cm) == want, name
        want = _mat(bd, xr, False).add(cv)
        assert want == 2 and getattr(m, name)(cv) == want, name
        other_domain = _mat(bd, _fill(3, 6, 17, dtype, 1, 10), False, domain=FREQ)
        assert getattr(m, name)(other_domain) == _mat(bd, xr, False).add(other_domain) == 2, name
        assert _bits_equal(m.data(), xr), name


# ---------------------------------------------------------------------------------------------- parts
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,pts", PART_SHAPES)
def test_getters(bd, rows, pts, dtype):
    eps = np.finfo(dtype).eps
    tol = 2e-6 if dtype == np.float32 else 1e-14
    x = _fill(rows, 2 * pts, _seed(rows, pts, 6), dtype)
    m = _mat(bd, x, True, delta=0.5, domain=FREQ)
    results = {}
    for name, kind in GETTERS:
        d = _dest(bd, dtype)
        assert getattr(m, name)(d) == 0, name
        assert not d.is_complex() and d.rows() == rows and d.row_len() == pts and d.delta() == 0.125 and d.domain() == TIME
        got = results[name] = d.data()
        ref = orc.complex_to_real(x.reshape(-1), kind).reshape(rows, pts)
        if name in ("get_real", "get_imag"):
            assert _bits_equal(got, ref), name
        else:
            np.testing.assert_allclose(got, ref, rtol=4 * eps, atol=4 * eps, err_msg=name)
        for r in _vector_path_rows(rows):
            dv = bd.DspVec(dtype=dtype, length=0)
            assert getattr(bd.DspVec(np.array(x[r]), is_complex=True), name)(dv) == 9   # the facade's convert_void
            assert _bits_equal(got[r], dv.data()), (name, r)
        assert _bits_equal(m.data(), x) and m.is_complex() and m.delta() == 0.5 and m.domain() == FREQ   # not consumed
    # the reference's matrix get_magnitude forwards to get_imag: not reproduced
    assert not np.array_equal(results["get_magnitude"], results["get_imag"])
    assert _bits_equal(results["get_real"], x[:, 0::2]) and _bits_equal(results["get_imag"], x[:, 1::2])

    a, b = _dest(bd, dtype), _dest(bd, dtype, delta=4.0)
    assert m.get_real_imag(a, b) == 0
    assert _bits_equal(a.data(), x[:, 0::2]) and _bits_equal(b.data(), x[:, 1::2])
    assert a.delta() == 0.125 and b.delta() == 4.0 and not a.is_complex() and not b.is_complex()
    assert m.get_mag_phase(a, b) == 0
    assert a.rows() == rows and a.row_len() == pts and b.rows() == rows and b.row_len() == pts
    mag, ph = orc.get_mag_phase(x.reshape(-1).astype(np.float64))
    gm, gp = a.data(), b.data()
    for r in range(rows):   # every row within the vector test's tolerance
        s = slice(r * pts, (r + 1) * pts)
        assert rel_l2(gm[r], mag[s]) < tol and np.max(np.abs(gp[r] - ph[s])) < tol * 4, r
    for r in _vector_path_rows(rows):
        v = bd.DspVec(np.array(x[r]), is_complex=True)
        va, vb = bd.DspVec(dtype=dtype, length=0), bd.DspVec(dtype=dtype, length=0)
        assert v.get_mag_phase(va, vb) == 9
        assert _bits_equal(gm[r], va.data()) and _bits_equal(gp[r], vb.data()), r
    assert _bits_equal(m.data(), x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,pts", PART_SHAPES)
def test_setters(bd, rows, pts, dtype):
    tol = 2e-6 if dtype == np.float32 else 1e-14
    x = _fill(rows, 2 * pts, _seed(rows, pts, 7), dtype)
    m = _mat(bd, x, True, delta=0.5)
    a, b = _dest(bd, dtype), _dest(bd, dtype)
    assert m.get_real_imag(a, b) == 0
    w = bd.DspMat(rows=1, row_len=2, is_complex=True, dtype=dtype, delta=0.5)
    assert w.set_real_imag(a, b) == 0
    assert w.is_complex() and w.rows() == rows and w.row_points() == pts and w.delta() == 0.5
    assert _bits_equal(w.data(), x)                               # get_real_imag -> set_real_imag restores the bits
    mag = _fill(rows, pts, _seed(rows, pts, 8), dtype, 0, 10)
    ph = _fill(rows, pts, _seed(rows, pts, 9), dtype, -3.1, 3.1)
    assert w.set_mag_phase(_mat(bd, mag, False), _mat(bd, ph, False)) == 0
    assert w.is_complex() and w.rows() == rows and w.row_points() == pts
    got = w.data()
    ref = orc.set_mag_phase(mag.reshape(-1).astype(np.float64), ph.reshape(-1).astype(np.float64)).reshape(rows, 2 * pts)
    for r in range(rows):
        assert rel_l2(got[r], ref[r]) < tol * 4, r
    for r in _vector_path_rows(rows):
        v = bd.DspVec(dtype=dtype, length=0, is_complex=True)
        assert v.set_mag_phase(bd.DspVec(np.array(mag[r])), bd.DspVec(np.array(ph[r]))) == 0
        assert _bits_equal(got[r], v.data()), r


@pytest.mark.parametrize("dtype", DTYPES)
def test_part_codes(bd, dtype):
    x = _fill(5, 14, 21, dtype)
    m = _mat(bd, x, True)
    # unequal shapes: 7, target untouched
    for name in ("set_real_imag", "set_mag_phase"):
        assert getattr(m, name)(_mat(bd, _fill(5, 7, 22, dtype), False), _mat(bd, _fill(5, 6, 23, dtype), False)) == 7
        assert getattr(m, name)(_mat(bd, _fill(5, 7, 22, dtype), False), _mat(bd, _fill(7, 5, 23, dtype), False)) == 7
        assert _bits_equal(m.data(), x)
    # a real source or a complex destination: destinations with rows() rows of length 0, code 0
    real = _mat(bd, x, False)
    for name, _ in GETTERS:
        d = _dest(bd, dtype)
        assert getattr(real, name)(d) == 0 and d.rows() == 5 and d.row_len() == 0 and d.delta() == 0.125, name
        d = _dest(bd, dtype, cplx=True)
        assert getattr(m, name)(d) == 0 and d.rows() == 5 and d.row_len() == 0, name
    for name in ("get_real_imag", "get_mag_phase"):
        a, b = _dest(bd, dtype), _dest(bd, dtype)
        assert getattr(real, name)(a, b) == 0 and (a.rows(), a.row_len(), b.rows(), b.row_len()) == (5, 0, 5, 0), name
        a, c = _dest(bd, dtype), _dest(bd, dtype, cplx=True)
        assert getattr(m, name)(a, c) == 0 and (a.rows(), a.row_len(), c.rows(), c.row_len()) == (5, 0, 5, 0), name
    assert _bits_equal(m.data(), x) and _bits_equal(real.data(), x)


# ---------------------------------------------------------------------------------------------- common
def _every_call(bd, dtype, cplx, rows, delta=1.0):
    """(name, call on a matrix) for every new in-place method that applies to a matrix of this number space; the
    operands of *_smaller hold one element per row and fit `rows` rows"""
    yl = 2 if cplx else 1
    other = bd.DspMat(np.full((rows, yl), 2.0, dtype), is_complex=cplx, delta=delta) if rows else \
        bd.DspMat(rows=0, row_len=yl, is_complex=cplx, dtype=dtype, delta=delta)
    vec = bd.DspVec(np.full(yl, 2.0, dtype), is_complex=cplx, delta=delta)
    calls = [(n, lambda m, n=n: getattr(m, n)()) for n in _COMPLEX_MATH0]
    calls += [(n, lambda m, n=n, a=a: getattr(m, n)(a)) for n, a in _COMPLEX_MATH1]
    if not cplx:
        calls += [(n, lambda m, n=n: getattr(m, n)()) for n in _REAL_ONLY0]
        calls += [(n, lambda m, n=n: getattr(m, n)(2.0)) for n in _REAL_ONLY1]
    calls.append(("reverse", lambda m: m.reverse()))
    if cplx:
        calls.append(("multiply_complex_exponential", lambda m: m.multiply_complex_exponential(0.02, 0.3)))
    for n in SMALLER:
        calls.append((n, lambda m, n=n: getattr(m, n)(other)))
        calls.append((n + " (vector)", lambda m, n=n: getattr(m, n)(vec)))
    return calls


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("rows,row_len", [(5, 0), (0, 10)])
def test_zero_rows_and_empty_rows(bd, rows, row_len, cplx, dtype):
    for name, call in _every_call(bd, dtype, cplx, rows, delta=0.5):
        m = bd.DspMat(rows=rows, row_len=row_len, is_complex=cplx, dtype=dtype, delta=0.5)
        assert call(m) == 0, name
        assert m.rows() == rows and m.row_len() == 0 and m.delta() == 0.5 and m.is_complex() == cplx, name
        assert m.data().shape == (rows, 0), name
    if cplx:
        m = bd.DspMat(rows=rows, row_len=row_len, is_complex=True, dtype=dtype)
        for name, _ in GETTERS:
            d = _dest(bd, dtype)
            assert getattr(m, name)(d) == 0 and d.rows() == rows and d.row_len() == 0, name
        a, b = _dest(bd, dtype), _dest(bd, dtype)
        assert m.get_real_imag(a, b) == 0 and m.get_mag_phase(a, b) == 0 and a.rows() == rows and b.row_len() == 0
        e1 = bd.DspMat(rows=rows, row_len=0, dtype=dtype)
        assert m.set_real_imag(e1, e1) == 0 and m.set_mag_phase(e1, e1) == 0
        assert m.rows() == rows and m.row_len() == 0 and m.is_complex()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", [False, True])
def test_a_poisoned_matrix_answers_minus_one(bd, cplx, dtype):
    def poisoned():
        m = bd.DspMat(_fill(3, 8, 31, dtype), is_complex=cplx)
        assert (m.wrap(1.0) if cplx else m.conj()) == -1 and _poisoned(m)
        return m
    for name, call in _every_call(bd, dtype, cplx, 3):
        m = poisoned()
        assert call(m) == -1, name
        assert _poisoned(m) and m.rows() == 3, name
    # an argument error comes first
    m = poisoned()
    wrong_rows = bd.DspMat(np.full((4, 2), 2.0, dtype), is_complex=cplx)
    for name in SMALLER:
        assert getattr(m, name)(wrong_rows) == 7, name
        assert getattr(m, name)(bd.DspVec(dtype=dtype, length=0, is_complex=cplx)) == 7, name
    a, b = _mat(bd, _fill(3, 4, 32, dtype), False), _mat(bd, _fill(3, 5, 33, dtype), False)
    for name in ("set_real_imag", "set_mag_phase"):
        assert getattr(m, name)(a, b) == 7, name
        assert getattr(m, name)(a, a) == -1 and _poisoned(m), name
    # a poisoned source: -1, destinations untouched
    keep = _fill(2, 4, 34, dtype)
    for name, _ in GETTERS:
        d = _mat(bd, keep, False, delta=0.125)
        assert getattr(m, name)(d) == -1 and _bits_equal(d.data(), keep) and d.delta() == 0.125, name
    for name in ("get_real_imag", "get_mag_phase"):
        d1, d2 = _mat(bd, keep, False), _mat(bd, keep, False)
        assert getattr(m, name)(d1, d2) == -1 and _bits_equal(d1.data(), keep) and _bits_equal(d2.data(), keep), name


def _row_aware_calls(bd, dtype, cplx, rows, pts):
    e = 2 if cplx else 1
    other = _mat(bd, _fill(rows, (pts // 5) * e, 41, dtype, 1, 10), cplx)
    vec = bd.DspVec(np.array(_fill(1, (pts // 5) * e, 42, dtype, 1, 10)[0]), is_complex=cplx)
    calls = [("reverse", lambda m: m.reverse()), ("sin", lambda m: m.sin()), ("powf", lambda m: m.powf(2.5)),
             ("mul_smaller", lambda m: m.mul_smaller(other)), ("div_smaller (vector)", lambda m: m.div_smaller(vec))]
    if cplx:
        calls.append(("multiply_complex_exponential", lambda m: m.multiply_complex_exponential(0.02, 0.3)))

        def mag(m):
            d = _dest(bd, dtype)
            code = m.get_magnitude(d)
            m._parts = d.data()
            return code
        calls.append(("get_magnitude", mag))
    return calls


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", [False, True])
def test_row_isolation_and_determinism(bd, cplx, dtype):
    rows, pts, e = 40, 100, 2 if cplx else 1   # 40 x 100: two rows and a part of a third share a workgroup
    x = _fill(rows, pts * e, 43, dtype, 0.5, 3)
    y = np.array(x)
    y[17] = _fill(1, pts * e, 44, dtype, 0.5, 3)[0]
    for name, call in _row_aware_calls(bd, dtype, cplx, rows, pts):
        outs = []
        for src in (x, x, y):
            m = _mat(bd, src, cplx)
            assert call(m) == 0, name
            outs.append(m._parts if name.startswith("get_") else m.data())
        assert _bits_equal(outs[0], outs[1]), (name, "two runs differ")
        changed = [r for r in range(rows) if not _bits_equal(outs[0][r], outs[2][r])]
        assert changed == [17], (name, changed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_readme_mixer_snippet(bd, dtype):
    """the README's snippet (mix every row down, transform, dB) as written, on 8 rows of 256 points: row r holds a tone
    r bins above f0, so its strongest dB bin is r bins above the centre of the shifted spectrum"""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "multiply_complex_exponential" in b]
    assert len(blocks) == 1
    code = blocks[0]
    assert "pulses.multiply_complex_exponential(-2 * np.pi * f0, 0.0) == 0" in code
    assert "pulses.fft() == 0 and pulses.magnitude() == 0" in code
    assert "pulses.log(10.0) == 0 and pulses.scale(20.0) == 0" in code
    rows, n, f0 = 8, 256, 32 / 256
    k = np.arange(n)
    tones = np.exp(2j * np.pi * (f0 + np.arange(rows)[:, None] / n) * k[None, :])
    noise = orc.fill_uniform(rows * 2 * n, 51, -0.01, 0.01, np.float64).view(np.complex128).reshape(rows, n)
    z = (tones + noise).astype(np.complex64 if dtype == np.float32 else np.complex128)
    env = {"np": np, "f0": f0, "pulses": bd.DspMat(z)}
    exec(code, env)
    pulses = env["pulses"]
    assert not pulses.is_complex() and pulses.rows() == rows and pulses.row_len() == n
    db = pulses.data()
    assert np.isfinite(db).all()
    assert list(np.argmax(db, axis=1)) == [n // 2 + r for r in range(rows)]
    assert np.all(np.abs(db.max(axis=1) - 20 * np.log10(n)) < 0.1)   # a unit tone of n points: 20 log10(n) dB
