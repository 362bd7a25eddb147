"""matmul: the product of two DspMat on the device, a . b and a . b^H, through the Python function and the C ABI.

Reference: the product of the SAME f32 / f64 inputs in numpy one precision up -- complex128 / float64 for f32,
np.longdouble (four real products per complex one) for f64.  With eps = np.finfo(dtype).eps every output element must
satisfy

    |out - ref| <= (2 K + 4) eps (|A| . |B|)[i, j]

with |A| . |B| the product of the element-wise moduli.  The bound is order-independent (a sum of K products has error
gamma_K sum |a| |b|; a complex component is a sum of 2 K real products, gamma_2K ~ K eps; the factor 2 covers the
modulus of two components; + 4 covers K = 0 and K = 1), so it holds for any chunking and tile order and no path has a
tolerance of its own; it is relative to sum |a| |b|, not to |ref|, so cancelling inputs are fair game.  Where the bound
is 0 the output must be 0.

Inputs are seeded, with mixed signs, magnitudes spread over four decades and about 2 % exact zeros.  The shapes and the
path each must take are tests/mat_mul_shapes.txt; tests/host_sim/sim_mat_mul.cpp (run by tests/test_mat_mul_abi.py)
checks every line of it against the dispatch rule.  Worst |out - ref| / bound measured on an MI355X, per path:
streaming 0.15 (f32) / 0.16 (f64); tiled 0.16 / 0.17; split 0.012 / 0.015 (the test prints them)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME, FREQ = 0, 1
VARIANTS = [(np.float32, True), (np.float32, False), (np.float64, True), (np.float64, False)]
VARIANT_IDS = ["f32-complex", "f32-real", "f64-complex", "f64-real"]
TRANSFORM_TOL = {np.float32: 1e-6, np.float64: 1e-12}  # rel-L2 per row of every transform test


def read_shapes():
    out = []
    with open(os.path.join(ROOT, "tests", "mat_mul_shapes.txt")) as f:
        for line in f:
            line = line.split("#")[0].split()
            if line:
                out.append((line[0], line[1] == "trans", int(line[2]), int(line[3]), int(line[4])))
    return out


SHAPES = read_shapes()


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    assert np.finfo(np.longdouble).nmant >= 63
    return b


def make(seed, rows, points, cplx, dtype):
    """[rows, row_len] scalars: mixed signs, four decades of magnitude, about 2 % exact zeros"""
    rng = np.random.default_rng(seed)
    shape = (rows, points * (2 if cplx else 1))
    v = rng.standard_normal(shape) * 10.0 ** rng.uniform(-2.0, 2.0, shape)
    v[rng.random(shape) < 0.02] = 0.0
    return v.astype(dtype)


def upload(bd, arr, cplx, **kw):
    if arr.size == 0:
        return bd.DspMat(is_complex=cplx, dtype=arr.dtype, rows=arr.shape[0], row_len=arr.shape[1], **kw)
    return bd.DspMat(arr, is_complex=cplx, **kw)


def as_points(arr, cplx):
    """[rows, row_len] scalars -> [rows, points] real or complex of the same precision"""
    if not cplx:
        return arr
    return np.ascontiguousarray(arr).view(np.complex64 if arr.dtype == np.float32 else np.complex128)


def reference(a, b, cplx, trans):
    """(ref, sum |a| |b|): ref one precision up -- a complex128 / float64 array for f32 inputs, a (re, im) pair of
    longdouble arrays for f64 inputs (im None for real operands)"""
    A, B = as_points(a, cplx), as_points(b, cplx)
    if trans:
        B = B.conj().T
    mod = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    if a.dtype == np.float32:
        wide = np.complex128 if cplx else np.float64
        return A.astype(wide) @ B.astype(wide), mod
    L = np.longdouble
    if not cplx:
        return (A.astype(L) @ B.astype(L), None), mod
    ar, ai, br, bi = A.real.astype(L), A.imag.astype(L), B.real.astype(L), B.imag.astype(L)
    return (ar @ br - ai @ bi, ar @ bi + ai @ br), mod


def worst_ratio(out, ref, mod, K, dtype, cplx):
    """max |out - ref| / ((2 K + 4) eps sum |a| |b|); where the bound is 0 the output must be 0"""
    o = as_points(out, cplx)
    assert o.shape == mod.shape, (o.shape, mod.shape)
    if o.size == 0:
        return 0.0
    if isinstance(ref, tuple):
        L = np.longdouble
        if cplx:
            err = np.hypot(o.real.astype(L) - ref[0], o.imag.astype(L) - ref[1]).astype(np.float64)
        else:
            err = np.abs(o.astype(L) - ref[0]).astype(np.float64)
    else:
        err = np.abs(o.astype(ref.dtype) - ref)
    bound = (2 * K + 4) * float(np.finfo(dtype).eps) * mod
    assert np.all(err[bound == 0] == 0)
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def product(bd, a, b, cplx, trans):
    """upload, multiply, download; asserts the code, the shape and that the operands came through untouched"""
    da, db = upload(bd, a, cplx), upload(bd, b, cplx)
    code, y = bd.matmul(da, db, conj_transpose=trans)
    assert code == 0 and y is not None
    M, N = a.shape[0], (b.shape[0] if trans else b.shape[1] // (2 if cplx else 1))
    assert (y.rows(), y.row_points(), y.is_complex()) == (M, N if M else 0, cplx)
    assert np.array_equal(da.data().view(np.uint8), a.view(np.uint8)) and np.array_equal(db.data().view(np.uint8), b.view(np.uint8))
    return y.data()


def operands(seed, M, K, N, cplx, trans, dtype):
    return make(seed, M, K, cplx, dtype), (make(seed + 1, N, K, cplx, dtype) if trans else make(seed + 1, K, N, cplx, dtype))


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("path", ["stream", "tiled", "split"])
def test_each_path_at_its_edges(bd, path, dtype, cplx):
    """every line of mat_mul_shapes.txt for this path: M, N and K in turn at 1, T - 1, T, T + 1, 2 T + 1 of the path's
    tiles (and K at C - 1, C, C + 1, 2 C + 1 of the split chunk), the others at the smallest values that keep the path,
    plus shapes with all three odd and coprime to the tiles; twice on fresh uploads, bit-equal"""
    worst = 0.0
    shapes = [s for s in SHAPES if s[0] == path]
    assert len(shapes) >= 20
    for n, (_, trans, M, K, N) in enumerate(shapes):
        a, b = operands(1000 + 2 * n, M, K, N, cplx, trans, dtype)
        ref, mod = reference(a, b, cplx, trans)
        out = product(bd, a, b, cplx, trans)
        r = worst_ratio(out, ref, mod, K, dtype, cplx)
        assert r <= 1.0, (path, trans, M, K, N, r)
        worst = max(worst, r)
        again = product(bd, a, b, cplx, trans)  # determinism: fresh uploads of the same data, the same bits
        assert np.array_equal(out.view(np.uint8), again.view(np.uint8)), (path, trans, M, K, N)
    print("matmul %s %s %s: worst |out - ref| / bound = %.3f over %d shapes" %
          (path, np.dtype(dtype).name, "complex" if cplx else "real", worst, len(shapes)))


@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
def test_split_chunks_longer_than_the_minimum(bd, cplx):
    """512 x 8200 x 512: 64 tiles, so at most 16 chunks, and the chunk grows from 512 to 544 (f32 only: the reference of
    the f64 case in longdouble would take a minute; the host simulation covers the chunking for both)"""
    M, K, N = 512, 8200, 512
    a, b = operands(77, M, K, N, cplx, True, np.float32)
    ref, mod = reference(a, b, cplx, True)
    r = worst_ratio(product(bd, a, b, cplx, True), ref, mod, K, np.float32, cplx)
    print("matmul split 512 x 8200 x 512 f32 %s: worst ratio %.3f" % ("complex" if cplx else "real", r))
    assert r <= 1.0


@pytest.mark.parametrize("trans", [False, True], ids=["plain", "trans"])
def test_real_f32_rows_on_4_byte_boundaries(bd, trans):
    """odd row_len in both operands, every path; one operand filled row by row with set_row and then shortened by diff,
    so that its buffer is larger than the matrix"""
    shapes = [(5, 7, 301), (17, 67, 33), (5, 513, 3)] if not trans else [(5, 67, 3), (65, 35, 67), (5, 513, 3)]
    for n, (M, K, N) in enumerate(shapes):
        a = make(300 + n, M, K, False, np.float32)
        braw = make(400 + n, N if trans else K, (K if trans else N) + 1, False, np.float32)
        da = upload(bd, a, False)
        db = bd.DspMat(is_complex=False, dtype=np.float32, rows=braw.shape[0], row_len=braw.shape[1])
        for r in range(braw.shape[0]):
            assert db.set_row(r, bd.DspVec(braw[r])) == 0
        assert db.diff() == 0
        b = db.data()
        assert b.shape == (braw.shape[0], braw.shape[1] - 1) and a.shape[1] % 2 == 1 and b.shape[1] % 2 == 1
        code, y = bd.matmul(da, db, conj_transpose=trans)
        assert code == 0
        ref, mod = reference(a, b, False, trans)
        assert worst_ratio(y.data(), ref, mod, K, np.float32, False) <= 1.0, (M, K, N)
        assert np.array_equal(db.data(), b) and np.array_equal(da.data(), a)
        assert db.scale(2.0) == 0 and np.array_equal(db.data(), b * np.float32(2))  # still usable


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_gram_matrix_of_the_same_object(bd, dtype, cplx):
    """matmul(x, x, conj_transpose=True) on the tiled and on the split path: within the bound, Hermitian to the bit (the
    implementation promises it: mm_cplx_step in mat_mul_core.h), a real, non-negative diagonal, x unchanged bit for bit"""
    for n, (M, K) in enumerate([(67, 35), (70, 1031)]):
        x = make(500 + n, M, K, cplx, dtype)
        dx = upload(bd, x, cplx)
        code, r = bd.matmul(dx, dx, conj_transpose=True)
        assert code == 0 and (r.rows(), r.row_points()) == (M, M)
        ref, mod = reference(x, x, cplx, True)
        out = r.data()
        assert worst_ratio(out, ref, mod, K, dtype, cplx) <= 1.0
        g = as_points(out, cplx)
        assert np.array_equal(g, g.conj().T)
        d = np.diagonal(g)
        assert np.all(d.imag == 0) and np.all(d.real >= 0)
        assert np.array_equal(dx.data().view(np.uint8), x.view(np.uint8))


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_domain_and_delta_follow_the_operand_whose_row_axis_survives(bd, dtype, cplx):
    a, b = make(1, 3, 5, cplx, dtype), make(2, 5, 4, cplx, dtype)
    da, db = upload(bd, a, cplx, domain=FREQ, delta=0.5), upload(bd, b, cplx, domain=TIME, delta=2.0)
    code, y = bd.matmul(da, db)
    assert code == 0 and (y.domain(), y.delta(), y.is_complex()) == (TIME, 2.0, cplx)
    bt = make(3, 4, 5, cplx, dtype)
    dbt = upload(bd, bt, cplx, domain=TIME, delta=2.0)
    code, y = bd.matmul(da, dbt, conj_transpose=True)
    assert code == 0 and (y.domain(), y.delta(), y.is_complex()) == (FREQ, 0.5, cplx)
    # the operands keep their own and are usable afterwards
    assert (da.domain(), da.delta(), db.domain(), db.delta()) == (FREQ, 0.5, TIME, 2.0)
    assert da.scale(2.0) == 0 and np.array_equal(da.data(), a * dtype(2))
    assert np.array_equal(db.data(), b)


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_codes(bd, dtype, cplx):
    e = 2 if cplx else 1
    a, b = make(1, 3, 5, cplx, dtype), make(2, 5, 4, cplx, dtype)
    da, db = upload(bd, a, cplx), upload(bd, b, cplx)
    # 7 for each shape mismatch in each form, no matrix
    for rows, points in ((4, 4), (6, 4), (3, 5)):
        other = upload(bd, make(3, rows, points, cplx, dtype), cplx)
        assert bd.matmul(da, other) == (7, None), (rows, points)
    for rows, points in ((4, 4), (5, 4), (5, 6)):
        other = upload(bd, make(3, rows, points, cplx, dtype), cplx)
        assert bd.matmul(da, other, conj_transpose=True) == (7, None), (rows, points)
    # 2 for real x complex, either way round, either form, even where the shapes would fit
    mixed = upload(bd, make(4, 5, 4, not cplx, dtype), not cplx)
    assert bd.matmul(da, mixed) == (2, None) and bd.matmul(mixed, da, conj_transpose=True) == (2, None)
    mixed_t = upload(bd, make(4, 4, 5, not cplx, dtype), not cplx)
    assert bd.matmul(da, mixed_t, conj_transpose=True) == (2, None)
    # -1 and a poisoned result for a poisoned a and for a poisoned b
    bad = upload(bd, make(5, 5, 4, True, dtype), True)
    assert bad.to_complex() == -1
    for x, y in ((bad, db), (da, bad), (bad, bad)):
        for trans in (False, True):
            code, r = bd.matmul(x, y, conj_transpose=trans)
            assert code == -1 and r is not None
            assert r.row_len() == 0 and np.isnan(r.delta()) and r.scale(2.0) == -1
    assert da.scale(1.0) == 0 and db.scale(1.0) == 0
    # the empty shapes: all 0
    zero = lambda rows, points: bd.DspMat(is_complex=cplx, dtype=dtype, rows=rows, row_len=points * e)
    code, r = bd.matmul(zero(3, 0), zero(4, 0), conj_transpose=True)  # K == 0: 3 x 4 of +0
    assert code == 0 and (r.rows(), r.row_points()) == (3, 4)
    assert not r.data().any() and not np.signbit(r.data()).any()
    code, r = bd.matmul(zero(3, 0), zero(0, 0))  # K == 0, plain: b without rows has no columns either
    assert code == 0 and (r.rows(), r.row_points()) == (3, 0)
    code, r = bd.matmul(zero(0, 0), zero(4, 0), conj_transpose=True)  # M == 0: no rows
    assert code == 0 and (r.rows(), r.row_len()) == (0, 0)
    code, r = bd.matmul(zero(0, 0), zero(0, 0))
    assert code == 0 and r.rows() == 0
    code, r = bd.matmul(da, zero(5, 0))  # N == 0: M empty rows
    assert code == 0 and (r.rows(), r.row_points()) == (3, 0) and r.data().shape == (3, 0)
    assert bd.matmul(zero(3, 5), zero(0, 0)) == (7, None)  # a has 5 points a row, b no rows
    # TypeError from the Python function
    with pytest.raises(TypeError):
        bd.matmul(da, bd.DspVec(np.ones(5, dtype=dtype)))
    with pytest.raises(TypeError):
        bd.matmul(a, db)
    with pytest.raises(TypeError):
        bd.matmul(da, upload(bd, b.astype(np.float64 if dtype == np.float32 else np.float32), cplx))


def test_the_c_entry_points_null_the_result_after_an_argument_error(bd):
    import ctypes as C
    for dtype, sfx in ((np.float32, "32"), (np.float64, "64")):
        da, db = upload(bd, make(1, 3, 5, False, dtype), False), upload(bd, make(2, 4, 4, False, dtype), False)
        fn = getattr(bd.lib, "bdsp_hip_mat_matmul" + sfx)
        for form in (0, 1):
            out = C.c_void_p(12345)
            assert fn(da._h, db._h, form, C.byref(out)) == 7 and out.value is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_chain_fft_matmul_ifft(bd, dtype):
    """8 real channels x 4099 points, to_complex, fft, matmul(W, .) with a complex 3 x 8 W, ifft, against the same chain
    in numpy.  Tolerance per row, in the units of the result: T ||y_i|| for the inverse transform, T sum_k |W_ik|
    ||x_k|| for the forward transform's error carried through the product, and the product's own bound on the spectra
    divided by sqrt(N) (the inverse transform scales an L2 norm by 1 / sqrt(N)); T = 1e-6 / 1e-12, the transform tests'
    rel-L2 figure."""
    C_, N_, B_ = 8, 4099, 3
    x = make(900, C_, N_, False, dtype)
    w = make(901, B_, C_, True, dtype)
    dx, dw = upload(bd, x, False), upload(bd, w, True)
    assert dx.to_complex() == 0 and dx.fft() == 0
    code, y = bd.matmul(dw, dx)
    assert code == 0 and y.domain() == FREQ and (y.rows(), y.row_points()) == (B_, N_)
    assert y.ifft() == 0 and y.domain() == TIME
    out = as_points(y.data(), True).astype(np.complex128)
    W, X = as_points(w, True).astype(np.complex128), np.fft.fft(x.astype(np.float64), axis=1)
    ref = np.fft.ifft(W @ X, axis=1)
    T, eps = TRANSFORM_TOL[dtype], float(np.finfo(dtype).eps)
    xn = np.linalg.norm(x.astype(np.float64), axis=1)
    allowed = (T * np.linalg.norm(ref, axis=1) + T * (np.abs(W) @ xn)
               + np.linalg.norm((2 * C_ + 4) * eps * (np.abs(W) @ np.abs(X)), axis=1) / np.sqrt(N_))
    err = np.linalg.norm(out - ref, axis=1)
    print("matmul chain %s: err / allowed per row %s" % (np.dtype(dtype).name, err / allowed))
    assert np.all(err <= allowed)
