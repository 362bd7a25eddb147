"""cholesky / cholesky_solve: Hermitian positive-definite systems on the device, through the Python functions and the C ABI.

Reference: numpy one precision up -- complex128 / float64 for f32, np.longdouble (four real products per complex one)
for f64.  With eps = np.finfo(dtype).eps, c(N) = 2 N + 4 and c2(N) = 3 c(N), element by element:

    cholesky            |A - L L^H|   <= c(N)  eps (|L| |L|^H)        A the loaded matrix, as the device reads it
    "forward"           |B - L X|     <= c(N)  eps (|L| |X|)
    "backward"          |B - L^H X|   <= c(N)  eps (|L|^H |X|)
    "both"              |B - L L^H X| <= c2(N) eps (|L| |L|^H |X|)

The bounds are derived from the order of operations (one rounding per fma, division and square root; a complex product is
four real ones), not measured, and no path has a tolerance of its own.  Inputs: A = G G^H / 2N + 0.1 I with G random
N x 2N, built in f64 and rounded; B random.  The shapes and the path each must take are tests/mat_chol_shapes.txt;
tests/host_sim/sim_mat_chol.cpp (run by tests/test_mat_chol_abi.py) checks every line of it against the dispatch rule.
The test prints the worst ratio to the bound per path."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(np.float32, True), (np.float32, False), (np.float64, True), (np.float64, False)]
VARIANT_IDS = ["f32-complex", "f32-real", "f64-complex", "f64-real"]
L = np.longdouble


def c1(N):
    return 2.0 * N + 4.0


def c2(N):
    return 3.0 * c1(N)


def read_shapes():
    out = []
    with open(os.path.join(ROOT, "tests", "mat_chol_shapes.txt")) as f:
        for line in f:
            line = line.split("#")[0].split()
            if line:
                out.append((line[0], int(line[1]), int(line[2])))
    return out


SHAPES = read_shapes()


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    assert np.finfo(np.longdouble).nmant >= 63
    return b


def as_points(arr, cplx):
    if not cplx:
        return arr
    return np.ascontiguousarray(arr).view(np.complex64 if arr.dtype == np.float32 else np.complex128)


def as_scalars(pts, dtype):
    """[rows, points] real or complex -> [rows, row_len] scalars of dtype"""
    if np.iscomplexobj(pts):
        return np.ascontiguousarray(pts.astype(np.complex64 if dtype == np.float32 else np.complex128)).view(dtype)
    return np.ascontiguousarray(pts.astype(dtype))


def upload(bd, arr, cplx, **kw):
    if arr.size == 0:
        return bd.DspMat(is_complex=cplx, dtype=arr.dtype, rows=arr.shape[0], row_len=arr.shape[1], **kw)
    return bd.DspMat(arr, is_complex=cplx, **kw)


_SPD = {}


def spd(N, cplx, dtype, seed=0):
    """A = G G^H / 2N + 0.1 I as [N, row_len] scalars of dtype (computed once per key and never changed)"""
    key = (N, cplx, np.dtype(dtype).name, seed)
    if key not in _SPD:
        rng = np.random.default_rng(7000 + 13 * N + seed)
        G = rng.standard_normal((N, 2 * N))
        if cplx:
            G = G + 1j * rng.standard_normal((N, 2 * N))
        A = G @ G.conj().T / (2.0 * max(N, 1)) + 0.1 * np.eye(N)
        a = as_scalars(A, dtype)
        a.setflags(write=False)
        _SPD[key] = a
    return _SPD[key]


def rhs(N, P, cplx, dtype, seed=0):
    rng = np.random.default_rng(9000 + 17 * N + P + seed)
    return rng.standard_normal((N, P * (2 if cplx else 1))).astype(dtype)


def wide(x):
    """(re, im) one precision up: float64 parts for f32 input, longdouble for f64"""
    w = np.float64 if x.real.dtype == np.float32 else L
    return x.real.astype(w), (x.imag.astype(w) if np.iscomplexobj(x) else None)


def cmul(a, b):
    """the product of two (re, im) pairs of wide arrays (im None for real), four real products"""
    ar, ai = a
    br, bi = b
    if ai is None and bi is None:
        return ar @ br, None
    z = lambda r, like: np.zeros_like(like) if r is None else r
    ai, bi = z(ai, ar), z(bi, br)
    return ar @ br - ai @ bi, ar @ bi + ai @ br


def conj_t(a):
    return a[0].T, (None if a[1] is None else -a[1].T)


def err_of(res, ref):
    """|res - ref| as float64 for (re, im) pairs"""
    dr = res[0] - ref[0]
    if ref[1] is None and res[1] is None:
        return np.abs(dr).astype(np.float64)
    z = lambda r, like: np.zeros_like(like) if r is None else r
    return np.hypot(dr, z(res[1], dr) - z(ref[1], dr)).astype(np.float64)


def ratio(err, bound):
    assert np.all(np.isfinite(err)), "a non-finite residual"
    assert np.all(err[bound == 0] == 0)
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def lower_of(l, cplx):
    """the factor as the solves read it: the lower triangle, the diagonal's real part"""
    Lp = np.tril(as_points(l, cplx))
    if cplx:
        Lp = Lp.copy()
        np.fill_diagonal(Lp, Lp.diagonal().real)
    return Lp


def chol_ratio(a_loaded_pts, l, cplx, dtype):
    """max |A - L L^H| / (c(N) eps |L| |L|^H) over the lower triangle (the upper one is its mirror image)"""
    N = l.shape[0]
    if N == 0:
        return 0.0
    Lp = lower_of(l, cplx)
    lw = wide(Lp)
    prod = cmul(lw, conj_t(lw))
    mod = np.abs(Lp).astype(np.float64) @ np.abs(Lp).astype(np.float64).T
    err = err_of(wide(a_loaded_pts), prod)
    bound = c1(N) * float(np.finfo(dtype).eps) * mod
    il = np.tril_indices(N)
    return ratio(err[il], bound[il])


def solve_ratio(l, b, x, part, cplx, dtype):
    N = l.shape[0]
    Xp, Bp = as_points(x, cplx), as_points(b, cplx)
    if Xp.size == 0:
        return 0.0
    Lp = lower_of(l, cplx)
    lw, xw = wide(Lp), wide(Xp)
    la, xa = np.abs(Lp).astype(np.float64), np.abs(Xp).astype(np.float64)
    eps = float(np.finfo(dtype).eps)
    if part == "forward":
        res, mod, c = cmul(lw, xw), la @ xa, c1(N)
    elif part == "backward":
        res, mod, c = cmul(conj_t(lw), xw), la.T @ xa, c1(N)
    else:
        res, mod, c = cmul(lw, cmul(conj_t(lw), xw)), la @ (la.T @ xa), c2(N)
    return ratio(err_of(wide(Bp), res), c * eps * mod)


def loaded(a, d, cplx):
    """a copy with T(d) added to the real part of the diagonal in precision T, one rounding -- what the device factors"""
    out = a.copy()
    N = a.shape[0]
    step = 2 if cplx else 1
    idx = np.arange(N)
    out[idx, idx * step] = (out[idx, idx * step] + a.dtype.type(d)).astype(a.dtype)
    return out


def factor(bd, a, cplx, loading=0.0):
    da = upload(bd, np.array(a), cplx)
    code, l = bd.cholesky(da, loading=loading) if loading else bd.cholesky(da)
    assert code == 0 and l is not None, code
    N = a.shape[0]
    assert (l.rows(), l.row_points() if N else 0, l.is_complex()) == (N, N, cplx)
    assert np.array_equal(da.data().view(np.uint8), np.asarray(a).view(np.uint8))  # the operand came through untouched
    return l, (l.data() if N else np.zeros((0, 0), a.dtype))


def check_structure(l, cplx):
    """+0 above the diagonal and in the diagonal's imaginary part, to the bit; the diagonal > 0"""
    N = l.shape[0]
    P = as_points(l, cplx)
    iu = np.triu_indices(N, 1)
    zero_bits = np.zeros(1, l.dtype).view(np.uint8)
    up = np.ascontiguousarray(P[iu])
    assert not up.view(np.uint8).any(), "above the diagonal"
    d = np.ascontiguousarray(P.diagonal())
    if cplx:
        assert not np.ascontiguousarray(d.imag).view(np.uint8).any(), "the diagonal's imaginary part"
        d = d.real
    assert np.all(d > 0) and zero_bits.size


WORST = {}


def note(path, what, r):
    WORST[(path, what)] = max(WORST.get((path, what), 0.0), r)


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("path", ["empty", "small", "blocked"])
def test_every_shape_within_the_derived_bounds(bd, path, dtype, cplx):
    """every line of mat_chol_shapes.txt of this path: the factor's structure and bound, the three solves' bounds, "both"
    bit-equal to forward then backward, the operands untouched, twice with the same bits"""
    shapes = [s for s in SHAPES if s[0] == path]
    assert shapes
    factors = {}
    for _, N, P in shapes:
        a = spd(N, cplx, dtype)
        if N not in factors:
            lh, l = factor(bd, a, cplx)
            _, l_again = factor(bd, a, cplx)
            assert np.array_equal(l.view(np.uint8), l_again.view(np.uint8)), "two runs differ"
            check_structure(l, cplx)
            r = chol_ratio(as_points(np.asarray(a), cplx), l, cplx, dtype)
            print("cholesky %s N %d: %.4f of the bound" % (path, N, r))
            assert r <= 1.0, (N, r)
            note(path, "cholesky", r)
            factors[N] = (lh, l)
        lh, l = factors[N]
        b = rhs(N, P, cplx, dtype)
        db = upload(bd, b, cplx)
        got = {}
        for part in ("forward", "backward", "both"):
            code, x = bd.cholesky_solve(lh, db, part=part)
            assert code == 0 and x is not None, (N, P, part, code)
            assert (x.rows(), x.is_complex()) == (N, cplx) and (x.row_points() == P or N == 0)
            got[part] = x.data() if N and P else np.zeros((N, 0), dtype)
            r = solve_ratio(l, b, got[part], part, cplx, dtype)
            print("%s %s N %d P %d: %.4f of the bound" % (part, path, N, P, r))
            assert r <= 1.0, (N, P, part, r)
            note(path, part, r)
            code, x2 = bd.cholesky_solve(lh, db, part=part)
            assert code == 0 and np.array_equal((x2.data() if N and P else got[part]).view(np.uint8), got[part].view(np.uint8)), "two runs differ"
        assert np.array_equal(db.data().view(np.uint8), b.view(np.uint8)) if b.size else True
        assert np.array_equal(lh.data().view(np.uint8), l.view(np.uint8)) if l.size else True
        if N and P:  # "both" = forward, then backward on its result
            code, y = bd.cholesky_solve(lh, db, part="forward")
            code2, x = bd.cholesky_solve(lh, y, part="backward")
            assert code == 0 and code2 == 0
            assert np.array_equal(x.data().view(np.uint8), got["both"].view(np.uint8))
    print("worst so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("N", [17, 64, 130])
def test_upper_triangle_and_diagonal_imaginary_parts_are_never_read(bd, N, dtype, cplx):
    a = np.array(spd(N, cplx, dtype))
    _, clean = factor(bd, a, cplx)
    dirty = a.copy()
    P = as_points(dirty, cplx)
    iu = np.triu_indices(N, 1)
    P[iu] = np.nan
    if cplx:
        P[np.arange(N), np.arange(N)] += 1j * np.linspace(-5.0, 5.0, N).astype(dtype)
        P[0, 0] = complex(P[0, 0].real, np.nan)
    _, got = factor(bd, dirty, cplx)
    assert np.array_equal(got.view(np.uint8), clean.view(np.uint8))
    # the solves read the same part of l only
    lp = as_points(clean.copy(), cplx)
    lp[iu] = np.nan
    if cplx:
        lp[np.arange(N), np.arange(N)] += 1j * 3.0
    b = rhs(N, 65, cplx, dtype)
    for part in ("forward", "backward", "both"):
        c0, x0 = bd.cholesky_solve(upload(bd, clean, cplx), upload(bd, b, cplx), part=part)
        c1_, x1 = bd.cholesky_solve(upload(bd, as_scalars(lp, dtype) if cplx else lp, cplx), upload(bd, b, cplx), part=part)
        assert c0 == 0 and c1_ == 0
        assert np.array_equal(x0.data().view(np.uint8), x1.data().view(np.uint8)), part


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("N", [33, 130])
def test_loading_is_one_rounded_add_on_the_diagonal(bd, N, dtype, cplx):
    a = np.array(spd(N, cplx, dtype, seed=1))
    d = 0.3217
    _, got = factor(bd, a, cplx, loading=d)
    _, want = factor(bd, loaded(a, d, cplx), cplx)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    r = chol_ratio(as_points(loaded(a, d, cplx), cplx), got, cplx, dtype)
    assert r <= 1.0, r


@pytest.mark.parametrize("dtype,cplx", [(np.float32, True), (np.float32, False)], ids=["f32-complex", "f32-real"])
@pytest.mark.parametrize("N", [48, 130])
def test_ill_conditioned_gram_matrix(bd, N, dtype, cplx):
    """nearly parallel rows, condition number about 1e6: the same backward bound, or 8 -- accepted only if the f64
    reference's smallest pivot is below N eps max diag"""
    rng = np.random.default_rng(31 + N)
    base = rng.standard_normal((1, 3 * N)) + (1j * rng.standard_normal((1, 3 * N)) if cplx else 0)
    G = base + 1e-3 * (rng.standard_normal((N, 3 * N)) + (1j * rng.standard_normal((N, 3 * N)) if cplx else 0))
    A = G @ G.conj().T / (3.0 * N)
    a = as_scalars(A, dtype)
    code, l = bd.cholesky(upload(bd, a, cplx))
    ap = as_points(a, cplx).astype(np.complex128 if cplx else np.float64)
    ap = np.tril(ap) + np.tril(ap, -1).conj().T
    if cplx:
        np.fill_diagonal(ap, ap.diagonal().real)
    if code == 8:
        assert l is None
        # the f64 reference's pivots: the squares of its factor's diagonal, where it exists at all
        try:
            piv = np.linalg.cholesky(ap).diagonal().real ** 2
            smallest = float(piv.min())
        except np.linalg.LinAlgError:
            smallest = 0.0
        assert smallest < N * float(np.finfo(dtype).eps) * float(ap.diagonal().real.max()), smallest
        return
    assert code == 0
    ld = l.data()
    check_structure(ld, cplx)
    r = chol_ratio(as_points(a, cplx), ld, cplx, dtype)
    print("ill-conditioned N %d: %.4f of the bound" % (N, r))
    assert r <= 1.0, r


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_not_positive_definite_gives_8_and_no_matrix(bd, dtype, cplx):
    N = 130
    step = 2 if cplx else 1
    base = np.array(spd(N, cplx, dtype))
    for at in (0, 40, 63, 64, N - 1):
        a = base.copy()
        a[at, at * step] = -1.0
        code, l = bd.cholesky(upload(bd, a, cplx))
        assert code == 8 and l is None, at
    code, l = bd.cholesky(upload(bd, np.zeros_like(base), cplx))
    assert code == 8 and l is None
    a = base.copy()
    a[100, 7 * step] = np.nan
    code, l = bd.cholesky(upload(bd, a, cplx))
    assert code == 8 and l is None
    small = np.array(spd(17, cplx, dtype))
    small[5, 5 * step] = -2.0
    code, l = bd.cholesky(upload(bd, small, cplx))
    assert code == 8 and l is None
    # the next call on the same device works
    _, good = factor(bd, base, cplx)
    assert chol_ratio(as_points(base, cplx), good, cplx, dtype) <= 1.0


def test_codes_and_argument_errors(bd):
    f32 = np.float32
    a = np.array(spd(8, False, f32))
    da = upload(bd, a, False)
    code, l = bd.cholesky(da)
    assert code == 0
    # 7: not square / rows disagree
    code, x = bd.cholesky(upload(bd, np.ones((3, 4), f32), False))
    assert code == 7 and x is None
    code, x = bd.cholesky_solve(l, upload(bd, np.ones((7, 5), f32), False))
    assert code == 7 and x is None
    code, x = bd.cholesky_solve(upload(bd, np.ones((8, 7), f32), False), upload(bd, np.ones((8, 5), f32), False))
    assert code == 7 and x is None
    # 2: a real and a complex operand
    code, x = bd.cholesky_solve(l, upload(bd, np.ones((8, 6), f32), True))
    assert code == 2 and x is None
    # -1: a poisoned operand gives a poisoned result
    bad = upload(bd, np.ones((8, 16), f32), True)
    assert bad.to_complex() == -1  # a complex matrix cannot be made complex: poisoned
    code, x = bd.cholesky(bad)
    assert code == -1 and x is not None
    code, y = bd.cholesky_solve(l, x)
    assert code == -1 and y is not None
    code, y = bd.cholesky_solve(bad, upload(bd, np.ones((8, 2), f32), False))
    assert code == -1 and y is not None
    # the empty shapes
    code, e = bd.cholesky(bd.DspMat(is_complex=False, dtype=f32, rows=0, row_len=0))
    assert code == 0 and e is not None and e.rows() == 0
    code, x = bd.cholesky_solve(l, bd.DspMat(is_complex=False, dtype=f32, rows=8, row_len=0))
    assert code == 0 and x.rows() == 8 and x.row_points() == 0
    code, x = bd.cholesky_solve(e, bd.DspMat(is_complex=False, dtype=f32, rows=0, row_len=0))
    assert code == 0 and x.rows() == 0
    # a zero on l's diagonal: inf / NaN and code 0
    lz = l.data().copy()
    lz[3, 3] = 0.0
    code, x = bd.cholesky_solve(upload(bd, lz, False), upload(bd, np.ones((8, 3), f32), False), part="forward")
    assert code == 0 and not np.all(np.isfinite(x.data()))
    # Python-level errors
    with pytest.raises(ValueError):
        bd.cholesky_solve(l, upload(bd, np.ones((8, 2), f32), False), part="upper")
    with pytest.raises(ValueError):
        bd.cholesky_solve(l, upload(bd, np.ones((8, 2), f32), False), part=1)
    with pytest.raises(TypeError):
        bd.cholesky(np.ones((4, 4), f32))
    with pytest.raises(TypeError):
        bd.cholesky_solve(l, np.ones((8, 2), f32))
    with pytest.raises(TypeError):
        bd.cholesky_solve(l, upload(bd, np.ones((8, 2), np.float64), False))
    # the C entry point: any other part is BDSP_ERR_UNSUPPORTED, no matrix
    import ctypes as C
    out = C.c_void_p(1)
    rc = bd.lib.bdsp_hip_mat_cholesky_solve32(l._h, da._h, 3, C.byref(out))
    assert rc == -102 and not out.value


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_covariance_to_adaptive_weights(bd, dtype):
    """matmul(x, x^H) -> cholesky(., loading) -> cholesky_solve(L, s) for 8 channels x 4096 points: the weights pass the
    "both" bound against the factor and against the downloaded covariance (c2 counts the factorisation's roundings and
    both passes': at most 2 N + 2 (2 N - 1) unit roundoffs, below 3 c(N) eps with room for the second-order terms)"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((8, 2 * 4096)).astype(dtype)
    dx = upload(bd, x, True)
    code, cov = bd.matmul(dx, dx, conj_transpose=True)
    assert code == 0
    d = 0.01 * 4096
    code, l = bd.cholesky(cov, loading=d)
    assert code == 0
    s = rng.standard_normal((8, 2)).astype(dtype)  # one steering vector: 8 x 1 complex
    ds = upload(bd, s, True)
    code, w = bd.cholesky_solve(l, ds)
    assert code == 0 and (w.rows(), w.row_points()) == (8, 1)
    ld, wd, cd = l.data(), w.data(), cov.data()
    assert solve_ratio(ld, s, wd, "both", True, dtype) <= 1.0
    assert chol_ratio(as_points(loaded(cd, d, True), True), ld, True, dtype) <= 1.0
    # against the loaded covariance itself
    A = as_points(loaded(cd, d, True), True)
    A = np.tril(A) + np.tril(A, -1).conj().T
    np.fill_diagonal(A, A.diagonal().real)
    res = cmul(wide(A), wide(as_points(wd, True)))
    la = np.abs(lower_of(ld, True)).astype(np.float64)
    bound = c2(8) * float(np.finfo(dtype).eps) * (la @ (la.T @ np.abs(as_points(wd, True)).astype(np.float64)))
    assert ratio(err_of(wide(as_points(s, True)), res), bound) <= 1.0
