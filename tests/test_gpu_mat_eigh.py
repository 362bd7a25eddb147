"""eigh: the eigendecomposition of a Hermitian DspMat on the device, through the Python function and the C ABI.

Reference: numpy one precision up -- complex128 / float64 for f32, np.clongdouble / np.longdouble for f64.  With
eps = np.finfo(dtype).eps, S the sweeps the call reports and A the Hermitian completion of the lower triangle the device
reads (mat_eigh_core.h has the same formulas as je_bound_res / je_bound_orth), in Frobenius norms:

    |A - v^H diag(w) v| <= c_res(N, S) eps |A|          |v v^H - I| <= c_orth(N, S) eps
    c_orth = 2 K S sqrt(N),  c_res = 2 K S (1 + sqrt(N)) + 1
    K = rho N (N <= 64),  8 (128 rho + 132) steps(ceil(N / 32)) (N > 64);  rho = 24 real, 40 complex

and for f32, by Weyl's theorem, |w_k - lambda_k| <= c_res eps |A| against numpy.linalg.eigvalsh of A in float64.  The
bounds are derived from the order of operations, not measured, and no path has a tolerance of its own.  The shapes and
the path each must take are tests/mat_eigh_shapes.txt; tests/host_sim/sim_mat_eigh.cpp (run by
tests/test_mat_eigh_abi.py) checks every line of it against the dispatch rule.  The test prints the worst ratio to the
bound per path."""
import os
import re

import numpy as np
import pytest

from test_gpu_mat_chol import VARIANTS, VARIANT_IDS, as_points, as_scalars, spd, upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SWEEPS = 30


def read_shapes():
    out = []
    with open(os.path.join(ROOT, "tests", "mat_eigh_shapes.txt")) as f:
        for line in f:
            line = line.split("#")[0].split()
            if line:
                out.append((line[0], int(line[1])))
    return out


SHAPES = read_shapes()


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    assert np.finfo(np.longdouble).nmant >= 63
    return b


def steps(n):
    return 0 if n < 2 else (n if n % 2 else n - 1)


def kappa(N, cplx):
    rho = 40.0 if cplx else 24.0
    if N <= 64:
        return rho * N
    return 8.0 * (128.0 * rho + 132.0) * steps((N + 31) // 32)


def c_orth(N, S, cplx):
    return 2.0 * kappa(N, cplx) * S * np.sqrt(float(N))


def c_res(N, S, cplx):
    return 2.0 * kappa(N, cplx) * S * (1.0 + np.sqrt(float(N))) + 1.0


def completed(a, cplx):
    """the matrix as the device reads it: the Hermitian completion of the lower triangle, the diagonal's real part"""
    P = as_points(np.asarray(a), cplx)
    A = np.tril(P) + np.tril(P, -1).conj().T
    if cplx:
        A = A.copy()
        np.fill_diagonal(A, A.diagonal().real)
    return A


def run(bd, a, cplx):
    """(w [N], v points [N, N], sweeps, handles) of one call; asserts the shapes and that the operand came through untouched"""
    a = np.asarray(a)
    N = a.shape[0]
    da = upload(bd, np.array(a), cplx)
    code, w, v, sweeps = bd.eigh(da, return_sweeps=True)
    assert code == 0 and w is not None and v is not None, code
    assert (w.rows(), w.is_complex()) == (1 if N else 0, False) and (w.row_points() == N or N == 0)
    assert (v.rows(), v.is_complex()) == (N, cplx) and (v.row_points() == N or N == 0)
    if N:
        assert np.array_equal(da.data().view(np.uint8), a.view(np.uint8))
    wd = w.data()[0] if N else np.zeros(0, a.dtype)
    vd = v.data() if N else np.zeros((0, 0), a.dtype)
    return wd, vd, sweeps


def ratios(a, cplx, w, v, sweeps):
    """(residual / bound, orthogonality defect / bound, |A|_F) in the wide precision"""
    dtype = a.dtype.type
    N = a.shape[0]
    if N == 0:
        return 0.0, 0.0, 0.0
    wide = (np.complex128 if cplx else np.float64) if dtype == np.float32 else (np.clongdouble if cplx else np.longdouble)
    A = completed(a, cplx).astype(wide)
    V = as_points(v, cplx).astype(wide)
    W = w.astype(np.float64 if dtype == np.float32 else np.longdouble)
    eps = float(np.finfo(dtype).eps)
    na = float(np.sqrt(np.sum(np.abs(A) ** 2)))
    res = float(np.sqrt(np.sum(np.abs(A - V.conj().T @ (W[:, None] * V)) ** 2)))
    orth = float(np.sqrt(np.sum(np.abs(V @ V.conj().T - np.eye(N)) ** 2)))
    assert np.isfinite(res) and np.isfinite(orth)
    br, bo = c_res(N, sweeps, cplx) * eps * na, c_orth(N, sweeps, cplx) * eps
    return (res / br if br > 0 else (0.0 if res == 0 else np.inf)), orth / bo, na


def check(a, cplx, w, v, sweeps, what):
    """both bounds, the f32 eigenvalue bound, the order of w; returns the two ratios"""
    N = a.shape[0]
    assert 1 <= sweeps <= MAX_SWEEPS, (what, sweeps)
    assert np.all(w[:-1] <= w[1:]), (what, "w does not ascend")
    rr, ro, na = ratios(a, cplx, w, v, sweeps)
    print("%s N %d: %d sweeps, residual %.6f and orthogonality %.6f of the bound" % (what, N, sweeps, rr, ro))
    assert rr <= 1.0 and ro <= 1.0, (what, N, rr, ro)
    if a.dtype == np.float32 and N:
        lam = np.linalg.eigvalsh(completed(a, cplx).astype(np.complex128 if cplx else np.float64))
        weyl = float(np.max(np.abs(w.astype(np.float64) - lam))) / (c_res(N, sweeps, cplx) * float(np.finfo(np.float32).eps) * na) if na else \
            float(np.max(np.abs(w)))
        print("%s N %d: eigenvalues %.6f of the bound" % (what, N, weyl))
        assert weyl <= 1.0, (what, N, weyl)
    return rr, ro


WORST = {}


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("path", ["empty", "small", "blocked"])
def test_every_shape_within_the_derived_bounds(bd, path, dtype, cplx):
    """every line of mat_eigh_shapes.txt of this path on A = G G^H / 2N + 0.1 I: both bounds and the f32 eigenvalue bound,
    w ascending, real, 1 x N, v N x N of the operand's kind, 1 <= sweeps <= cap, the operand untouched, twice the same bits"""
    shapes = [s for s in SHAPES if s[0] == path]
    assert shapes
    for _, N in shapes:
        a = spd(N, cplx, dtype)
        w, v, sweeps = run(bd, a, cplx)
        w2, v2, sweeps2 = run(bd, a, cplx)
        assert sweeps2 == sweeps and np.array_equal(w.view(np.uint8), w2.view(np.uint8)) and np.array_equal(v.view(np.uint8), v2.view(np.uint8)), \
            "two runs differ"
        if N == 0:
            assert sweeps == 1
            continue
        rr, ro = check(np.asarray(a), cplx, w, v, sweeps, "gram " + path)
        WORST[(path, "residual")] = max(WORST.get((path, "residual"), 0.0), rr)
        WORST[(path, "orthogonality")] = max(WORST.get((path, "orthogonality"), 0.0), ro)
    print("worst so far:", {k: round(x, 6) for k, x in sorted(WORST.items())})


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("N", [17, 64, 130])
def test_upper_triangle_and_diagonal_imaginary_parts_are_never_read(bd, N, dtype, cplx):
    a = np.array(spd(N, cplx, dtype))
    w, v, sweeps = run(bd, a, cplx)
    dirty = a.copy()
    P = as_points(dirty, cplx)
    P[np.triu_indices(N, 1)] = np.nan
    if cplx:
        P[np.arange(N), np.arange(N)] += 1j * np.linspace(-5.0, 5.0, N).astype(dtype)
        P[0, 0] = complex(P[0, 0].real, np.nan)
    w2, v2, sweeps2 = run(bd, dirty, cplx)
    assert sweeps2 == sweeps and np.array_equal(w.view(np.uint8), w2.view(np.uint8)) and np.array_equal(v.view(np.uint8), v2.view(np.uint8))


def structured(kind, N, cplx, dtype):
    rng = np.random.default_rng(4100 + 7 * N + len(kind))
    rnd = lambda *s: rng.standard_normal(s) + (1j * rng.standard_normal(s) if cplx else 0)
    if kind == "diagonal":
        return as_scalars(np.diag(rng.permutation(N).astype(np.float64) - 3.0) + (0j if cplx else 0), dtype)
    if kind == "zero":
        return np.zeros((N, N * (2 if cplx else 1)), dtype)
    if kind == "rank3":
        s = rnd(N, 3)
        return as_scalars(s @ s.conj().T, dtype)
    if kind == "rank3+I":
        s = rnd(N, 3)
        return as_scalars(s @ s.conj().T + np.eye(N), dtype)
    if kind == "indefinite":
        h = rnd(N, N)
        return as_scalars((h + h.conj().T) / 2.0, dtype)
    assert kind == "graded"
    h = rnd(N, N)
    d = 10.0 ** (-np.arange(N) / 4.0)
    return as_scalars(d[:, None] * (h @ h.conj().T) * d[None, :], dtype)


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("N", [48, 130])
@pytest.mark.parametrize("kind", ["diagonal", "zero", "rank3", "rank3+I", "indefinite", "graded"])
def test_structure_cases(bd, kind, N, dtype, cplx):
    a = structured(kind, N, cplx, dtype)
    w, v, sweeps = run(bd, a, cplx)
    check(a, cplx, w, v, sweeps, kind)
    eps = float(np.finfo(dtype).eps)
    na = float(np.sqrt(np.sum(np.abs(completed(a, cplx).astype(np.complex128)) ** 2)))
    if kind in ("diagonal", "zero"):
        assert sweeps == 1
        d = np.ascontiguousarray(as_points(a, cplx).diagonal().real)
        assert np.array_equal(w.view(np.uint8), np.sort(d, kind="stable").view(np.uint8))  # to the bit
        Vp = as_points(v, cplx)
        want = np.zeros((N, N), Vp.dtype)
        want[np.arange(N), np.argsort(d, kind="stable")] = 1
        assert np.array_equal(np.ascontiguousarray(Vp).view(np.uint8), want.view(np.uint8)), "v is no permutation matrix to the bit"
    if kind == "zero":
        assert not w.view(np.uint8).any()  # all +0
    if kind == "rank3":
        small = np.sort(np.abs(w))[:N - 3]
        assert np.all(small <= c_res(N, sweeps, cplx) * eps * na)
        assert np.all(np.sort(np.abs(w))[N - 3:] > 1.0)  # (the three others stand clear: sums of N squares of normal values)
    if kind == "rank3+I":
        assert np.all(np.abs(w[:N - 3] - 1.0) <= c_res(N, sweeps, cplx) * eps * na) and np.all(w[N - 3:] > 2.0)


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_not_finite_gives_8_and_no_matrices(bd, dtype, cplx):
    step = 2 if cplx else 1
    for N, (i, j) in ((130, (100, 7)), (17, (5, 5))):
        base = np.array(spd(N, cplx, dtype))
        for bad in (np.nan, np.inf):
            a = base.copy()
            a[i, j * step] = bad
            code, w, v, sweeps = bd.eigh(upload(bd, a, cplx), return_sweeps=True)
            assert code == 8 and w is None and v is None and sweeps == 0, (N, bad, code)
            # the next call on the same device is correct
            w, v, sweeps = run(bd, base, cplx)
            rr, ro, _ = ratios(base, cplx, w, v, sweeps)
            assert rr <= 1.0 and ro <= 1.0


def test_codes_and_argument_errors(bd):
    import ctypes as C
    f32 = np.float32
    a = np.array(spd(8, False, f32))
    da = upload(bd, a, False)
    out = bd.eigh(da)
    assert len(out) == 3 and out[0] == 0
    out4 = bd.eigh(da, return_sweeps=True)
    assert len(out4) == 4 and out4[0] == 0 and 1 <= out4[3] <= MAX_SWEEPS
    assert np.array_equal(out[1].data().view(np.uint8), out4[1].data().view(np.uint8))
    # 7: not square
    code, w, v = bd.eigh(upload(bd, np.ones((3, 4), f32), False))
    assert code == 7 and w is None and v is None
    code, w, v = bd.eigh(upload(bd, np.ones((4, 4), f32), True))  # 4 x 2 points
    assert code == 7 and w is None and v is None
    # -1: a poisoned operand gives two poisoned results
    bad = upload(bd, np.ones((8, 16), f32), True)
    assert bad.to_complex() == -1  # a complex matrix cannot be made complex: poisoned
    code, w, v = bd.eigh(bad)
    assert code == -1 and w is not None and v is not None
    assert bd.eigh(w)[0] == -1 and bd.eigh(v)[0] == -1
    # the empty shape
    code, w, v, sweeps = bd.eigh(bd.DspMat(is_complex=False, dtype=f32, rows=0, row_len=0), return_sweeps=True)
    assert code == 0 and w is not None and v is not None and w.rows() == 0 and v.rows() == 0 and sweeps == 1
    # domain and delta come from a
    dm = bd.DspMat(a, is_complex=False, delta=0.25)
    code, w, v = bd.eigh(dm)
    assert code == 0 and w.delta() == 0.25 and v.delta() == 0.25 and w.domain() == dm.domain() and v.domain() == dm.domain()
    # Python-level errors
    with pytest.raises(TypeError):
        bd.eigh(np.ones((4, 4), f32))
    with pytest.raises(TypeError):
        bd.eigh(None, return_sweeps=True)
    # the C entry point with sweeps == NULL, in both precisions
    for dtype, sfx in ((np.float32, "32"), (np.float64, "64")):
        m = upload(bd, np.array(spd(17, True, dtype)), True)
        hw, hv = C.c_void_p(), C.c_void_p()
        rc = getattr(bd.lib, "bdsp_hip_mat_eigh" + sfx)(m._h, C.byref(hw), C.byref(hv), None)
        assert rc == 0 and hw.value and hv.value
        w = bd.DspMat(_handle=hw.value, _sfx=sfx)
        v = bd.DspMat(_handle=hv.value, _sfx=sfx)
        w0, v0, _ = run(bd, spd(17, True, dtype), True)
        assert np.array_equal(w.data()[0].view(np.uint8), w0.view(np.uint8)) and np.array_equal(v.data().view(np.uint8), v0.view(np.uint8))
        rc = getattr(bd.lib, "bdsp_hip_mat_eigh" + sfx)(upload(bd, np.ones((3, 4), dtype), False)._h, C.byref(hw), C.byref(hv), None)
        assert rc == 7 and not hw.value and not hv.value


def test_readme_music_snippet(bd):
    """The README's chain as written: two sources on a half-wavelength line array of 8 channels x 4096 complex points plus
    noise -> matmul(x, x, conj_transpose=True) -> eigh -> matmul(v, steer) with an 8 x 181 steering matrix -> transpose,
    magnitude_squared, dot_product with the mask of the 6 noise rows.  The 181 values have their two smallest local minima
    at the two source angles, and the two largest eigenvalues stand clear of the six others."""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "eigh(" in b]
    assert len(blocks) == 1
    code = blocks[0]
    for line in ("code, cov = matmul(x, x, conj_transpose=True)", "code, w, v = eigh(cov)", "code, proj = matmul(v, steer)",
                 "proj.transpose() == 0", "proj.magnitude_squared() == 0", "code, null = proj.dot_product(noise)"):
        assert line in code, line
    rng = np.random.default_rng(77)
    M, T = 8, 4096
    angles = np.arange(-90, 91)
    sources = (-20, 35)
    k = np.arange(M)[:, None]
    manifold = np.exp(1j * np.pi * k * np.sin(np.deg2rad(angles))[None, :])  # 8 x 181, half-wavelength spacing
    sig = (rng.standard_normal((2, T)) + 1j * rng.standard_normal((2, T))) / np.sqrt(2.0)
    noise = 0.1 * (rng.standard_normal((M, T)) + 1j * rng.standard_normal((M, T))) / np.sqrt(2.0)
    xs = manifold[:, [int(np.where(angles == s)[0][0]) for s in sources]] @ sig + noise
    env = {"np": np, "DspVec": bd.DspVec, "DspMat": bd.DspMat, "matmul": bd.matmul,
           "x": bd.DspMat(xs.astype(np.complex64)), "steer": bd.DspMat(manifold.astype(np.complex64))}
    exec(code, env)
    assert env["code"] == 0
    w = env["w"].data()[0]
    null = np.asarray(env["null"], dtype=np.float64)
    assert null.shape == (181,) and w.shape == (8,)
    assert w[-2:].min() > 10.0 * w[:6].max()  # two sources of power T against noise of power 0.01 T
    inner = np.arange(1, 180)
    minima = inner[(null[inner] < null[inner - 1]) & (null[inner] < null[inner + 1])]
    two = minima[np.argsort(null[minima])[:2]]
    assert sorted(int(angles[i]) for i in two) == sorted(sources), (angles[two], null[two])
