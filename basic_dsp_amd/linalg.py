"""Dense linear algebra across the rows of DspMat: the matrix product, the Cholesky factorisation, the solves with its
factor and the Hermitian eigendecomposition.  Module-level functions, like zoom_fft: DspVec and DspMat gain no method."""
import ctypes as C

from . import _lib
from ._lib import lib
from .matrix import DspMat


def matmul(a, b, conj_transpose=False):
    """(code, DspMat-or-None): the product of two DspMat on the device.  Sizes in points.

        matmul(a, b)                       a: M x K, b: K x N  ->  M x N,  y[i, n] = sum_k a[i, k] * b[k, n]
        matmul(a, b, conj_transpose=True)  a: M x K, b: N x K  ->  M x N,  r[i, j] = sum_k a[i, k] * conj(b[j, k])

    matmul(x, x, conj_transpose=True) is the Gram / covariance matrix of the rows of x (the same object twice is
    allowed); it is Hermitian to the bit and its diagonal has imaginary part +0.  Both operands are real or both are
    complex (use to_complex() for real weights on complex data); the result has their number space, and for real operands
    conj is the identity.  Domains and deltas need not agree: the result takes domain and delta from the operand whose row
    axis survives, b in the plain form and a in the transposed one.  Both operands stay untouched; rows may start on any
    element boundary.  A complex product is four real products, and every element is within (2 K + 4) eps
    sum_k |a[i, k]| |b[k, n]| of the exact value.

    Codes: 0; -1 for a poisoned operand (the result is poisoned too); 2 for a real and a complex operand (no matrix); 7
    unless a.row_points() == b.rows() (plain) or a.row_points() == b.row_points() (transposed) (no matrix).  Empty shapes
    give 0: K == 0 an M x N matrix of +0, M == 0 a matrix without rows, N == 0 M empty rows.  A failed allocation or a
    result too long for the address space raises BackendError.  TypeError for anything that is not two DspMat of one
    precision.

    Deterministic: the path and the order of summation depend on (M, N, K, number kind, precision, form) only, never on
    the device's CU count or on timing; the same call gives the same bits on every run.  One launch, or two where a long
    K is cut into chunks (K >= 256 with at most 64 tiles of 64 x 64 outputs).  Allocates its result, so it cannot be
    captured into a Graph."""
    if not isinstance(a, DspMat) or not isinstance(b, DspMat):
        raise TypeError("matmul: two DspMat")
    if a._sfx != b._sfx:
        raise TypeError("matmul: two DspMat of one precision")
    out = C.c_void_p()
    code = _lib.check(getattr(lib, "bdsp_hip_mat_matmul" + a._sfx)(a._h, b._h, int(bool(conj_transpose)), C.byref(out)),
                      "mat_matmul" + a._sfx)
    return code, (DspMat(_handle=out.value, _sfx=a._sfx) if out.value else None)


_PARTS = {"both": 0, "forward": 1, "backward": 2}


def cholesky(a, loading=0.0):
    """(code, DspMat-or-None): the lower Cholesky factor L of a Hermitian positive-definite DspMat, a = L . L^H, on the
    device.

    a is N x N points, real (symmetric) or complex (Hermitian), f32 or f64.  Only the lower triangle is read, and of the
    diagonal only the real part: the upper triangle and the diagonal's imaginary parts may hold anything, NaN included,
    and do not change a bit of the result.  loading (a float) is rounded once to the matrix's precision and added to every
    diagonal element as it is read, with one rounding: diagonal loading, R + s^2 I, the ordinary cure for a sample
    covariance of fewer snapshots than channels.  a stays untouched.  L is a new N x N matrix: lower triangular, its
    diagonal real and > 0 with imaginary part +0, every element above the diagonal +0, domain and delta from a.  With A the
    loaded matrix, |A - L L^H| <= (2 N + 4) eps |L| |L|^H element by element.

    Codes: 0; -1 for a poisoned operand (the result is poisoned too); 7 unless a.rows() == a.row_points() (no matrix); 8
    when a pivot is <= 0 or not finite, so a is not the Hermitian positive-definite matrix the call needs (no matrix) --
    one 4-byte read-back after the last launch, the only synchronisation of the call.  N == 0 gives 0 and an empty
    matrix.  A failed allocation raises BackendError.  TypeError for anything that is not a DspMat.

    Deterministic: the path and the order of operations depend on (N, number kind, precision) only, never on the device's
    CU count or on timing; the same call gives the same bits on every run.  One launch for N <= 64, else blocks of 64 and
    2 ceil(N / 64) - 1 launches.  Allocates its result, so it cannot be captured into a Graph."""
    if not isinstance(a, DspMat):
        raise TypeError("cholesky: a DspMat")
    out = C.c_void_p()
    code = _lib.check(getattr(lib, "bdsp_hip_mat_cholesky" + a._sfx)(a._h, float(loading), C.byref(out)), "mat_cholesky" + a._sfx)
    return code, (DspMat(_handle=out.value, _sfx=a._sfx) if out.value else None)


def cholesky_solve(l, b, part="both"):
    """(code, DspMat-or-None): solve with a Cholesky factor on the device.  Sizes in points.

        cholesky_solve(l, b)                    l: N x N, b: N x P  ->  X: N x P,  l l^H X = b   (A^-1 b)
        cholesky_solve(l, b, part="forward")    l X = b      (L^-1 b: whitening)
        cholesky_solve(l, b, part="backward")   l^H X = b    (L^-H b)

    l is a factor as cholesky returns it; only its lower triangle is read, and of its diagonal only the real part.  "both"
    is the forward pass followed by the backward pass, bit for bit.  X is a new matrix with domain and delta from b; both
    operands stay untouched.  Element by element |b - l X| <= (2 N + 4) eps |l| |X| (forward; backward with l^H) and
    |b - l l^H X| <= 3 (2 N + 4) eps |l| |l|^H |X| (both).

    Codes: 0; -1 for a poisoned operand (the result is poisoned too); 2 for a real and a complex operand (no matrix); 7
    unless l is square and l.rows() == b.rows() (no matrix).  P == 0 gives N empty rows, N == 0 a matrix without rows.  A
    zero on l's diagonal gives inf / NaN in the result and code 0, as in any triangular solve: nothing is tested and
    nothing is read back, so this call does not synchronise.  ValueError for any other part; TypeError for anything that
    is not two DspMat of one precision; a failed allocation raises BackendError.

    Deterministic: the path and the order of operations depend on (N, P, number kind, precision, part) only.  One launch
    per triangular pass for N <= 64 (l in LDS, one thread per column of b, b read once and X written once), else
    2 ceil(N / 64) - 1 launches per pass, whatever P.  Allocates its result, so it cannot be captured into a Graph."""
    if not isinstance(l, DspMat) or not isinstance(b, DspMat):
        raise TypeError("cholesky_solve: two DspMat")
    if l._sfx != b._sfx:
        raise TypeError("cholesky_solve: two DspMat of one precision")
    if not isinstance(part, str) or part not in _PARTS:
        raise ValueError("cholesky_solve: part is 'both', 'forward' or 'backward'")
    out = C.c_void_p()
    code = _lib.check(getattr(lib, "bdsp_hip_mat_cholesky_solve" + l._sfx)(l._h, b._h, _PARTS[part], C.byref(out)),
                      "mat_cholesky_solve" + l._sfx)
    return code, (DspMat(_handle=out.value, _sfx=l._sfx) if out.value else None)


def eigh(a, return_sweeps=False):
    """(code, w, v) or, with return_sweeps, (code, w, v, sweeps): the eigendecomposition of a Hermitian DspMat on the
    device.

    a is N x N points, real (symmetric) or complex (Hermitian), f32 or f64.  Only the lower triangle is read, and of the
    diagonal only the real part: the upper triangle and the diagonal's imaginary parts may hold anything, NaN included,
    and do not change a bit of the result.  a stays untouched.  w is a new real DspMat of 1 row x N points: the
    eigenvalues in ascending order, ties in the order of the index a value had before sorting.  v is a new N x N DspMat of
    a's number kind; both take domain and delta from a.  Row k of v is the k-th eigenvector conjugate-transposed:
    v a v^H = diag(w) and v v^H = I, so matmul(v, x) is the KLT / the principal components of the rows of x, and a
    subspace is a set of rows.  The phase of a row is arbitrary but reproducible.  sweeps counts the sweeps taken, the
    last one, which rotated nothing, included: 1 for the identity, a diagonal matrix and the zero matrix, whose v is a
    permutation matrix to the bit.

    Codes: 0; -1 for a poisoned operand (w and v are poisoned too); 7 unless a.rows() == a.row_points() (w and v are
    None); 8 when the Frobenius norm of the matrix as read is not finite -- a NaN or an infinity in what is read, or
    squares that overflow -- or when the iteration has not converged after 30 sweeps (w and v are None; sweeps is 0).
    N == 0 gives 0 and two empty matrices.  A failed allocation raises BackendError.  TypeError for anything that is not a
    DspMat.

    Method: cyclic two-sided Jacobi in the round-robin ordering; a pair (p, q) is rotated iff |a_pq| > eps |a|_F / N.  In
    Frobenius norms |a - v^H diag(w) v| <= c_res(N, sweeps) eps |a| and |v v^H - I| <= c_orth(N, sweeps) eps with
    c_orth = 2 K sweeps sqrt(N), c_res = 2 K sweeps (1 + sqrt(N)) + 1; K = rho N for N <= 64, else 8 (128 rho + 132)
    times the block steps of a sweep; rho = 24 (real), 40 (complex).

    Deterministic: the path, the ordering and the order of operations depend on (N, number kind, precision) only, never
    on the device's CU count or on timing; the same call gives the same bits on every run.  One launch and one 4-byte
    read-back for N <= 64; else blocks of 32 columns, 3 launches per block step and one small read-back per sweep.
    Allocates its results, so it cannot be captured into a Graph."""
    if not isinstance(a, DspMat):
        raise TypeError("eigh: a DspMat")
    w, v, sweeps = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    code = _lib.check(getattr(lib, "bdsp_hip_mat_eigh" + a._sfx)(a._h, C.byref(w), C.byref(v), C.byref(sweeps)), "mat_eigh" + a._sfx)
    wm = DspMat(_handle=w.value, _sfx=a._sfx) if w.value else None
    vm = DspMat(_handle=v.value, _sfx=a._sfx) if v.value else None
    return (code, wm, vm, int(sweeps.value)) if return_sweeps else (code, wm, vm)
