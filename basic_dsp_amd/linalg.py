"""Dense linear algebra across the rows of DspMat: the matrix product.  A module-level function, like zoom_fft: DspVec
and DspMat gain no method."""
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
