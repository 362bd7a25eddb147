"""Order statistics of every row, beyond the reference's trait surface, as module-level functions on DspVec / DspMat, like
zoom_fft, sosfilt, rank_filter and detect: the classes gain no method."""
import ctypes as C
import numbers
import operator

import numpy as np

from . import _lib
from ._lib import lib
from .matrix import DspMat
from .vector import DspVec

_METHODS = ("linear", "lower", "higher")


def _target(x, what):
    """(is a matrix, rows, n) of x; TypeError for anything but a DspVec or a DspMat"""
    if isinstance(x, DspMat):
        return True, x.rows(), x.row_len()
    if isinstance(x, DspVec):
        return False, 1, len(x)
    raise TypeError("%s: a DspVec or a DspMat" % what)


def _flag(value):
    """0 / 1 of a bool or of the integers 0 and 1, else None"""
    if isinstance(value, (bool, np.bool_)):
        return int(value)
    if isinstance(value, numbers.Integral) and value in (0, 1):
        return int(value)
    return None


def _select(x, mat, rows, descending, count, ranks, want_index, want_value, what):
    """bdsp_hip_(mat_)order_select: (code, int64[rows, count] or None, x.dtype[rows, count] or None)"""
    name = "bdsp_hip_mat_order_select" if mat else "bdsp_hip_order_select"
    index = np.empty((rows, count), dtype=np.int64) if want_index else None
    value = np.empty((rows, count), dtype=x.dtype) if want_value else None
    rptr = None if ranks is None else ranks.ctypes.data_as(C.c_void_p)
    code = _lib.check(getattr(lib, name + x._sfx)(x._h, descending, count, rptr,
                                                  index.ctypes.data_as(C.c_void_p) if want_index else None,
                                                  value.ctypes.data_as(C.c_void_p) if want_value else None),
                      name[len("bdsp_hip_"):] + x._sfx)
    return code, index, value


def sort(x, descending=False):
    """Sort the DspVec `x`, or every row of the DspMat `x`, in place, on the device.  Returns the result code.

    x is real, f32 or f64, in any domain; length, domain, delta and number kind stay.
    Order: ascending is IEEE totalOrder on the bit patterns, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN; the kernels
    compare the keys k = bits ^ (sign ? all ones : sign bit) as unsigned integers.  Descending is the ascending order of
    the complemented key ~k: +NaN first.  The output carries exactly the bits of the inputs, NaN payloads and denormals
    included: no flush and no arithmetic touches a value.  sort carries no index: equal keys are equal bits.

    Codes: 0; 7, with the data untouched, for a `descending` that is not a bool (or 0 / 1), before any device call; -1 for
    a poisoned x; 4 for complex data; in that order.  n at or above 2^32 and rows x tiles above 2^31 raise BackendError (the
    backend's unsupported code).  No rows, or rows of no points, give 0 and change nothing.  TypeError, before any device
    call, for an x that is not a DspVec or DspMat.

    Deterministic: 1 + P launches whatever the row count, P = ceil(log2(ceil(n / 4096))): one launch sorts tiles of 4096
    points (rows of at most 2048 points share a workgroup, 4096 / p of them, p the power of two >= n) with a bitonic
    network in registers and LDS; P merge passes follow, between the live and the trade buffer.  No atomics, no early
    exit: the result is a function of the input bits alone, and row r of the matrix call is bit-equal to the vector call
    on that row."""
    if isinstance(x, DspMat):
        name = "bdsp_hip_mat_sort"
    elif isinstance(x, DspVec):
        name = "bdsp_hip_sort"
    else:
        raise TypeError("sort: a DspVec or a DspMat")
    flag = _flag(descending)
    if flag is None:
        return 7
    return _lib.check(getattr(lib, name + x._sfx)(x._h, flag), name[len("bdsp_hip_"):] + x._sfx)


def argsort(x, descending=False):
    """The permutation that sorts the DspVec `x`, or every row of the DspMat `x`.  Returns (code, index): int64[rows, n]
    for a DspMat, int64[n] for a DspVec, None unless the code is 0.  x is not modified.

    index[r, j] is the position in row r of the element of rank j.  Order and codes are sort's (totalOrder on the bit
    patterns); ties are broken by ascending index, so the permutation is the stable one, np.argsort(key, kind="stable").
    Descending is the stable ascending sort of the complemented key: largest first, and among equal bit patterns the
    lower index first; it is not the reverse of the ascending permutation.

    2 + P launches whatever the row count (tile sort of (key, index) pairs, P merge passes, gather), in two workspaces of
    rows x n x (4 + 4) or (8 + 4) bytes, one synchronisation.  No rows, or rows of no points, give 0 and an empty array."""
    if not isinstance(x, (DspVec, DspMat)):
        raise TypeError("argsort: a DspVec or a DspMat")
    flag = _flag(descending)
    if flag is None:
        return 7, None
    mat, rows, n = _target(x, "argsort")
    code, index, _ = _select(x, mat, rows, flag, n, None, True, False, "argsort")
    if code != 0:
        return code, None
    return 0, index if mat else index[0]


def top_k(x, k, largest=True):
    """The k largest (largest=False: smallest) elements of the DspVec `x`, or of every row of the DspMat `x`.  Returns
    (code, {"index": int64[rows, k], "value": x's dtype [rows, k]}) ([k] for a DspVec); the dict is None unless the code is
    0.  x is not modified.

    Entry j is the element of rank j of the descending order (largest=False: of the ascending order) of sort and argsort:
    totalOrder on the bit patterns, so a +NaN is the largest value; among equal bit patterns the lower index comes first.
    value holds exactly the bits of x[row, index].  Only the rows x k entries are copied to the host.  Today a top_k is the
    full sort and a crop: there is no partial selection for k far below n, and the cost is argsort's.

    Codes: 0; 7 for a k that is not a non-negative integer or a `largest` that is not a bool, before any device call, and
    for k > n; then sort's.  k = 0 gives empty arrays and 0."""
    if not isinstance(x, (DspVec, DspMat)):
        raise TypeError("top_k: a DspVec or a DspMat")
    flag = _flag(largest)
    try:
        k = operator.index(k)
    except TypeError:
        return 7, None
    if flag is None or k < 0:
        return 7, None
    mat, rows, n = _target(x, "top_k")
    if k > n:
        return 7, None
    code, index, value = _select(x, mat, rows, flag, k, None, True, True, "top_k")
    if code != 0:
        return code, None
    return 0, {"index": index if mat else index[0], "value": value if mat else value[0]}


def _quantile_args(q, method):
    """(q as float64[Q], scalar) or None"""
    if not isinstance(method, str) or method not in _METHODS:
        return None
    if isinstance(q, (bool, np.bool_, str, bytes)):
        return None
    try:
        a = np.asarray(q, dtype=np.float64)
    except (TypeError, ValueError):
        return None
    if a.ndim > 1 or a.size == 0 and a.ndim == 0:
        return None
    flat = a.reshape(-1)
    if not np.all((flat >= 0.0) & (flat <= 1.0)):  # (a NaN fails both)
        return None
    return flat, a.ndim == 0


def quantile(x, q, method="linear"):
    """The quantiles q of the DspVec `x`, or of every row of the DspMat `x`.  Returns (code, float64[rows, Q]) ([Q] for a
    DspVec; a scalar q drops the Q axis); the array is None unless the code is 0.  x is not modified.

    q lies in [0, 1].  With v the sorted row of n points (sort's order), the position is p = q (n - 1), computed in double
    on the host, lo = floor(p), hi = min(lo + 1, n - 1), g = p - lo.  "lower" gives v[lo], "higher" gives v[ceil(p)],
    "linear" gives v[lo] exactly if g == 0 or v[lo] and v[hi] have equal bits, else double(v[lo]) + (double(v[hi]) -
    double(v[lo])) g.  The device selects the order statistics (argsort's launches; only the ranks that the q need come to
    the host); the host does this one line of arithmetic in double.
    NaNs sit at the two ends of totalOrder: -NaN first, +NaN last.  A quantile that touches one is NaN and no other is.
    This differs from numpy, where one NaN poisons every quantile.

    Codes: 0; 7 for a q outside [0, 1], a NaN q, a q that is no real number or 1-D sequence of them, or an unknown method,
    before any device call, and for rows of no points; then sort's."""
    if not isinstance(x, (DspVec, DspMat)):
        raise TypeError("quantile: a DspVec or a DspMat")
    args = _quantile_args(q, method)
    if args is None:
        return 7, None
    qs, scalar = args
    mat, rows, n = _target(x, "quantile")
    if n == 0:
        return 7, None
    pos = qs * float(n - 1)
    lo = np.floor(pos).astype(np.int64)
    up = np.ceil(pos).astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    g = pos - lo
    ranks = np.unique(np.concatenate([lo, hi, up])).astype(np.uint64)
    code, _, value = _select(x, mat, rows, 0, ranks.size, ranks, False, True, "quantile")
    if code != 0:
        return code, None
    where = {int(r): j for j, r in enumerate(ranks)}
    bits = value.view(np.uint32 if x._sfx == "32" else np.uint64)
    out = np.empty((rows, qs.size), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):  # (a signalling NaN converts quietly; inf - inf is the NaN it should be)
        wide = value.astype(np.float64)
        for j in range(qs.size):
            jl, jh, ju = where[int(lo[j])], where[int(hi[j])], where[int(up[j])]
            vl, vh = wide[:, jl], wide[:, jh]
            if method == "lower":
                out[:, j] = vl
            elif method == "higher":
                out[:, j] = wide[:, ju]
            elif g[j] == 0.0:
                out[:, j] = vl
            else:
                out[:, j] = np.where(bits[:, jl] == bits[:, jh], vl, vl + (vh - vl) * g[j])
    if not mat:
        out = out[0]
    if scalar:
        out = out[..., 0]
    return 0, out


def median(x):
    """quantile(x, 0.5): the middle element of every row of odd n, the mean of the two middle ones of even n (exactly that
    element where both have equal bits), through the same C entry.  Returns (code, float64[rows]) (a float64 scalar for a
    DspVec).  Order, NaN rule and codes are quantile's: a row's median is NaN only where a middle element is one."""
    if not isinstance(x, (DspVec, DspMat)):
        raise TypeError("median: a DspVec or a DspMat")
    return quantile(x, 0.5)
