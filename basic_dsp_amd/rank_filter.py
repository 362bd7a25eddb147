"""Sliding order statistics beyond the reference's trait surface, as module-level functions on DspVec / DspMat, like
zoom_fft and sosfilt: the classes gain no method."""
import operator

from . import _lib
from ._lib import lib
from .matrix import DspMat
from .vector import DspVec

_BOUNDARIES = {"zero": 0, "wrap": 1, "nearest": 2}


def rank_filter(x, half, rank, guard=None, boundary="zero"):
    """Replace every point of the DspVec `x`, or of every row of the DspMat `x`, by the element of rank `rank` of the
    window around it, in place, on the device.  Returns the result code.

    x is real, f32 or f64, in any domain (magnitude spectra are real frequency-domain data); length, domain, delta and
    number kind stay.  For point i of a row of n points the window is the multiset x[i + d], guard < |d| <= half; with
    guard=None it is all |d| <= half, the centre included.  So W = 2 half + 1 without a guard and 2 (half - guard) with
    one.  The result is the window's element of rank `rank`: 0 the smallest, W - 1 the largest.  Every result is computed
    from the row as it was on entry.  rank 0 and W - 1 are the running minimum and maximum (erosion, dilation, envelopes);
    a guard gives the ordered-statistic CFAR noise floor: the k-th smallest of the training cells around every cell, the
    cell and its guard cells excluded.

    boundary says how positions outside the row are read: "zero" as +0.0 (scipy.signal.medfilt's rule), "wrap" as index
    mod n (the rule of the library's circular convolve; correct also where half >= n and the window wraps more than
    once), "nearest" as the row's first or last point.

    Order: IEEE totalOrder on the bit patterns, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN; the kernel compares the
    keys bits ^ (sign ? all ones : sign bit) as unsigned integers.  The output carries exactly the bits of the selected
    input, NaN payloads and denormals included: no flush and no arithmetic touches a value.

    Codes: 0; 7, with the data untouched, for rank >= W, guard >= half, an unknown boundary or an argument that is not a
    non-negative integer; -1 for a poisoned x; 4 for complex data; in that order.  half above 1024 (RANK_MAX_HALF) and
    rows x tiles above 2^31 raise BackendError (the backend's unsupported code).  No rows, or rows of no points, give 0
    and change nothing.  TypeError, before any device call, for an x that is not a DspVec or DspMat.

    Deterministic: one launch whatever the row count; short windows count ranks, long windows bisect the key, chosen by W
    and the precision alone, neither with an early exit.  The result depends on the row and the arguments only: row r of
    the matrix call is bit-equal to the vector call on that row."""
    if isinstance(x, DspMat):
        name = "bdsp_hip_mat_rank_filter"
    elif isinstance(x, DspVec):
        name = "bdsp_hip_rank_filter"
    else:
        raise TypeError("rank_filter: a DspVec or a DspMat")
    code = _BOUNDARIES.get(boundary) if isinstance(boundary, str) else None
    try:
        half, rank, guard = operator.index(half), operator.index(rank), None if guard is None else operator.index(guard)
    except TypeError:
        return 7
    if code is None or not (0 <= half < 1 << 64 and 0 <= rank < 1 << 64 and (guard is None or 0 <= guard < 1 << 63)):
        return 7
    return _lib.check(getattr(lib, name + x._sfx)(x._h, half, rank, -1 if guard is None else guard, code),
                      name[len("bdsp_hip_"):] + x._sfx)


def medfilt(x, kernel_size=3, boundary="zero"):
    """The median filter of scipy.signal.medfilt along the DspVec `x` or every row of the DspMat `x`, in place:
    rank_filter(x, (k - 1) // 2, (k - 1) // 2, None, boundary) with k = kernel_size, through the same C entry.  Returns
    7, with the data untouched, for an even or zero kernel_size; every other code, the order of the values (IEEE
    totalOrder on the bit patterns: a NaN is the largest or, with its sign set, the smallest value, never contagious)
    and the boundary rules are rank_filter's.  TypeError, before any device call, for an x that is not a DspVec or
    DspMat."""
    if not isinstance(x, (DspVec, DspMat)):
        raise TypeError("medfilt: a DspVec or a DspMat")
    try:
        kernel_size = operator.index(kernel_size)
    except TypeError:
        return 7
    if kernel_size <= 0 or kernel_size % 2 == 0:
        return 7
    return rank_filter(x, (kernel_size - 1) // 2, (kernel_size - 1) // 2, None, boundary)
