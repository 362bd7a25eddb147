"""Detections of every row as a compact list, beyond the reference's trait surface, as module-level functions on DspVec /
DspMat, like zoom_fft, sosfilt and rank_filter: the classes gain no method."""
import ctypes as C
import numbers
import operator

import numpy as np

from . import _lib
from ._lib import lib
from .matrix import DspMat
from .vector import DspVec

_BOUNDARIES = {"open": 0, "wrap": 1, "nearest": 2}
_MODES = {"clip": "nearest", "wrap": "wrap"}  # scipy.signal.argrelmax's modes

# capacity=None: the lists of the first call; a second call of exactly the total follows only where the total is larger
FIRST_CAPACITY = 65536


def _threshold_kind(threshold):
    """(kind, payload) of the C ABI; TypeError for a threshold of no known kind"""
    if threshold is None:
        return 0, None
    if isinstance(threshold, DspMat):
        return 4, threshold
    if isinstance(threshold, DspVec):
        return 3, threshold
    if isinstance(threshold, bool) or isinstance(threshold, (str, bytes, dict, set)):
        raise TypeError("detect: a threshold is None, a real number, a sequence of real numbers, a DspVec or a DspMat")
    if isinstance(threshold, numbers.Real) or (isinstance(threshold, np.ndarray) and threshold.ndim == 0
                                               and threshold.dtype.kind in "fiu"):
        return 1, np.array([float(threshold)], dtype=np.float64)
    try:
        a = np.asarray(threshold)
    except Exception:
        raise TypeError("detect: a threshold is None, a real number, a sequence of real numbers, a DspVec or a DspMat")
    if a.dtype.kind not in "fiu" or a.ndim == 0:
        raise TypeError("detect: a threshold is None, a real number, a sequence of real numbers, a DspVec or a DspMat")
    return 2, np.ascontiguousarray(a, dtype=np.float64)


def detect(x, threshold=None, order=0, boundary="open", capacity=None):
    """The detections of the DspVec `x`, or of every row of the DspMat `x`, as a compact list, computed on the device.
    Returns (code, det); det is None unless the code is 0.  x is not modified.

    x is real, f32 or f64, in any domain.  Cell j of a row of n points is a detection iff both hold.
    Threshold, by the Python type: None, always true; a real number t, double(x[j]) > t; a sequence or array of `rows`
    numbers, double(x[r][j]) > t[r] (of one number for a DspVec; another length is 7); a real DspVec of n points of the
    same precision, one profile for all rows, x[r][j] > t[j]; a real DspMat of rows x n of the same precision, one value
    per cell, x[r][j] > t[r][j] (the CFAR floor).  Every comparison is IEEE >: a NaN on either side is never a detection,
    -0 is not above +0, denormals compare by value, +inf > t holds for finite t.
    Strict local maximum of order `order` (0: no condition): for every d with 0 < |d| <= order, x[j] > x[j + d].
    boundary says how positions outside the row are read: "open" skips the comparison, so an end point can be a peak and
    with n = 1 every cell passes; "wrap" reads index mod n, any number of turns, so order >= n compares a cell with itself
    and detects nothing; "nearest" repeats the end point (scipy's mode "clip"): an end point is never a peak for order
    >= 1.  Plateaus yield no peak; a NaN neighbour blocks a peak.

    det of a DspMat is a dict: "count", int64[rows], the true number of detections of every row; "row", "index", int64[k],
    and "value", x's dtype [k], the detections in row-major order, rows ascending and index ascending within a row; value
    holds exactly the bits of x[row, index].  det of a DspVec has an int "count" and no "row".  capacity=None lists all
    detections: one call with FIRST_CAPACITY entries, and a second call of exactly the total only where the total exceeds
    it.  An integer capacity truncates the lists to the first `capacity` detections; count stays true, and capacity 0
    skips the write launch.  Only the counts and the listed entries are copied to the host.

    Codes: 0; 7 for an order or capacity that is not a non-negative integer, an unknown boundary, a sequence of the wrong
    length or a DspMat threshold for a DspVec, all before any device call; 2 for a device threshold of another precision;
    -1 for a poisoned x or threshold; 4 for complex data; for a DspVec or DspMat threshold the size and meta-data codes of
    add (7 for another row count, 1, 2); in that order.  order above 1024 (DETECT_MAX_ORDER) and rows x tiles above 2^31
    raise BackendError (the backend's unsupported code).  No rows, or rows of no points, give 0 and empty lists.
    TypeError, before any device call, for an x that is not a DspVec or DspMat and for a threshold of no known kind.

    Deterministic: four launches whatever the row count (count per tile, prefix over the tiles of each row, prefix over
    the rows, write), no atomics; the list is a function of the data and the arguments only: row r of the matrix call
    equals the vector call on that row."""
    if isinstance(x, DspMat):
        name, mat = "bdsp_hip_mat_detect", True
    elif isinstance(x, DspVec):
        name, mat = "bdsp_hip_detect", False
    else:
        raise TypeError("detect: a DspVec or a DspMat")
    kind, payload = _threshold_kind(threshold)
    code = _BOUNDARIES.get(boundary) if isinstance(boundary, str) else None
    try:
        order = operator.index(order)
        capacity = None if capacity is None else operator.index(capacity)
    except TypeError:
        return 7, None
    if code is None or not 0 <= order < 1 << 64 or (capacity is not None and capacity < 0):
        return 7, None
    if kind == 4 and not mat:
        return 7, None
    if kind >= 3 and payload._sfx != x._sfx:
        return 2, None
    rows = x.rows() if mat else 1
    cells = rows * x.row_len() if mat else len(x)
    if kind == 2:
        if payload.ndim != 1 or payload.size != rows:
            return 7, None
        if not mat:
            kind = 1
    tptr = None if kind == 0 else C.c_void_p(payload._h) if kind >= 3 else payload.ctypes.data_as(C.c_void_p)
    fn = getattr(lib, name + x._sfx)
    counts = np.zeros(max(rows, 1), dtype=np.int64)

    def call(cap):
        index, value = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=x.dtype)
        c = _lib.check(fn(x._h, kind, tptr, order, code, cap, counts.ctypes.data_as(C.c_void_p),
                          index.ctypes.data_as(C.c_void_p) if cap else None, value.ctypes.data_as(C.c_void_p) if cap else None),
                       name[len("bdsp_hip_"):] + x._sfx)
        return c, index, value

    cap = min(FIRST_CAPACITY if capacity is None else capacity, cells)
    c, index, value = call(cap)
    if c != 0:
        return c, None
    total = int(counts[:rows].sum())
    if capacity is None and total > cap:
        cap = total
        c, index, value = call(cap)
        if c != 0:
            return c, None
    k = min(total, cap)
    det = {"count": counts[:rows].copy() if mat else int(counts[0])}
    if mat:
        det["row"] = np.repeat(np.arange(rows, dtype=np.int64), counts[:rows])[:k]
    det["index"], det["value"] = index[:k].copy(), value[:k].copy()
    return 0, det


def argrelmax(x, order=1, mode="clip"):
    """scipy.signal.argrelmax(data, axis=-1, order=order, mode=mode) of the DspVec `x` or of every row of the DspMat `x`,
    through the same C entry as detect: detect(x, None, order, "nearest" for mode "clip" or "wrap" for mode "wrap").
    Returns (code, (index,)) for a DspVec and (code, (row, index)) for a DspMat, int64 arrays in row-major order; the tuple
    is None unless the code is 0.  7 for an order below 1 or not an integer and for an unknown mode; every other code is
    detect's.  TypeError, before any device call, for an x that is not a DspVec or DspMat."""
    if not isinstance(x, (DspVec, DspMat)):
        raise TypeError("argrelmax: a DspVec or a DspMat")
    try:
        order = operator.index(order)
    except TypeError:
        return 7, None
    if order < 1 or not isinstance(mode, str) or mode not in _MODES:
        return 7, None
    code, det = detect(x, None, order, _MODES[mode])
    if code != 0:
        return code, None
    return 0, ((det["row"], det["index"]) if isinstance(x, DspMat) else (det["index"],))
