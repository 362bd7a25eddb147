"""Spectral operations beyond the reference's trait surface, as module-level functions on DspVec / DspMat."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .matrix import DspMat
from .vector import DspVec


def zoom_fft(x, start, step, bins):
    """Chirp-z transform of a frequency band, in place: every row x[0..N) of the time-domain DspVec or DspMat `x`
    (complex, or real read with a zero imaginary part) becomes

        X[k] = sum_{n<N} x[n] exp(-2 pi i (start + k step) n),   k = 0 .. bins-1

    `start` and `step` are in cycles per sample (doubles in both precisions); nothing is scaled, as in plain_fft; `step`
    may be 0 or negative and `bins` may exceed N.  For a DspMat `start` is one number for all rows, or a one-dimensional
    sequence / array with one value per row: coarse transform -> per-row peak -> every row zoomed around its own peak
    in one call.  The result is complex, in the frequency domain, `bins` points per row; delta becomes step / delta.
    start = 0, step = 1/N, bins = N is plain_fft.

    Returns the result code: 0; 7 for bins == 0, a start or step that is not finite, or a start sequence that does not
    have one value per row (the data are untouched); 5 for frequency-domain input; -1 for a poisoned input."""
    if isinstance(x, DspMat):
        if np.ndim(start) == 0:
            return _lib.check(getattr(lib, "bdsp_hip_mat_zoom_fft" + x._sfx)(x._h, float(start), float(step), int(bins)),
                              "mat_zoom_fft" + x._sfx)
        s = np.ascontiguousarray(start, dtype=np.float64)
        if s.ndim != 1:
            raise ValueError("start: a number or a one-dimensional sequence with one value per row")
        ptr = s.ctypes.data_as(C.POINTER(C.c_double))
        return _lib.check(getattr(lib, "bdsp_hip_mat_zoom_fft_starts" + x._sfx)(x._h, ptr, s.size, float(step), int(bins)),
                          "mat_zoom_fft_starts" + x._sfx)
    if isinstance(x, DspVec):
        if np.ndim(start) != 0:
            raise ValueError("start: a DspVec takes one number")
        return _lib.check(getattr(lib, "bdsp_hip_zoom_fft" + x._sfx)(x._h, float(start), float(step), int(bins)),
                          "zoom_fft" + x._sfx)
    raise TypeError("zoom_fft: a DspVec or a DspMat")
