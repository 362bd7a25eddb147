"""Recursive (IIR) filtering beyond the reference's trait surface, as a module-level function on DspVec / DspMat, like
zoom_fft: the classes gain no method."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .matrix import DspMat
from .vector import DspVec


def sosfilt(x, sos, state=None):
    """Filter the DspVec `x`, or every row of the DspMat `x`, with a cascade of second-order sections, in place, on the
    device.  Returns the result code.

    x is real or complex, f32 or f64, in the time domain; length, domain, delta and number kind stay.  Complex data are
    filtered as two independent real signals, because the coefficients are real.  sos is a host array shaped [S, 6] of
    doubles, one row b0 b1 b2 a0 a1 a2 per section: the layout scipy's output='sos' produces.  Every section is divided
    by its a0 in double, then rounded once to the data's precision.  Each section is direct form II transposed,

        y = b0 x + s1,   s1 <- b1 x - a1 y + s2,   s2 <- b2 x - a2 y,

    the form and state convention of scipy.signal.sosfilt; the sections are applied in order.  state is None (a zero
    initial state; the final state is dropped), or for a DspVec a DspVec of 2 S points and for a DspMat a DspMat of
    rows x 2 S points, of the number kind and precision of x: s1, s2 of section 0, then of section 1, and so on.  It is
    read as the initial state and overwritten with the state after the last point, so a recording can be filtered block
    after block without leaving the device.  The zero-phase filter is a composition: sosfilt, reverse, sosfilt, reverse.

    Codes: 0; -1 for a poisoned x or state; 5 for frequency-domain x; 2 for a state of the other number kind; 7, with the
    data untouched, for a sos that is not [S, 6], a coefficient that is not finite, a0 == 0, S above 16 or a state of the
    wrong shape.  S == 0, no rows, or rows of no points give 0 and change nothing.  An unstable filter gives inf or NaN
    exactly as the recurrence would, with code 0: nothing is tested.  TypeError, before any device call, for an x that is
    not a DspVec or DspMat and for a state of another class or precision.  A failed allocation raises BackendError.

    Deterministic: one algorithm whatever the row count.  A row is cut into tiles of 4096 points and a tile into 256
    chunks of 16; the chunk states are combined by a fixed tree and every chunk is run again from its true state.  The
    result depends on (row length, sos, number kind, precision, incoming state) only, never on the row count, the
    device's CU count or on timing: row r of the matrix call is bit-equal to the vector call on that row.  One launch for
    rows of at most 4096 points, else three.  The call uploads its coefficient tables, so it cannot be captured into a
    Graph."""
    if isinstance(x, DspMat):
        name = "bdsp_hip_mat_sosfilt"
    elif isinstance(x, DspVec):
        name = "bdsp_hip_sosfilt"
    else:
        raise TypeError("sosfilt: a DspVec or a DspMat")
    if state is not None and (type(state) is not type(x) or state._sfx != x._sfx):
        raise TypeError("sosfilt: state is None or %s of the precision of x" % ("a DspMat" if isinstance(x, DspMat) else "a DspVec"))
    try:
        c = np.ascontiguousarray(sos, dtype=np.float64)
    except (TypeError, ValueError):
        return 7
    if c.ndim != 2 or c.shape[1] != 6:
        return 7
    ptr = c.ctypes.data_as(C.POINTER(C.c_double))
    return _lib.check(getattr(lib, name + x._sfx)(x._h, ptr, c.shape[0], state._h if state is not None else None),
                      name[len("bdsp_hip_"):] + x._sfx)
