"""Host-side mirror of the reference's matrix crate for the hot path (matrix/src/lib.rs,
matrix/src/time_freq.rs): `DspMat` = a set of equally long row vectors that live in ONE HBM
allocation; every method is a batched launch over all rows (the reference loops over the rows on
one CPU thread, matrix/src/lib.rs:195-208).  Methods return the facade result codes like DspVec.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .vector import DspVec, TIME, PAD_END


class DspMat:
    def __init__(self, rows_data=None, is_complex=False, domain=TIME, delta=1.0, dtype=np.float32,
                 rows=None, row_len=None, _handle=None, _sfx=None):
        if _handle is not None:
            self._h, self._sfx = _handle, _sfx
            self.dtype = np.float32 if _sfx == "32" else np.float64
            return
        _lib.require_gpu()
        if rows_data is not None:
            a = np.ascontiguousarray(rows_data)
            if a.dtype in (np.complex64, np.complex128):
                is_complex = True
                a = a.view(np.float32 if a.dtype == np.complex64 else np.float64)
            assert a.ndim == 2, "rows_data must be [rows, row_len]"
            dtype, (rows, row_len) = a.dtype, a.shape
        self.dtype = np.dtype(dtype).type
        self._sfx = "32" if self.dtype == np.float32 else "64"
        h = self._fn("new")(int(bool(is_complex)), int(domain), int(rows), int(row_len), delta)
        if not h:
            raise _lib.BackendError("mat_new%s failed: %s" % (self._sfx, _lib.last_error()))
        self._h = h
        if rows_data is not None and a.size:
            _lib.check(self._fn("upload")(self._h, a.ctypes.data_as(C.c_void_p), a.size), "mat_upload")

    def _fn(self, name):
        return getattr(lib, "bdsp_hip_mat_" + name + self._sfx)

    def _call(self, name, *args):
        return _lib.check(self._fn(name)(self._h, *args), "mat_" + name + self._sfx)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._fn("delete")(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    # ------------------------------------------------------------------ metadata / transfer
    def rows(self):
        return self._fn("rows")(self._h)

    def row_len(self):
        return self._fn("row_len")(self._h)

    def row_points(self):
        return self._fn("row_points")(self._h)

    def is_complex(self):
        return bool(self._fn("is_complex")(self._h))

    def domain(self):
        return self._fn("get_domain")(self._h)

    def delta(self):
        return self._fn("get_delta")(self._h)

    def device_ptr(self):
        return self._fn("device_ptr")(self._h)

    def data(self):
        """Download as a [rows, row_len] array of scalars (interleaved if complex)."""
        out = np.empty((self.rows(), self.row_len()), dtype=self.dtype)
        if out.size:
            _lib.check(self._fn("download")(self._h, out.ctypes.data_as(C.c_void_p), out.size), "mat_download")
        return out

    def get_row(self, row):
        h = self._fn("get_row")(self._h, int(row))
        if not h:
            raise IndexError(row)
        return DspVec(_handle=h, _sfx=self._sfx)

    def set_row(self, row, vector):
        return self._call("set_row", int(row), vector._h)

    # ------------------------------------------------------------------ vector <-> matrix
    # A signal that lives in HBM becomes a batch and a batch becomes a signal again without a host round trip: one
    # launch each, whatever the number of rows.  All three allocate their result, so none can be captured into a Graph.
    @classmethod
    def from_frames(cls, vector, frame_points, hop, pad_tail=False):
        """(code, DspMat-or-None): the overlapping frames of the DspVec `vector` as rows -- row r, point j is
        x[r * hop + j], positions past the end read as zero (frame_points and hop in points; the analysis step of an
        STFT).  Rows: (points - frame_points) // hop + 1 whole frames (none if the vector is shorter than a frame); with
        pad_tail a last, zero-extended frame covers the tail, ceil((points - frame_points) / hop) + 1 (one row for a
        vector no longer than a frame, none for an empty one).  Number space, domain and delta are the vector's, which
        stays as it is.  Bit-exact.  Codes: 0; 7 if frame_points or hop is 0 (no matrix); -1 for a poisoned vector (the
        matrix is poisoned too).  Allocates, so it cannot be captured into a Graph."""
        out = C.c_void_p()
        fn = getattr(lib, "bdsp_hip_mat_from_frames" + vector._sfx)
        code = _lib.check(fn(vector._h, int(frame_points), int(hop), int(bool(pad_tail)), C.byref(out)),
                          "mat_from_frames" + vector._sfx)
        return code, (cls(_handle=out.value, _sfx=vector._sfx) if out.value else None)

    @classmethod
    def from_vectors(cls, vectors, dtype=np.float32):
        """(code, DspMat-or-None): row r is a copy of the DspVec vectors[r] (the reference's to_mat); number space,
        domain and delta are the first vector's.  One pointer-table upload and one launch, however many vectors.  An
        empty list gives a real matrix of `dtype` without rows.  Codes: 0; -1 if any vector is poisoned (the matrix is
        poisoned too); 7 for unequal lengths, 2 for unequal number space or domain (no matrix).  Allocates, so it cannot be
        captured into a Graph."""
        vectors = list(vectors)
        sfx = vectors[0]._sfx if vectors else ("32" if np.dtype(dtype).type == np.float32 else "64")
        assert all(v._sfx == sfx for v in vectors), "vectors of one precision"
        out = C.c_void_p()
        arr = (C.c_void_p * max(len(vectors), 1))(*[v._h for v in vectors])
        code = _lib.check(getattr(lib, "bdsp_hip_mat_from_vectors" + sfx)(arr, len(vectors), C.byref(out)),
                          "mat_from_vectors" + sfx)
        return code, (cls(_handle=out.value, _sfx=sfx) if out.value else None)

    def overlap_add(self, hop):
        """(code, DspVec-or-None): the rows summed into one vector, row r starting at point r * hop -- (rows - 1) * hop +
        row_points() points, y[i] = sum of row r's point i - r * hop over the rows that reach i (the synthesis step of an
        STFT).  A gather without atomics: the terms are added in ascending r from +0, so the result is deterministic and
        bit-equal to the row loop y[r * hop : r * hop + F] += m[r] in the matrix's dtype.  hop > row_points() leaves zero
        gaps, hop == row_points() flattens the matrix.  Number space, domain and delta are the matrix's, which stays as it
        is.  Codes: 0 (a matrix without rows gives an empty vector); 7 if hop is 0 (no vector); -1 for a poisoned matrix
        (the vector is poisoned too).  Allocates, so it cannot be captured into a Graph."""
        out = C.c_void_p()
        code = _lib.check(self._fn("overlap_add")(self._h, int(hop), C.byref(out)), "mat_overlap_add" + self._sfx)
        return code, (DspVec(_handle=out.value, _sfx=self._sfx) if out.value else None)

    # ------------------------------------------------------------------ across the rows
    # One tiled transpose of whole elements (a complex pair stays together) serves all three; one launch each, no host
    # round trip, no pointer table, no synchronisation.
    def transpose(self):
        """Rows become columns in place: rows() <- the old row_points(), row_points() <- the old rows(), element (r, j)
        moves to (j, r); bit-exact.  After it every row operation (fft, windowed_fft, statistics, convolve, diff, ...)
        works down the old columns.  Number space, domain and delta stay -- delta belongs to the row axis, so its meaning
        after a transpose is the caller's.  A matrix without rows or with empty rows becomes a matrix without rows
        (transposing an empty matrix twice does not bring the row count back).  Codes: 0; -1 for a poisoned matrix, which
        is left as it is.  Goes through the trade buffer like swap_halves and does not allocate, so it can be captured
        into a Graph."""
        return self._call("transpose")

    @classmethod
    def from_interleaved(cls, vector, channels):
        """(code, DspMat-or-None): the DspVec `vector` of interleaved channels as a matrix of `channels` rows x
        points // channels points -- row c, point j is x[j * channels + c] (in points), every row bit-equal to target c of
        DspVec.split_into with `channels` targets.  Number space, domain and delta are the vector's, which stays as it
        is.  An empty vector gives `channels` empty rows.  Codes: 0; 7 if channels is 0 or does not divide the points (no
        matrix); -1 for a poisoned vector (the matrix is poisoned too).  Allocates, so it cannot be captured into a
        Graph."""
        out = C.c_void_p()
        fn = getattr(lib, "bdsp_hip_mat_from_interleaved" + vector._sfx)
        code = _lib.check(fn(vector._h, int(channels), C.byref(out)), "mat_from_interleaved" + vector._sfx)
        return code, (cls(_handle=out.value, _sfx=vector._sfx) if out.value else None)

    def to_interleaved(self):
        """(code, DspVec-or-None): the rows interleaved into one vector of rows() * row_points() points, y[j * rows + r] =
        row r's point j -- bit-equal to DspVec.merge of the rows, and the inverse of from_interleaved.  Number space,
        domain and delta are the matrix's, which stays as it is.  Codes: 0 (a matrix without rows gives an empty vector);
        -1 for a poisoned matrix (the vector is poisoned too).  Allocates, so it cannot be captured into a Graph."""
        out = C.c_void_p()
        code = _lib.check(self._fn("to_interleaved")(self._h, C.byref(out)), "mat_to_interleaved" + self._sfx)
        return code, (DspVec(_handle=out.value, _sfx=self._sfx) if out.value else None)

    def zero_interleave(self, factor):
        """Every point of every row is followed by factor - 1 zeros, as DspVec.zero_interleave on every row; row_points()
        grows by `factor`, rows, delta and domain stay.  Codes: 0 (a factor <= 1 leaves the matrix as it is); -1 for a
        matrix that was poisoned before.  Grows the buffers on the first call at a size, so only a repeated call can be
        captured into a Graph."""
        return self._call("zero_interleave", int(factor))

    # ------------------------------------------------------------------ elementwise
    def scale(self, factor):
        if isinstance(factor, complex):
            return self._call("complex_scale", factor.real, factor.imag)
        return self._call("real_scale", factor)

    def offset(self, value):
        return self._call("real_offset", value)

    def conj(self):
        return self._call("conj")

    def _binary(self, name, other):
        if isinstance(other, DspVec):
            return self._call(name + "_vector", other._h)
        return self._call(name, other._h)

    def add(self, other):
        return self._binary("add", other)

    def sub(self, other):
        return self._binary("sub", other)

    def mul(self, other):
        return self._binary("mul", other)

    def div(self, other):
        return self._binary("div", other)

    def magnitude(self):
        return self._call("magnitude")

    def magnitude_squared(self):
        return self._call("magnitude_squared")

    def to_real(self):
        return self._call("to_real")

    def to_imag(self):
        return self._call("to_imag")

    def phase(self):
        return self._call("phase")

    # ------------------------------------------------------------------ differences, running sums, phase wrapping
    # Every row as the DspVec method of the same name on that row; one batched launch (cum_sum: three for rows of
    # more than 4096 points) whatever the number of rows.
    def diff(self):
        """Every row loses its first point: row[j] = row[j + 1] - row[j]."""
        return self._call("diff")

    def diff_with_start(self):
        """As diff, but every row keeps its first point."""
        return self._call("diff_with_start")

    def cum_sum(self):
        """Running sum of every row (carried in double, rounded once per element, as DspVec.cum_sum)."""
        return self._call("cum_sum")

    def wrap(self, divisor):
        """fmod(x, divisor) of every element; a complex matrix is poisoned (-1)."""
        return self._call("wrap", divisor)

    def unwrap(self, divisor):
        """Undoes wrap along every row (divisor 2 pi for a phase); a complex matrix is poisoned (-1)."""
        return self._call("unwrap", divisor)

    # ------------------------------------------------------------------ math family, reverse, mixer, *_smaller, parts
    # Every row as the DspVec method of the same name on that row, bit for bit; one launch each, whatever the number of
    # rows, and no synchronisation.
    def _math0(name, real_only):  # noqa: N805 -- method factory
        def method(self):
            return self._call(name)
        method.__name__ = name
        method.__doc__ = "`%s` of every element in place, as DspVec.%s on every row.  Codes: 0; -1 for a %smatrix that " \
            "was poisoned before; no rows or empty rows: 0." % (name, name, "complex matrix (poisoned) or a " if real_only else "")
        return method

    def _math1(name, real_only):  # noqa: N805
        def method(self, value):
            return self._call(name, value)
        method.__name__ = name
        method.__doc__ = "`%s(value)` of every element in place, as DspVec.%s on every row.  Codes: 0; -1 for a %smatrix " \
            "that was poisoned before; no rows or empty rows: 0." % (name, name, "complex matrix (poisoned) or a " if real_only else "")
        return method

    for _n in ("sqrt", "square", "ln", "exp", "sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh",
               "asinh", "acosh", "atanh"):
        locals()[_n] = _math0(_n, False)
    for _n in ("abs", "ln_approx", "exp_approx", "sin_approx", "cos_approx"):
        locals()[_n] = _math0(_n, True)
    for _n in ("powf", "root", "log", "expf"):
        locals()[_n] = _math1(_n, False)
    for _n in ("log_approx", "expf_approx", "powf_approx"):
        locals()[_n] = _math1(_n, True)
    del _n, _math0, _math1

    def reverse(self):
        """Every row back to front: row[i] <- row[points - 1 - i], bit-exact; the order of the rows, delta and domain
        stay.  Codes: 0; -1 for a matrix that was poisoned before; no rows or empty rows: 0."""
        return self._call("reverse")

    def multiply_complex_exponential(self, a, b):
        """z[r][k] *= exp(j (a * delta * k + b * delta)) with k counted from 0 in every row: mixes every row by the same
        frequency.  The phasor of a position is computed once and reused down the rows.  Codes: 0; -1 for a real matrix
        (poisoned) or one that was poisoned before; no rows or empty rows: 0."""
        return self._call("multiply_complex_exponential", a, b)

    def add_smaller(self, other):
        """row[i] += operand[i mod len(operand)]: row r wraps around row r of a DspMat, or every row around one DspVec.
        Codes: 0; 7 if the row counts differ, the operand('s rows) are empty or their length does not divide the ROW
        length; 2 if number space, domain or delta disagree; -1 for a matrix that was poisoned before.  The matrix is
        untouched after an error."""
        return self._binary("add_smaller", other)

    def sub_smaller(self, other):
        """row[i] -= operand[i mod len(operand)].  Codes: as add_smaller (0, 7, 2, -1)."""
        return self._binary("sub_smaller", other)

    def mul_smaller(self, other):
        """row[i] *= operand[i mod len(operand)].  Codes: as add_smaller (0, 7, 2, -1)."""
        return self._binary("mul_smaller", other)

    def div_smaller(self, other):
        """row[i] /= operand[i mod len(operand)].  Codes: as add_smaller (0, 7, 2, -1)."""
        return self._binary("div_smaller", other)

    def get_real(self, destination):
        """The real parts into the DspMat `destination`, which becomes rows x points real scalars and keeps its delta;
        self stays as it is.  A real self or a complex destination leaves `destination` with rows() empty rows.  Codes: 0;
        -1 if self is poisoned (destination untouched)."""
        return self._call("get_real", destination._h)

    def get_imag(self, destination):
        """The imaginary parts into `destination`.  Codes and shapes: as get_real (0, -1)."""
        return self._call("get_imag", destination._h)

    def get_magnitude(self, destination):
        """|z| of every point into `destination`.  Codes and shapes: as get_real (0, -1)."""
        return self._call("get_magnitude", destination._h)

    def get_magnitude_squared(self, destination):
        """re^2 + im^2 of every point into `destination`.  Codes and shapes: as get_real (0, -1)."""
        return self._call("get_magnitude_squared", destination._h)

    def get_phase(self, destination):
        """atan2(im, re) of every point into `destination`.  Codes and shapes: as get_real (0, -1)."""
        return self._call("get_phase", destination._h)

    def get_real_imag(self, real, imag):
        """Real and imaginary parts into two DspMat in one pass.  Codes and shapes: as get_real (0, -1)."""
        return self._call("get_real_imag", real._h, imag._h)

    def get_mag_phase(self, mag, phase):
        """Magnitude and phase into two DspMat in one pass.  Codes and shapes: as get_real (0, -1)."""
        return self._call("get_mag_phase", mag._h, phase._h)

    def set_real_imag(self, real, imag):
        """self becomes complex with the shape of `real`: z = real + j imag.  Codes: 0; 7 unless both arguments have the
        same row count and row length; -1 for a matrix that was poisoned before."""
        return self._call("set_real_imag", real._h, imag._h)

    def set_mag_phase(self, mag, phase):
        """self becomes complex with the shape of `mag`: z = mag * exp(j phase).  Codes: as set_real_imag (0, 7, -1)."""
        return self._call("set_mag_phase", mag._h, phase._h)

    # ------------------------------------------------------------------ transforms, windows, index moves
    def plain_fft(self):
        return self._call("plain_fft")

    def fft(self):
        return self._call("fft")

    def windowed_fft(self, window):
        return self._call("windowed_fft", int(window))

    def plain_ifft(self):
        return self._call("plain_ifft")

    def ifft(self):
        return self._call("ifft")

    def windowed_ifft(self, window):
        return self._call("windowed_ifft", int(window))

    def apply_window(self, window):
        return self._call("apply_window", int(window))

    def unapply_window(self, window):
        return self._call("unapply_window", int(window))

    # the four index moves below are one launch over rows x row points each, every row as the DspVec method on it
    def swap_halves(self):
        return self._call("swap_halves")

    def fft_shift(self):
        return self._call("fft_shift")

    def ifft_shift(self):
        return self._call("ifft_shift")

    def zero_pad(self, points, option=PAD_END):
        return self._call("zero_pad", int(points), int(option))

    # ------------------------------------------------------------------ symmetric transforms of real rows
    # Every row as the DspVec method of the same name on that row.  N = real points of a row, p = N // 2 + 1.  The
    # forward forms are the batched transform plus one crop, the inverse forms one mirror launch, one 4-byte read-back
    # (the only synchronisation) and the batched inverse transform -- whatever the number of rows.
    def plain_sfft(self):
        """Real time rows of odd N -> the p non-redundant bins of plain_fft per row, densely packed (complex,
        frequency domain, delta <- N * delta).  Codes: 5 (not real / time; poisoned), 9 (N even or 0; poisoned)."""
        return self._call("plain_sfft")

    def sfft(self):
        """As plain_sfft from the shifted spectrum fft() leaves: its first p bins, the negative half plus DC."""
        return self._call("sfft")

    def windowed_sfft(self, window):
        """As sfft after `window` (WINDOW_*) on every row; the window is fused into the transform."""
        return self._call("windowed_sfft", int(window))

    def plain_sifft(self):
        """Half spectra of p bins per row -> real time rows of 2p - 1 points, unnormalised (delta <- (2p - 1) * delta).
        Codes: 6 (not complex / frequency; poisoned), 8 (the first bin of some row is not real; the whole matrix is
        poisoned)."""
        return self._call("plain_sifft")

    def sifft(self):
        """As plain_sifft after scaling by 1 / p and ifft_shift of every half spectrum (DspVec.sifft per row)."""
        return self._call("sifft")

    def windowed_sifft(self, window):
        """As sifft, then every row divided by `window`."""
        return self._call("windowed_sifft", int(window))

    def mirror(self):
        """Every row grows from p to 2p - 1 complex points: the conjugate-symmetric full spectrum of a half spectrum
        (bit-exact).  A real time-domain matrix is poisoned (-1)."""
        return self._call("mirror")

    def to_complex(self):
        """Every real scalar x becomes (x, 0); a complex matrix is poisoned (-1)."""
        return self._call("to_complex")

    # ------------------------------------------------------------------ convolution / interpolation
    def convolve_signal(self, impulse_response):
        """One DspVec shared by all rows, or a rows x rows nested list of DspVec (MIMO:
        out[n] = sum_r row[r] (*) h[n][r], matrix/src/time_freq.rs:439-483)."""
        if isinstance(impulse_response, DspVec):
            return self._call("convolve_signal", impulse_response._h)
        flat = [h for row in impulse_response for h in row]
        arr = (C.c_void_p * len(flat))(*[h._h for h in flat])
        return self._call("convolve_signal_mat", arr, len(flat))

    def prepare_argument(self):
        """Every row becomes the argument `correlate` takes: plain_fft, conjugated (CrossCorrelationArgumentOps)."""
        return self._call("prepare_argument")

    def prepare_argument_padded(self):
        """As prepare_argument after Surround-padding every row to 2 * points - 1; 7 for rows of one point or less."""
        return self._call("prepare_argument_padded")

    def correlate(self, other):
        """Cross-correlates row r with row r of a prepared DspMat, or every row with one prepared DspVec
        (matrix/src/time_freq.rs:241-264).  Rows grow to the argument's points.  Codes: 5 (self not complex / time or
        `other` not prepared; self is poisoned), 7 (argument not longer than the rows, or unequal row counts)."""
        return self._binary("correlate", other)

    def interpolatef(self, function, interpolation_factor, delay, conv_len, rolloff=0.0):
        """Every row resampled by `interpolation_factor` with wrap-around inside the row, as DspVec.interpolatef on that
        row: rows become interpolatef_new_len points long, delta stays.  `delay` is one number for all rows, or a
        one-dimensional sequence / array with one value per row (converted to the matrix's dtype): row r then equals
        DspVec.interpolatef on row r with delay[r], bit for bit.  One launch for all rows (one more for the tap tables
        of an integer factor), whatever their number.  Codes: 0; a delay sequence that does not have one value per row
        leaves the matrix untouched and the code is 7.  -1 for a matrix that was poisoned before.  A matrix with no
        rows or empty rows is left as it is (0).  (tests/test_gpu_mat_interpf.py holds the argument error.)"""
        if np.ndim(delay) == 0:
            return self._call("interpolatef", int(function), rolloff, interpolation_factor, delay, int(conv_len))
        d = np.ascontiguousarray(delay, dtype=np.float32 if self._sfx == "32" else np.float64)
        if d.ndim != 1:
            raise ValueError("delay: a number or a one-dimensional sequence with one value per row")
        ptr = d.ctypes.data_as(C.POINTER(C.c_float if self._sfx == "32" else C.c_double))
        return self._call("interpolatef_delays", int(function), rolloff, interpolation_factor, ptr, d.size, int(conv_len))

    def multiply_frequency_response(self, function, ratio, rolloff=0.0):
        return self._call("multiply_frequency_response", int(function), rolloff, ratio)

    # ------------------------------------------------------------------ time-domain smoothing, real-row resampling
    # Every row as the DspVec method of the same name on that row.  One launch for the weight table (none for a
    # callable) and one for all rows while the 2 * conv_len + 1 weights are few or wrap around the row, else the batched
    # block convolution; one launch for an interpolation -- whatever the number of rows.
    def convolve(self, function, ratio, conv_len, rolloff=0.0):
        """Circular convolution of every row with an impulse response sampled at 2 * conv_len + 1 points `ratio`
        apart (conv_len is clipped to the row's points): `function` is CONV_SINC, CONV_RAISED_COSINE with `rolloff`, or a
        Python callable f(x) the host samples once for all rows.  Delta and domain stay.  Codes: 0; -1 for a
        frequency-domain matrix (poisoned) or one that was poisoned before; a matrix with no rows or empty rows is left
        as it is (0)."""
        if callable(function):
            cb = (_lib.REAL_FN32 if self._sfx == "32" else _lib.REAL_FN64)(lambda _data, x: function(x))
            return self._call("convolve_real", cb, None, True, ratio, int(conv_len))
        return self._call("convolve", int(function), rolloff, ratio, int(conv_len))

    def convolve_complex(self, function, ratio, conv_len):
        """As convolve with a complex-valued Python callable f(x), complex rows only.  Codes: 0; -1 for a real or a
        frequency-domain matrix (poisoned) or one that was poisoned before."""
        def cb(_ctx, x, out):
            r = complex(function(x))
            out[0], out[1] = r.real, r.imag
        bridge = getattr(_lib, "ComplexBridge" + self._sfx)(getattr(_lib, "COMPLEX_PTR_FN" + self._sfx)(cb), None)
        fn = C.cast(getattr(lib, "bdsp_hip_complex_fn_bridge" + self._sfx), C.c_void_p)
        return self._call("convolve_complex", fn, C.addressof(bridge), True, ratio, int(conv_len))

    def interpolate_lin(self, interpolation_factor, delay=0.0):
        """Every real row of n scalars resampled to round((n - 1) * interpolation_factor) + 1 scalars by linear
        interpolation between its samples, shifted by `delay` samples; bit-equal to DspVec.interpolate_lin on the row.
        Delta and domain stay.  Codes: 0; -1 for a complex matrix (poisoned) or one that was poisoned before; no rows or
        empty rows: 0."""
        return self._call("interpolate_lin", interpolation_factor, delay)

    def interpolate_hermite(self, interpolation_factor, delay=0.0):
        """As interpolate_lin with piecewise cubic Hermite (Catmull-Rom) interpolation, the end points extrapolated
        linearly; bit-equal to DspVec.interpolate_hermite on the row.  Codes: 0; -1 for a complex matrix
        (poisoned) or one that was poisoned before; no rows or empty rows: 0."""
        return self._call("interpolate_hermite", interpolation_factor, delay)

    # ------------------------------------------------------------------ FFT-domain resampling, decimation
    # Every row as the DspVec method of the same name on that row; real rows stay real.  One launch when the new row
    # length is an integer multiple of the old one and a power of two of at most 4096 points, else a batched forward
    # transform, one spectrum pass and a batched inverse transform -- whatever the number of rows.
    def interpolatei(self, function, interpolation_factor, rolloff=0.0):
        """Every row grows to points * interpolation_factor: zero interleave, then `function` (CONV_SINC or
        CONV_RAISED_COSINE with `rolloff`) as a low pass in the frequency domain.  delta stays.  A factor <= 1 leaves the
        matrix as it is (0)."""
        return self._call("interpolatei", int(function), rolloff, int(interpolation_factor))

    def interpolate(self, function, dest_points, delay=0.0, rolloff=0.0):
        """Every row resampled to dest_points (more or fewer than before) through its spectrum, shifted by `delay` (in
        units of delta); function=None is interpft.  delta <- delta / (dest_points / points).  7 for dest_points == 0
        or rows without points."""
        if function is None:
            return self._call("interpft", int(dest_points))
        return self._call("interpolate", int(function), rolloff, int(dest_points), delay)

    def interpft(self, dest_points):
        """Every row resampled to dest_points by padding or cropping its spectrum (no response, no delay)."""
        return self._call("interpft", int(dest_points))

    def decimatei(self, decimation_factor, delay):
        """Every row keeps the points delay, delay + decimation_factor, ...; 7 for a factor of 0.  delta stays."""
        return self._call("decimatei", int(decimation_factor), int(delay))

    # ------------------------------------------------------------------ per-row statistics, sums, dot products
    # One batched device pass each (matrix/src/general/statistics.rs, mod.rs); results per row as numpy columns.
    _STAT_KEYS = ("sum", "count", "average", "rms", "min", "min_index", "max", "max_index")

    def _out_dtypes(self, prec):
        """(result struct, scalar dtype, complex dtype) of this matrix's precision, or double with prec"""
        if prec or self._sfx == "64":
            st = _lib.ComplexStatistics64 if self.is_complex() else _lib.Statistics64
            return st, np.float64, np.complex128
        st = _lib.ComplexStatistics32 if self.is_complex() else _lib.Statistics32
        return st, np.float32, np.complex64

    def _stats(self, split, length, prec):
        cplx = self.is_complex()
        st, _, cdt = self._out_dtypes(prec)
        n = self.rows() * (length if split else 1)
        arr = np.zeros(n, dtype=np.dtype(st))  # the #[repr(C)] layout, filled by one copy
        name = ("complex" if cplx else "real") + "_statistics" + ("_split" if split else "") + ("_prec" if prec else "")
        args = (arr.ctypes.data_as(C.POINTER(st)), n) + ((int(length),) if split else ())
        code = self._call(name, *args)
        cols = {}
        for k in self._STAT_KEYS:
            col = arr[k]
            if k in ("count", "min_index", "max_index"):
                cols[k] = col.astype(np.int64)
            elif cplx:
                z = np.empty(n, dtype=cdt)
                z.real, z.imag = col["re"], col["im"]
                cols[k] = z
            else:
                cols[k] = col.copy()
        return code, cols

    def statistics(self, prec=False):
        """StatisticsOps / PreciseStatisticsOps per row: dict of arrays of length rows (keys of DspVec.statistics)."""
        return self._stats(False, 1, prec)[1]

    def statistics_split(self, length, prec=False):
        """(code, dict of arrays shaped [rows, length]); element j of a row goes to bucket j % length."""
        code, cols = self._stats(True, length, prec)
        if code not in (0, -1):
            return code, {}
        return code, {k: v.reshape(self.rows(), int(length)) for k, v in cols.items()}

    def _value_out(self, prec):
        """one (complex) value per row: the array and the pointer the C ABI takes"""
        _, rdt, cdt = self._out_dtypes(prec)
        out = np.zeros(self.rows(), dtype=cdt if self.is_complex() else rdt)
        ct = {np.float32: C.c_float, np.float64: C.c_double, np.complex64: _lib.Complex32,
              np.complex128: _lib.Complex64}[out.dtype.type]
        return out, out.ctypes.data_as(C.POINTER(ct))

    def _sums(self, which, prec):
        cplx = self.is_complex()
        out, ptr = self._value_out(prec)
        name = ("complex" if cplx else "real") + which + ("_prec" if prec else "")
        self._call(name, ptr, out.size)
        return out

    def sum(self, prec=False):
        return self._sums("_sum", prec)

    def sum_sq(self, prec=False):
        return self._sums("_sum_sq", prec)

    def dot_product(self, other, prec=False):
        """(code, array of one value per row): row r with row r of a DspMat, or every row with one DspVec.
        Codes as DspVec.dot_product (4 / 3 / 2), 7 for unequal row counts, -1 poisoned."""
        cplx = self.is_complex()
        out, ptr = self._value_out(prec)
        name = ("complex" if cplx else "real") + "_dot_product" + ("_vector" if isinstance(other, DspVec) else "") + \
            ("_prec" if prec else "")
        code = self._call(name, other._h, ptr, out.size)
        return code, out
