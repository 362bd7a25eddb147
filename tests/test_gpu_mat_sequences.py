"""DspMat under the state it carries from call to call.  Every other matrix test builds a fresh matrix, calls one method
and compares; here the matrix has a history first.

  * Part 2, test_mover_sequences_*: generated sequences of 16 "movers" (tests/mat_model.py: the operations that only
    rearrange scalars).  After EVERY step the return codes, rows / row_len / row_points / is_complex / domain, delta and
    the data -- bit for bit, as unsigned integers, so -0.0, NaN and Inf count -- equal the numpy model's.
  * Part 3, test_results_owe_nothing_to_history: every other public method (CATALOGUE) on "dirty" matrices (shrunk,
    transposed, filling their allocation exactly, regrown, number space changed twice, made from a vector, empty) and on a
    fresh copy of the same values: the same kernel on the same values with the same launch geometry, so code, metadata
    and bits are equal -- no tolerance.  No kernel under these methods accumulates with atomics (the only atomic is the
    atomicOr of plain_sifft's flag), so no entry needs one.  The fresh result is also held to the CPU oracle once per
    entry, with the tolerance of the method's own test, quoted next to each check.  Argument errors leave a dirty matrix
    as it was; poisoning calls poison it as documented.
  * Part 4, test_more_than_65535_rows_*: the base operations on 70000 rows of 3, 16, 17 and 30 points -- the state
    transpose leaves behind a wide, short matrix.
  * Part 5, test_plans_* / test_interpolatef_tap_table_*: the process-wide caches under the methods.

tests/test_mat_model.py checks on the CPU that the model agrees with the oracle, what the sequences cover, and that
every public DspMat method is a mover, an accessor or in CATALOGUE."""
import os
import re

import numpy as np
import pytest

import mat_model as mm
import oracle_lib as orc
from mat_model import FREQ, PAD_SURROUND, TIME

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.float32, np.float64)
HAMMING = 1
SINC, RAISED_COSINE = 0, 1
DELTA = 0.5
# read at every step of part 2 (device_ptr is an address: it differs between two matrices by design)
ACCESSORS = ("rows", "row_len", "row_points", "is_complex", "domain", "delta", "data", "device_ptr")


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


# ---------------------------------------------------------------------------------------------- helpers
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])


def _same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if not np.array_equal(_bits(got), _bits(ref)):
        bad = np.argwhere(_bits(got).reshape(got.shape[0] if got.ndim > 1 else 1, -1) !=
                          _bits(ref).reshape(got.shape[0] if got.ndim > 1 else 1, -1))
        raise AssertionError((what, "first differing (row, scalar)", bad[:4].tolist(), "of", len(bad)))


def _meta(o):
    if hasattr(o, "rows"):
        return ("matrix", o.rows(), o.row_len(), o.row_points(), bool(o.is_complex()), o.domain())
    return ("vector", len(o), o.points(), bool(o.is_complex()), o.domain())


def _same_delta(a, b, what):
    assert a == b or (np.isnan(a) and np.isnan(b)), (what, "delta", a, b)


def _same_state(got, want, what):
    """metadata, delta (exactly) and data (bit for bit) of two matrices or two vectors, from either side"""
    assert _meta(got) == _meta(want), (what, _meta(got), _meta(want))
    _same_delta(got.delta(), want.delta(), what)
    _same_bits(got.data(), want.data(), what)


def _mat(bd, x, cplx, domain=TIME, delta=1.0):
    x = np.ascontiguousarray(x)
    if x.size == 0:
        return bd.DspMat(rows=x.shape[0], row_len=x.shape[1] if x.shape[0] else 0, is_complex=cplx, dtype=x.dtype,
                         domain=domain, delta=delta)
    return bd.DspMat(x, is_complex=cplx, domain=domain, delta=delta)


class _Api:
    """the GPU side of mat_model.apply_step / build_dirty"""

    def __init__(self, bd):
        self.bd, self.Mat = bd, bd.DspMat

    def mat(self, a, is_complex, domain, delta):
        return _mat(self.bd, a, is_complex, domain, delta)


def _fill(rows, scalars, seed, dtype, lo=-10, hi=10):
    return orc.fill_uniform(rows * scalars, seed, lo, hi, dtype).reshape(rows, scalars)


def _as_real(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return np.ascontiguousarray(a.astype(np.complex128)).view(np.float64)
    return a.astype(np.float64)


def rel_l2(got, ref):
    got, ref = _as_real(got).ravel(), _as_real(ref).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def _rows_close(got, ref, tol, what):
    """rel-L2 < tol for EVERY row on its own (one wrong row must fail); NaN where the reference has NaN"""
    got, ref = _as_real(got), _as_real(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    g, f = np.where(nan, 0.0, got), np.where(nan, 0.0, ref)
    err = np.linalg.norm(g - f, axis=1) / np.maximum(np.linalg.norm(f, axis=1), 1e-300)
    if err.size:
        print("%s: worst row rel-L2 %.3e (bound %.1e)" % (what, err.max(), tol))
        assert err.max() < tol, (what, "row", int(err.argmax()), float(err.max()), tol)


def _per_row(fn, x):
    out = [fn(r) for r in x]
    return np.stack(out) if out else np.zeros((0, 0), x.dtype)


def _to_complex64(x, cplx):
    """rows as float64 interleaved complex (a real row is zero-interleaved first)"""
    xd = x.astype(np.float64)
    if cplx:
        return xd
    out = np.zeros((x.shape[0], 2 * x.shape[1]))
    out[:, 0::2] = xd
    return out


def _z(x64):
    return np.ascontiguousarray(x64).view(np.complex128)


def _hamming(n, cplx=True):
    """the oracle's Hamming window of n points, float64"""
    with np.errstate(all="ignore"):
        w = orc.apply_window(np.ones(2 * n if cplx else n), cplx, 1, 0.54)
    return w[0::2] if cplx else w


# ============================================================================================== part 2: mover sequences
_SEQ = {}


def _sequence(rows, pts, cplx, seed):
    key = (rows, pts, cplx, seed)
    if key not in _SEQ:
        _SEQ[key] = mm.gen_sequence(*key)[0]
    return _SEQ[key]


def _start_data(rows, pts, cplx, dtype, seed):
    """uniform noise with a few -0.0, a NaN and an Inf planted (as many of them as the size holds): movers must carry
    them unchanged"""
    e = 2 if cplx else 1
    x = _fill(rows, pts * e, 7000 + seed, dtype)
    f, n = x.reshape(-1), x.size
    for k, v in ((0, -0.0), (n // 2, np.nan), (n - 1, np.inf), (n // 3, -0.0), (2 * n // 3, -0.0), (n // 5, -np.inf)):
        if k < n and (k == 0 or n >= 8):
            f[k] = v
    if n == 2:
        f[1] = np.nan
    return x


SEQ_CASES = [(r, p, c, d, dom) for (r, p) in mm.START_SHAPES for c in (False, True) for d in DTYPES for dom in (TIME, FREQ)]


@pytest.mark.parametrize("rows,pts,cplx,dtype,domain", SEQ_CASES,
                         ids=["%dx%d-%s-%s-%s" % (r, p, "complex" if c else "real", np.dtype(d).name, "freq" if dom else "time")
                              for (r, p, c, d, dom) in SEQ_CASES])
def test_mover_sequences_equal_the_model_at_every_step(bd, rows, pts, cplx, dtype, domain):
    """24 sequences of 16 movers from this start state; nothing is skipped.  The step assertion below names the seed, the
    step index and the step: a transpose that forgot `rows`, or a zero_pad that skipped the buffer trade, fails here at
    that step (metadata in the first case, data bits in the second)."""
    api = _Api(bd)
    for seed in mm.SEEDS:
        x = _start_data(rows, pts, cplx, dtype, seed)
        g, w = api.mat(x, cplx, domain, 0.25), mm.MatModel(x, cplx, domain, 0.25)
        _same_state(g, w, (seed, "start"))
        for i, step in enumerate(_sequence(rows, pts, cplx, seed)):
            what = ("seed", seed, "step", i, step)
            g_codes, g, g_side = mm.apply_step(api, g, step)
            w_codes, w, w_side = mm.apply_step(mm.ModelApi, w, step)
            assert g_codes == w_codes, (what, "codes", g_codes, w_codes)
            _same_state(g, w, what)
            assert len(g_side) == len(w_side)
            for k, (a, b) in enumerate(zip(g_side, w_side)):   # sources stay as they were, destinations and vectors are right
                _same_state(a, b, (what, "side object", k))


# ============================================================================================== part 3: the catalogue
class Ctx:
    """what a catalogue entry's call and check see: the state's description and the operands"""

    def __init__(self, bd, dtype, cplx, domain, rows, points, seed, dirty):
        self.bd, self.dtype, self.cplx, self.domain, self.rows, self.points = bd, dtype, cplx, domain, rows, points
        self.e = 2 if cplx else 1
        self.seed, self.dirty, self.arrays, self.sel = seed, dirty, {}, None

    def sub(self, a):
        """the rows of an operand matrix that belong to the rows being checked"""
        return a if self.sel is None else a[self.sel]

    def mat(self, k, lo=-10, hi=10, cplx=None):
        """operand matrix k of the state's shape.  Dirty: uploaded transposed and transposed back on the device (traded
        buffers, `rows` rewritten); fresh: uploaded as it is.  Equal values either way."""
        cplx = self.cplx if cplx is None else cplx
        e = 2 if cplx else 1
        base = _fill(self.rows, self.points * e, self.seed + 101 * k, self.dtype, lo, hi)
        self.arrays[("mat", k)] = base
        if self.dirty and base.size:
            t = np.ascontiguousarray(base.reshape(self.rows, self.points, e).transpose(1, 0, 2)).reshape(self.points, self.rows * e)
            m = _mat(self.bd, t, cplx, self.domain, DELTA)
            assert m.transpose() == 0
            return m
        return _mat(self.bd, base, cplx, self.domain, DELTA)

    def vec(self, k, points=None, lo=-10, hi=10, scale=1.0, cplx=None, domain=None):
        """operand vector k of `points` points (default: a row's).  Dirty: uploaded zero-interleaved and decimated on
        the device (shrunk, traded); fresh: uploaded as it is."""
        cplx = self.cplx if cplx is None else cplx
        domain = self.domain if domain is None else domain
        points = self.points if points is None else points
        e = 2 if cplx else 1
        base = (orc.fill_uniform(points * e, self.seed + 211 * k, lo, hi, self.dtype) * self.dtype(scale)).astype(self.dtype)
        self.arrays[("vec", k)] = base
        if self.dirty and base.size:
            wide = np.zeros((points, 2, e), self.dtype)
            wide[:, 0, :] = base.reshape(points, e)
            v = self.bd.DspVec(wide.reshape(-1), is_complex=cplx, domain=domain, delta=DELTA)
            assert v.decimatei(2, 0) == 0 and v.points() == points
            return v
        return self.bd.DspVec(base, is_complex=cplx, domain=domain, delta=DELTA)

    def small(self, k):
        """a destination of another shape and delta than anything a getter produces"""
        return self.bd.DspMat(rows=2, row_len=4, is_complex=False, dtype=self.dtype, delta=0.125)


class Entry:
    def __init__(self, method, call, check=None, label=None, space=None, domain=TIME, rng=(-10, 10), pre=None, prep=None):
        """call(m, ctx) -> code or (code, extras): extras are matrices, vectors, arrays or dicts of arrays the call
        produced.  check(ctx, x, got, extras): the oracle assertions on rows x -> got.  space: "real" / "complex" / None
        (both).  pre(rows, points): the method's precondition on the shape.  prep(m): movers that bring the dirty matrix
        into the method's domain of definition before the fresh copy is taken."""
        self.method, self.call, self.check, self.label = method, call, check, label or method
        self.space, self.domain, self.rng, self.pre, self.prep = space, domain, rng, pre, prep


def _tol(dtype, f32, f64):
    return f32 if dtype == np.float32 else f64


# ---- elementwise -----------------------------------------------------------------------------------------------------
def _chk_bits(fn):
    def check(c, x, got, extras):
        _same_bits(got, _per_row(lambda r: fn(c, r), x).reshape(got.shape), "oracle, bit-exact")
    return check


def e_scale():
    # test_flat_elementwise_ops_equal_the_oracle_bit_for_bit: bit-equal
    return [Entry("scale", lambda m, c: m.scale(2.5), _chk_bits(lambda c, r: orc.real_scale(r, 2.5))),
            Entry("scale", lambda m, c: m.scale(complex(0.5, -1.5)), _chk_bits(lambda c, r: orc.complex_scale(r, 0.5, -1.5)),
                  label="scale(complex)", space="complex"),
            Entry("offset", lambda m, c: m.offset(-1.25), _chk_bits(lambda c, r: orc.real_offset(r, -1.25, c.cplx)))]


def e_binary(name, op, kind, smaller=False):
    method = name + ("_smaller" if smaller else "")

    def call(m, c):   # operands from (1, 10): div stays tame (test_smaller_with_a_matrix_and_with_a_vector_operand)
        return getattr(m, method)(c.mat(1, 1, 10) if kind == "matrix" else c.vec(1, None, 1, 10))

    def check(c, x, got, extras):
        if kind == "matrix":
            ref = np.stack([orc.binary(p, q, c.cplx, op)[1] for p, q in zip(x, c.sub(c.arrays[("mat", 1)]))])
        else:
            ref = np.stack([orc.binary(p, c.arrays[("vec", 1)], c.cplx, op)[1] for p in x])
        if name == "div" and c.cplx and not smaller:   # test_flat_elementwise_ops...: complex division within 4 eps
            np.testing.assert_allclose(got, ref, rtol=4 * np.finfo(c.dtype).eps)
        else:                                          # everything else bit-equal
            _same_bits(got, ref, method)
    return Entry(method, call, check, label="%s(%s)" % (method, kind))


def e_complex_to_real(name, kind, getter=False):
    def call(m, c):
        if not getter:
            return getattr(m, name)()
        dst = c.small(0)
        return getattr(m, name)(dst), [dst]

    def check(c, x, got, extras):
        if getter:
            got = extras[0].data()
        ref = _per_row(lambda r: orc.complex_to_real(r, kind), x)
        if kind == 1:   # test_complex_to_real_maps: magnitude_squared bit-equal, magnitude and phase 4 eps rel and abs
            _same_bits(got, ref, name)
        else:
            eps = np.finfo(c.dtype).eps
            np.testing.assert_allclose(got, ref, rtol=4 * eps, atol=4 * eps)
    return Entry(name, call, check, space="complex")


# ---- differences, running sums, phase wrapping ----------------------------------------------------------------------
def _chk_cum_sum(c, x, got, extras):
    # test_cum_sum_rows: max |got - prefix| / (max |prefix| + 1) < 2e-7 (f32) / 1e-13 (f64) per row
    if not x.size:
        return
    g = got.astype(np.float64).reshape(x.shape[0], -1, c.e)
    ref = np.cumsum(x.astype(np.float64).reshape(x.shape[0], -1, c.e), axis=1)
    err = np.max(np.abs(g - ref), axis=(1, 2)) / (np.max(np.abs(ref), axis=(1, 2)) + 1.0)
    assert err.max() < _tol(c.dtype, 2e-7, 1e-13), err.max()


def e_scan():
    return [Entry("diff", lambda m, c: m.diff(), _chk_bits(lambda c, r: orc.diff(r, c.cplx))),   # test_diff_rows...: bit-equal
            Entry("diff_with_start", lambda m, c: m.diff_with_start(), _chk_bits(lambda c, r: orc.diff(r, c.cplx, True))),
            Entry("cum_sum", lambda m, c: m.cum_sum(), _chk_cum_sum),
            # test_wrap_equals_the_oracle_on_the_flat_data, test_unwrap_rows_equal_the_oracle_bit_for_bit: bit-equal
            Entry("wrap", lambda m, c: m.wrap(c.dtype(7.0)), _chk_bits(lambda c, r: orc.math(r, False, "wrap", c.dtype(7.0))),
                  space="real", rng=(-100, 100)),
            Entry("unwrap", lambda m, c: m.unwrap(c.dtype(7.0)), _chk_bits(lambda c, r: orc.unwrap(r, c.dtype(7.0))),
                  space="real", rng=(-30, 30))]


# ---- math family (test_gpu_mat_ew.py / test_gpu_parity.py: ranges that keep the functions real-valued) ---------------
_MATH_DOMAINS = {
    "sqrt": (0.0, 50.0), "square": (-10, 10), "ln": (1e-3, 50.0), "exp": (-10, 10), "sin": (-10, 10), "cos": (-10, 10),
    "tan": (-1.4, 1.4), "asin": (-0.99, 0.99), "acos": (-0.99, 0.99), "atan": (-10, 10), "sinh": (-8, 8),
    "cosh": (-8, 8), "tanh": (-8, 8), "asinh": (-10, 10), "acosh": (1.01, 50.0), "atanh": (-0.99, 0.99),
    "abs": (-10, 10), "ln_approx": (1e-3, 50.0), "exp_approx": (-10, 10), "sin_approx": (-10, 10),
    "cos_approx": (-10, 10)}
_MATH_ARGS = {"powf": ((0.1, 10.0), 2.5), "root": ((0.1, 10.0), 3.0), "log": ((1e-3, 50.0), 10.0),
              "expf": ((-3, 3), 10.0), "log_approx": ((1e-3, 50.0), 10.0),
              "expf_approx": ((-3, 3), 10.0), "powf_approx": ((0.1, 10.0), 2.5)}
_COMPLEX_MATH0 = ("sqrt", "square", "ln", "exp", "sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh",
                  "asinh", "acosh", "atanh")
_COMPLEX_MATH1 = (("powf", 2.5), ("root", 3.0), ("log", 10.0), ("expf", 7.0))


def _oracle_math(x, cplx, name, arg):
    key = {"ln_approx": "ln", "exp_approx": "exp", "sin_approx": "sin", "cos_approx": "cos", "log_approx": "log"}.get(name, name)
    if name == "root":
        key, arg = "powf", 1.0 / arg
    return orc.math(x.astype(np.float64), cplx, key, arg)


def e_math(name, arg, cplx):
    args = () if arg is None else (arg,)

    def check(c, x, got, extras):
        ref = _oracle_math(x.reshape(-1), cplx, name, arg or 0.0).reshape(x.shape)
        if cplx:   # test_math_family_...: complex rel-L2 < 2e-5 / 1e-12
            assert rel_l2(got, ref) < _tol(c.dtype, 2e-5, 1e-12), name
        else:      # real: max |got - ref| / (|ref| + 1) < 3e-6 / 1e-13, four times that with an argument
            tol = _tol(c.dtype, 3e-6, 1e-13) * (4 if args else 1)
            assert float(np.max(np.abs(got - ref) / (np.abs(ref) + 1.0))) < tol, name
    rng = (-3, 3) if cplx else (_MATH_ARGS[name][0] if args else _MATH_DOMAINS[name])
    return Entry(name, lambda m, c: getattr(m, name)(*args), check, label="%s(%s)" % (name, "complex" if cplx else "real"),
                 space="complex" if cplx else "real", rng=rng)


def _chk_cexp(a, b):
    def check(c, x, got, extras):
        # test_multiply_complex_exponential: rel-L2 < 2e-7 / 1e-14 per row against the exact float64 phase; a and b are
        # multiplied by delta in T first, the phase restarts in every row
        ad, bdl = float(c.dtype(a) * c.dtype(DELTA)), float(c.dtype(b) * c.dtype(DELTA))
        k = np.arange(x.shape[1] // 2)
        ref = _z(x.astype(np.float64)) * np.exp(1j * (ad * k + bdl))[None, :]
        _rows_close(got, ref, _tol(c.dtype, 2e-7, 1e-14), "multiply_complex_exponential")
    return check


# ---- pairs -----------------------------------------------------------------------------------------------------------
def _call_get_mag_phase(m, c):
    mag, ph = c.small(0), c.small(1)
    return m.get_mag_phase(mag, ph), [mag, ph]


def _chk_get_mag_phase(c, x, got, extras):
    # test_pairs_split_merge_map: magnitudes rel-L2 < tol = 2e-6 / 1e-14, phases within 4 * tol absolute, per row
    tol = _tol(c.dtype, 2e-6, 1e-14)
    gm, gp = extras[0].data(), extras[1].data()
    for r in range(x.shape[0]):
        mag, ph = orc.get_mag_phase(x[r])
        assert rel_l2(gm[r], mag) < tol and np.max(np.abs(gp[r] - ph)) < 4 * tol, r


def _call_set_mag_phase(m, c):
    return m.set_mag_phase(c.mat(1, 0, 10, cplx=False), c.mat(2, -3, 3, cplx=False))


def _chk_set_mag_phase(c, x, got, extras):
    # test_pairs_split_merge_map: rel-L2 < 4 * tol, tol = 2e-6 / 1e-14, per row
    mag, ph = c.sub(c.arrays[("mat", 1)]), c.sub(c.arrays[("mat", 2)])
    _rows_close(got, np.stack([orc.set_mag_phase(a, b) for a, b in zip(mag, ph)]), 4 * _tol(c.dtype, 2e-6, 1e-14), "set_mag_phase")


# ---- transforms (test_gpu_mat_basic.py, test_transforms_of_every_row: numpy's FFT in float64, rel-L2 per row
# < 1e-6 (f32) / 1e-12 (f64)) ------------------------------------------------------------------------------------------
def _fft_ref(xc64, name):
    """all rows at once: xc64 [rows, 2n] float64 interleaved -> the transform `name` along axis 1"""
    z = _z(xc64)
    n = z.shape[1]
    with np.errstate(all="ignore"):
        if name == "plain_fft":
            return np.fft.fft(z, axis=1)
        if name == "fft":
            return np.roll(np.fft.fft(z, axis=1), n // 2, axis=1)
        if name == "windowed_fft":
            return np.roll(np.fft.fft(z * _hamming(n)[None, :], axis=1), n // 2, axis=1)
        if name == "plain_ifft":
            return np.fft.ifft(z, axis=1) * n
        out = np.fft.ifft(np.roll(z, -(n // 2), axis=1), axis=1)   # ifft = scale(1 / n) -> ifft_shift -> plain_ifft
        return out / _hamming(n)[None, :] if name == "windowed_ifft" else out


def e_fft(name):
    args = (HAMMING,) if "windowed" in name else ()

    def check(c, x, got, extras):
        if x.size:
            _rows_close(got, _fft_ref(_to_complex64(x, c.cplx), name), _tol(c.dtype, 1e-6, 1e-12), name)
    return Entry(name, lambda m, c: getattr(m, name)(*args), check, domain=FREQ if "ifft" in name else TIME)


def _ulp_of_10(dtype):
    return float(np.spacing(np.asarray(10.0, dtype=dtype)))


def _chk_window(unapply):
    def check(c, x, got, extras):
        # test_windows_on_every_row: Hamming within 4 ulp of 10 absolute; unapply within 4 * 4 ulp / 1e-2 where the
        # window exceeds 1e-2 (Hamming does everywhere from two points on)
        if not x.size:
            return
        with np.errstate(all="ignore"):
            ref = np.stack([orc.apply_window(r, c.cplx, 1, 0.54, unapply=unapply) for r in x])
        atol = 4 * _ulp_of_10(c.dtype) * (4 / 1e-2 if unapply else 1)
        np.testing.assert_allclose(got.astype(np.float64), ref.astype(np.float64), rtol=0, atol=atol)
    return check


MFR_RATIO, MFR_ROLLOFF = 1.7, 0.35


def _chk_mfr(fid):
    def check(c, x, got, extras):
        # test_multiply_frequency_response_on_every_row: f64 within 1e-12 absolute; f32 within 4 ulp of the row's max |ref|
        ref = _per_row(lambda r: orc.multiply_frequency_response(r, c.cplx, fid, MFR_ROLLOFF, MFR_RATIO, False), x)
        if c.dtype == np.float64:
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
            return
        for r in range(x.shape[0]):
            top = np.max(np.abs(ref[r].astype(np.float64)))
            ulp = float(np.spacing(np.asarray(top if top > 0 else 1.0, dtype=ref.dtype)))
            assert float(np.max(np.abs(got[r].astype(np.float64) - ref[r].astype(np.float64)))) / ulp <= 4.0, r
    return check


# ---- symmetric transforms (test_gpu_mat_sym.py: tol = 1e-6 / 1e-12; forward forms < 2 tol against the oracle,
# plain_sifft and sifft < 2 tol, windowed_sifft < 4 tol) ---------------------------------------------------------------
def _odd(rows, points):
    return points % 2 == 1


def e_sfft(name):
    args = (HAMMING,) if "windowed" in name else ()

    def check(c, x, got, extras):
        n = x.shape[1]
        p = n // 2 + 1
        xd = x.astype(np.float64)
        if name == "plain_sfft":
            ref = np.fft.fft(xd, axis=1)[:, :p]
        else:
            w = _hamming(n) if args else 1.0
            ref = np.roll(np.fft.fft(xd * w, axis=1), n // 2, axis=1)[:, :p]
        _rows_close(got, ref, 2 * _tol(c.dtype, 1e-6, 1e-12), name)
    return Entry(name, lambda m, c: getattr(m, name)(*args), check, space="real", pre=_odd)


def _real_spectrum(m):
    """imaginary parts <- 0 by two movers: every half spectrum then passes the first-bin rule, shifted or not"""
    assert m.to_real() == 0 and m.to_complex() == 0


def e_sifft(name):
    args = (HAMMING,) if "windowed" in name else ()

    def check(c, x, got, extras):
        h = _z(x.astype(np.float64))
        p = h.shape[1]
        n = 2 * p - 1
        if name != "plain_sifft":   # scale(1 / p) and ifft_shift of the HALF spectrum come first
            h = np.roll(h / p, -(p // 2), axis=1)
        full = np.concatenate([h, np.conj(h[:, :0:-1])], axis=1)
        ref = np.real(np.fft.ifft(full, axis=1) * n)
        if args:
            ref = ref / _hamming(n, False)[None, :]
        _rows_close(got, ref, (4 if args else 2) * _tol(c.dtype, 1e-6, 1e-12), name)
    return Entry(name, lambda m, c: getattr(m, name)(*args), check, space="complex", domain=FREQ, prep=_real_spectrum,
                 pre=lambda rows, points: points >= 1)


# ---- convolution, correlation ---------------------------------------------------------------------------------------
def e_convolve_signal(taps):
    def check(c, x, got, extras):
        # test_convolve_signal_with_a_shared_filter: rel-L2 < 1e-6 / 1e-12 per row against the direct form in float64
        h = c.arrays[("vec", 1)].astype(np.float64)
        ref = _per_row(lambda r: orc.convolve_direct(r.astype(np.float64), h, c.cplx), x)
        _rows_close(got, ref, _tol(c.dtype, 1e-6, 1e-12), "convolve_signal")
    return Entry("convolve_signal", lambda m, c: m.convolve_signal(c.vec(1, taps, -1, 1, 1.0 / taps)), check,
                 label="convolve_signal(%d taps)" % taps, pre=lambda rows, points: points >= taps)


def _call_mimo(m, c):
    return m.convolve_signal([[c.vec(10 + c.rows * n + r, 17, -1, 1, 1.0 / 17) for r in range(c.rows)] for n in range(c.rows)])


def _chk_mimo(c, x, got, extras):
    # test_convolve_signal_mimo: rel-L2 < 1e-6 / 1e-12 per row; out[n] = sum_r row[r] (*) h[n][r] (all rows needed)
    h = lambda n, r: c.arrays[("vec", 10 + c.rows * n + r)].astype(np.float64)
    ref = np.stack([sum(orc.convolve_direct(x[r].astype(np.float64), h(n, r), c.cplx) for r in range(c.rows)) for n in range(c.rows)])
    _rows_close(got, ref, _tol(c.dtype, 1e-6, 1e-12), "convolve_signal(mimo)")


def e_prepare_argument(padded):
    name = "prepare_argument_padded" if padded else "prepare_argument"

    def check(c, x, got, extras):
        # test_gpu_mat_correlate.py, tol_for: rel-L2 < 2e-6 / 1e-12 per row
        ref = _per_row(lambda r: orc.prepare_argument(r, padded)[1], _to_complex64(x, c.cplx))
        _rows_close(got, ref, _tol(c.dtype, 2e-6, 1e-12), name)
    return Entry(name, lambda m, c: getattr(m, name)(), check, pre=lambda rows, points: points >= 2)


def e_correlate(kind, arg_points=None):
    """arg_points: the argument's length l (None: 2 p - 1 through prepare_argument_padded)"""
    def call(m, c):
        arg = c.mat(1) if kind == "matrix" else c.vec(1)
        if arg_points is None:
            assert arg.prepare_argument_padded() == 0
        else:
            assert arg.zero_pad(arg_points, PAD_SURROUND) == 0 and arg.prepare_argument() == 0
        return m.correlate(arg)

    def check(c, x, got, extras):
        # test_gpu_mat_correlate.py, test_against_the_oracle: rel-L2 < 2e-6 / 1e-12 per row, the argument from the oracle
        p = x.shape[1] // 2
        for r in range(x.shape[0]):
            y = (c.sub(c.arrays[("mat", 1)])[r] if kind == "matrix" else c.arrays[("vec", 1)]).astype(np.float64)
            if arg_points is None:
                code, ref_arg = orc.prepare_argument(y, True)
            else:
                code, padded = orc.zero_pad(y, True, arg_points, PAD_SURROUND, buffered=True)
                assert code == 0
                code, ref_arg = orc.prepare_argument(padded, False)
            assert code == 0
            code, ref = orc.correlate(x[r].astype(np.float64), ref_arg)
            assert code == 0
            err = rel_l2(got[r], ref)
            assert err < _tol(c.dtype, 2e-6, 1e-12), ("correlate", kind, arg_points, r, err)
    return Entry("correlate", call, check, label="correlate(%s%s)" % (kind, "" if arg_points is None else ", %d" % arg_points),
                 space="complex", pre=lambda rows, points: points >= 2 and (arg_points is None or arg_points > points))


def e_interpolatef(fid, rolloff, factor, conv_len):
    def check(c, x, got, extras):
        # test_interpolatef_of_every_row: rel-L2 < 2e-6 / 1e-12 per row; integer factor against the float64 oracle,
        # fractional factor against the oracle in T with exact weights
        if factor == int(factor):
            ref = _per_row(lambda r: orc.interpolatef(r.astype(np.float64), c.cplx, fid, rolloff, factor, 0.0, conv_len)[0], x)
        else:
            with orc.exact_weights():
                ref = _per_row(lambda r: orc.interpolatef(r, c.cplx, fid, rolloff, c.dtype(factor), 0.0, conv_len)[0], x)
        _rows_close(got, ref, _tol(c.dtype, 2e-6, 1e-12), "interpolatef")
    return Entry("interpolatef", lambda m, c: m.interpolatef(fid, factor, 0.0, conv_len, rolloff), check,
                 label="interpolatef(%d, %g)" % (fid, factor), pre=lambda rows, points: rows <= 100)   # one launch per row


def e_convolve(fid, rolloff, ratio, conv_len, how="builtin"):
    def call(m, c):
        if how == "callable":
            return m.convolve(lambda t: float(np.sinc(t)), ratio, conv_len)
        if how == "complex":
            return m.convolve_complex(lambda t: np.sinc(t) * (1 + 0.5j), ratio, conv_len)
        return m.convolve(fid, ratio, conv_len, rolloff=rolloff)

    def check(c, x, got, extras):
        # test_gpu_mat_interp.py: rel-L2 < 2e-6 / 1e-12 per row against the float64 oracle (at most 2 * 300 + 1 weights)
        ref = _per_row(lambda r: orc.convolve_function(r.astype(np.float64), c.cplx, fid, rolloff, ratio, conv_len), x)
        if how == "complex":
            ref = np.ascontiguousarray(_z(ref) * (1 + 0.5j)).view(np.float64)
        _rows_close(got, ref, _tol(c.dtype, 2e-6, 1e-12), "convolve")
    method = "convolve_complex" if how == "complex" else "convolve"
    return Entry(method, call, check, label="%s(%s, %d, L=%d)" % (method, how, fid, conv_len),
                 space="complex" if how == "complex" else None)


def e_interpolate_real(name, factor, delay):
    # test_interpolations_are_bit_equal: bit-equal to the oracle in the matrix's precision
    return Entry(name, lambda m, c: getattr(m, name)(factor, delay),
                 _chk_bits(lambda c, r: getattr(orc, name)(r, factor, delay)), space="real")


def e_resample(op):
    """op as in test_gpu_mat_resample.py: ("interpolatei", fid, rolloff, factor) | ("interpolate", fid, rolloff, extra
    points, delay) | ("interpft", extra points); tolerances from there: interpolatei rel-L2 < 5e-6 / 1e-11, interpolate
    and interpft < 2e-5 / 1e-10, per row against the float64 oracle"""
    def dest(points):
        return points + op[3 if op[0] == "interpolate" else 1]

    def call(m, c):
        if op[0] == "interpolatei":
            return m.interpolatei(op[1], op[3], op[2])
        if op[0] == "interpolate":
            return m.interpolate(op[1], dest(m.row_points()), op[4], op[2])
        return m.interpft(dest(m.row_points()))

    def check(c, x, got, extras):
        points = x.shape[1] // c.e

        def ref_row(r):
            r = r.astype(np.float64)
            if op[0] == "interpolatei":
                code, ref = orc.interpolatei(r, c.cplx, op[1], op[2], op[3])
            elif op[0] == "interpolate":
                code, ref, _ = orc.interpolate(r, c.cplx, op[1], op[2], dest(points), op[4], DELTA)
            else:
                code, ref, _ = orc.interpolate(r, c.cplx, -1, 0.0, dest(points), 0.0, DELTA)
            assert code == 0
            return ref
        tol = _tol(c.dtype, 5e-6, 1e-11) if op[0] == "interpolatei" else _tol(c.dtype, 2e-5, 1e-10)
        _rows_close(got, _per_row(ref_row, x), tol, op[0])
    return Entry(op[0], call, check, label="%s%s" % (op[0], op[1:]), pre=lambda rows, points: points >= 1)


# ---- reductions (test_gpu_mat_reductions.py, test_rows_against_the_oracle: tol = 2e-5 / 1e-12; sums, averages, rms and
# dot products within 50 * tol * max(1, |ref|), counts, extremes and their indices equal) ------------------------------
def _chk_stats(split):
    def check(c, x, got, extras):
        st = extras[0]
        tol = 50 * _tol(c.dtype, 2e-5, 1e-12)
        fn = orc.complex_statistics if c.cplx else orc.real_statistics
        for r in range(x.shape[0]):
            x64 = x[r].astype(np.float64)
            for b in range(split or 1):
                ref = fn(x64, b, split) if split else fn(x64)
                val = (lambda k: st[k][r, b]) if split else (lambda k: st[k][r])
                for key in ("count", "min_index", "max_index"):
                    assert val(key) == ref[key], (r, b, key)
                if not split:
                    assert val("min") == ref["min"] and val("max") == ref["max"], r
                for key in ("sum", "average", "rms"):
                    assert abs(val(key) - ref[key]) <= tol * max(1.0, abs(ref[key])), (r, b, key)
    return check


def _chk_sum(squared):
    def check(c, x, got, extras):
        tol = 50 * _tol(c.dtype, 2e-5, 1e-12)
        for r in range(x.shape[0]):
            ref = orc.vec_sum(x[r].astype(np.float64), c.cplx, squared)
            assert abs(extras[0][r] - ref) <= tol * max(1.0, abs(ref)), r
    return check


def e_dot(kind, prec):
    def call(m, c):
        code, d = m.dot_product(c.mat(1, -1, 1) if kind == "matrix" else c.vec(1, None, -1, 1), prec=prec)
        return code, [d]

    def check(c, x, got, extras):
        tol = 50 * _tol(c.dtype, 2e-5, 1e-12)
        for r in range(x.shape[0]):
            y = c.sub(c.arrays[("mat", 1)])[r] if kind == "matrix" else c.arrays[("vec", 1)]
            ref = orc.dot(x[r].astype(np.float64), y.astype(np.float64), c.cplx)
            assert abs(extras[0][r] - ref) <= tol * max(1.0, abs(ref)), r
    return Entry("dot_product", call, check, label="dot_product(%s%s)" % (kind, ", prec" if prec else ""))


def _stat_calls():
    out = []
    for prec in (False, True):
        tag = "(prec)" if prec else ""
        out.append(Entry("statistics", lambda m, c, prec=prec: (0, [m.statistics(prec=prec)]), _chk_stats(0), label="statistics" + tag))
        out.append(Entry("statistics_split", lambda m, c, prec=prec: (lambda r: (r[0], [r[1]]))(m.statistics_split(3, prec=prec)),
                         _chk_stats(3), label="statistics_split" + tag, pre=lambda rows, points: points >= 3))
        out.append(Entry("sum", lambda m, c, prec=prec: (0, [m.sum(prec=prec)]), _chk_sum(False), label="sum" + tag))
        out.append(Entry("sum_sq", lambda m, c, prec=prec: (0, [m.sum_sq(prec=prec)]), _chk_sum(True), label="sum_sq" + tag))
        out += [e_dot("matrix", prec), e_dot("vector", prec)]
    return out


def _catalogue():
    cat = e_scale()
    for op, name in enumerate(("add", "sub", "mul", "div")):
        cat += [e_binary(name, op, "matrix"), e_binary(name, op, "vector")]
    for op, name in enumerate(("add", "sub", "mul", "div")):
        cat += [e_binary(name, op, "matrix", True), e_binary(name, op, "vector", True)]
    cat += [e_complex_to_real("magnitude", 0), e_complex_to_real("magnitude_squared", 1), e_complex_to_real("phase", 4)]
    cat += e_scan()
    cat += [e_math(n, None, False) for n in _MATH_DOMAINS] + [e_math(n, a, False) for n, (_, a) in _MATH_ARGS.items()]
    cat += [e_math(n, None, True) for n in _COMPLEX_MATH0] + [e_math(n, a, True) for n, a in _COMPLEX_MATH1]
    cat.append(Entry("multiply_complex_exponential", lambda m, c: m.multiply_complex_exponential(0.02, 0.3), _chk_cexp(0.02, 0.3),
                     space="complex"))
    cat += [e_complex_to_real("get_magnitude", 0, True), e_complex_to_real("get_magnitude_squared", 1, True),
            e_complex_to_real("get_phase", 4, True),
            Entry("get_mag_phase", _call_get_mag_phase, _chk_get_mag_phase, space="complex"),
            Entry("set_mag_phase", _call_set_mag_phase, _chk_set_mag_phase)]
    cat += [e_fft(n) for n in ("plain_fft", "fft", "windowed_fft", "plain_ifft", "ifft", "windowed_ifft")]
    cat += [Entry("apply_window", lambda m, c: m.apply_window(HAMMING), _chk_window(False)),
            Entry("unapply_window", lambda m, c: m.unapply_window(HAMMING), _chk_window(True), pre=lambda rows, points: points != 1)]
    cat += [Entry("multiply_frequency_response", lambda m, c, fid=fid: m.multiply_frequency_response(fid, MFR_RATIO, MFR_ROLLOFF),
                  _chk_mfr(fid), label="multiply_frequency_response(%d)" % fid, domain=FREQ, rng=(-1, 1)) for fid in (SINC, RAISED_COSINE)]
    cat += [e_sfft(n) for n in ("plain_sfft", "sfft", "windowed_sfft")] + [e_sifft(n) for n in ("plain_sifft", "sifft", "windowed_sifft")]
    cat += [e_convolve_signal(33), e_convolve_signal(3),
            Entry("convolve_signal", _call_mimo, _chk_mimo, label="convolve_signal(mimo)",
                  pre=lambda rows, points: 1 <= rows <= 5 and points >= 17)]
    cat += [e_prepare_argument(False), e_prepare_argument(True), e_correlate("matrix"), e_correlate("vector")]
    cat += [e_interpolatef(SINC, 0.0, 2.0, 8), e_interpolatef(RAISED_COSINE, 0.35, 1.5, 10)]
    cat += [e_convolve(SINC, 0.0, 0.25, 12), e_convolve(RAISED_COSINE, 0.35, 0.25, 12), e_convolve(SINC, 0.0, 0.25, 64),
            e_convolve(SINC, 0.0, 0.25, 12, "callable"), e_convolve(SINC, 0.0, 0.25, 12, "complex")]
    cat += [e_interpolate_real("interpolate_lin", 2.5, 0.0), e_interpolate_real("interpolate_hermite", 2.5, 0.25)]
    cat += [e_resample(("interpolatei", SINC, 0.0, 2)), e_resample(("interpolatei", RAISED_COSINE, 0.35, 3)),
            e_resample(("interpolate", SINC, 0.0, 37, 0.0)), e_resample(("interpolate", RAISED_COSINE, 0.35, 12, 0.25)),
            e_resample(("interpft", 37))]
    cat += _stat_calls()
    return cat


CATALOGUE = _catalogue()
assert len({e.label for e in CATALOGUE}) == len(CATALOGUE)

# (state, is_complex) of every dirty state
DIRTY_STATES = [(name, c) for name, d in mm.DIRTY.items() for c in ((False, True) if d["is_complex"] is None else (d["is_complex"],))]


def _build_states(bd, name, cplx, dtype, domain, rng, seed):
    """the dirty matrix on the GPU and the same recipe in the model: the dirty content is known exactly"""
    api = _Api(bd)
    fill = lambda rows, scalars: _fill(rows, scalars, seed, dtype, *rng)
    d = mm.build_dirty(api, name, fill, dtype, cplx, domain, DELTA, vec=lambda a: bd.DspVec(a, is_complex=True, domain=domain, delta=DELTA))
    w = mm.build_dirty(mm.ModelApi, name, fill, dtype, cplx, domain, DELTA, vec=lambda a: mm.VecModel(a, True, domain, DELTA))
    _same_state(d, w, (name, "the recipe's result"))
    return d, w


def _run_entry(entry, m, ctx):
    res = entry.call(m, ctx)
    return (res, []) if isinstance(res, (int, np.integer)) else (res[0], list(res[1]))


def _same_extras(a, b, what):
    assert len(a) == len(b), what
    for k, (p, q) in enumerate(zip(a, b)):
        if isinstance(p, dict):
            assert p.keys() == q.keys(), what
            for key in p:
                _same_bits(p[key], q[key], (what, "result", k, key))
        elif isinstance(p, np.ndarray):
            _same_bits(p, q, (what, "result", k))
        else:
            _same_state(p, q, (what, "result", k))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("entry", CATALOGUE, ids=[e.label for e in CATALOGUE])
def test_results_owe_nothing_to_history(bd, entry, dtype):
    """the method on every dirty state it is defined on, and on a fresh matrix of the same values and metadata: equal
    code, metadata and bits (for reductions: bit-equal result arrays).  The comparison names the dirty state: a
    transpose that forgot `rows` or a zero_pad that skipped the trade makes D2 / D3 / D4 differ from their fresh copies
    here (and fails _build_states' comparison with the model before that).  Then the fresh result against the oracle,
    once, on the first state with data."""
    ran, checked = 0, False
    for k, (name, cplx) in enumerate(DIRTY_STATES):
        if entry.space is not None and (entry.space == "complex") != cplx:
            continue
        seed = 3000 + 17 * k
        d, w = _build_states(bd, name, cplx, dtype, entry.domain, entry.rng, seed)
        if entry.pre is not None and not entry.pre(w.rows(), w.row_points()):
            continue
        if entry.prep is not None:
            entry.prep(d)
        x = d.data()
        f = _mat(bd, x, d.is_complex(), d.domain(), d.delta())
        _same_state(f, d, (name, "fresh copy"))
        what = (entry.label, name, "complex" if cplx else "real")
        ctxs = [Ctx(bd, dtype, d.is_complex(), entry.domain, d.rows(), d.row_points(), seed, dirty) for dirty in (True, False)]
        code_d, extra_d = _run_entry(entry, d, ctxs[0])
        code_f, extra_f = _run_entry(entry, f, ctxs[1])
        assert code_d == code_f, (what, "codes", code_d, code_f)
        _same_state(d, f, what)
        _same_extras(extra_d, extra_f, what)
        ran += 1
        if not checked and x.size and entry.check is not None:
            assert code_f == 0, (what, code_f)
            with np.errstate(all="ignore"):
                entry.check(ctxs[1], x, f.data(), extra_f)
            checked = True
    assert ran >= 2 and checked, (entry.label, ran, checked)


# ---- argument errors on dirty matrices ------------------------------------------------------------------------------
def _fewer_rows(c, k, cplx=None):
    """operand matrix k without its last row"""
    cplx = c.cplx if cplx is None else cplx
    return _mat(c.bd, c.arrays_of(k, cplx)[:-1], cplx, c.domain, DELTA)


def _prepared(arg, points):
    assert arg.zero_pad(points, PAD_SURROUND) == 0 and arg.prepare_argument() == 0
    return arg


def _dot_other_space(m, other):
    """dot_product through the C entry point of the OTHER number space: DspMat.dot_product picks the entry point by
    is_complex(), so the codes 4 (must be real) and 3 (must be complex) its docstring names exist at this level only"""
    import ctypes as C
    name = ("real" if m.is_complex() else "complex") + "_dot_product" + ("_vector" if hasattr(other, "points") else "")
    fn = m._fn(name)
    out = np.zeros(2 * max(m.rows(), 1), m.dtype)
    return fn(m._h, other._h, C.cast(out.ctypes.data_as(C.c_void_p), fn.argtypes[2]), m.rows())


def _arg_errors():
    """(method, label, space, bad call -> code, the documented code (or cplx -> code), a following good call): every
    method whose docstring names an argument-error code (tests/test_mat_model.py checks that none is missing), and the
    undocumented ones the other matrix tests pin (zero_pad, set_row, add .. div, convolve_signal, interpft)"""
    good = lambda m, c: m.scale(2.0)
    t = [
        ("zero_pad", "to the current length", None, lambda m, c: m.zero_pad(m.row_points()), 7, lambda m, c: m.zero_pad(m.row_points() + 3)),
        ("decimatei", "by 0", None, lambda m, c: m.decimatei(0, 0), 7, lambda m, c: m.decimatei(3, 1)),
        ("set_row", "past the end", None, lambda m, c: m.set_row(m.rows(), c.vec(1)), 7, lambda m, c: m.set_row(1, c.vec(1))),
        ("set_row", "of another length", None, lambda m, c: m.set_row(0, c.vec(1, c.points - 1)), 7, good),
        ("set_real_imag", "unequal parts", None, lambda m, c: m.set_real_imag(c.mat(1, cplx=False), _fewer_rows(c, 2, False)), 7, good),
        ("set_mag_phase", "unequal parts", None, lambda m, c: m.set_mag_phase(c.mat(1, 0, 10, cplx=False), _fewer_rows(c, 2, False)), 7, good),
        ("convolve_signal", "filter longer than a row", None, lambda m, c: m.convolve_signal(c.vec(1, c.points + 1)), 7,
         lambda m, c: m.convolve_signal(c.vec(1, 33, -1, 1, 1 / 33))),
        ("convolve_signal", "other number space", None, lambda m, c: m.convolve_signal(c.vec(1, 6, cplx=not c.cplx)), 2, good),
        ("correlate", "argument not longer than the rows", "complex", lambda m, c: m.correlate(c.prepared(1)), 7,
         lambda m, c: m.plain_fft()),
        ("correlate", "unequal row counts", "complex", lambda m, c: m.correlate(_prepared(_fewer_rows(c, 1), 2 * c.points)), 7,
         lambda m, c: m.correlate(_prepared(c.mat(1), 2 * c.points))),
        ("interpolate", "to 0 points", None, lambda m, c: m.interpolate(SINC, 0), 7, lambda m, c: m.interpolate(SINC, m.row_points() + 5)),
        ("interpft", "to 0 points", None, lambda m, c: m.interpft(0), 7, lambda m, c: m.interpft(m.row_points() + 5)),
        ("overlap_add", "hop 0", None, lambda m, c: m.overlap_add(0)[0], 7, good),
        ("dot_product", "other row count", None, lambda m, c: m.dot_product(_fewer_rows(c, 1))[0], 7,
         lambda m, c: m.dot_product(c.mat(1))[0]),
        ("dot_product", "complex rows, real operand", "complex", lambda m, c: m.dot_product(c.vec(1, cplx=False))[0], 2, good),
        ("dot_product", "complex rows, operand of the other domain", "complex", lambda m, c: m.dot_product(c.vec(1, domain=FREQ))[0], 2, good),
        ("dot_product", "entry point of the other number space, matrix", None, lambda m, c: _dot_other_space(m, c.mat(1)),
         lambda cplx: 4 if cplx else 3, good),
        ("dot_product", "entry point of the other number space, vector", None, lambda m, c: _dot_other_space(m, c.vec(1)),
         lambda cplx: 4 if cplx else 3, good),
    ]
    for name in ("add", "sub", "mul", "div"):   # test_gpu_mat_basic.py::test_codes: 7 row counts, 1 lengths, 2 metadata
        t += [(name, "matrix of another row count", None, lambda m, c, name=name: getattr(m, name)(_fewer_rows(c, 1)), 7,
               lambda m, c, name=name: getattr(m, name)(c.mat(1, 1, 10))),
              (name, "vector of another length", None, lambda m, c, name=name: getattr(m, name)(c.vec(1, c.points - 1)), 1,
               lambda m, c, name=name: getattr(m, name)(c.vec(1, None, 1, 10))),
              (name, "vector of the other domain", None, lambda m, c, name=name: getattr(m, name)(c.vec(1, domain=FREQ)), 2, good)]
        sm = name + "_smaller"
        t += [(sm, "vector whose length does not divide", None, lambda m, c, sm=sm: getattr(m, sm)(c.vec(1, c.points - 1)), 7,
               lambda m, c, sm=sm: getattr(m, sm)(c.vec(1, None, 1, 10))),
              (sm, "matrix of another row count", None, lambda m, c, sm=sm: getattr(m, sm)(_fewer_rows(c, 1)), 7,
               lambda m, c, sm=sm: getattr(m, sm)(c.mat(1, 1, 10))),
              (sm, "vector of the other domain", None, lambda m, c, sm=sm: getattr(m, sm)(c.vec(1, domain=FREQ)), 2, good)]
    return t


class _ErrCtx(Ctx):
    def arrays_of(self, k, cplx=None):
        self.mat(k, cplx=cplx)
        return self.arrays[("mat", k)]

    def prepared(self, k):
        v = self.vec(k)   # as long as the rows: not longer
        assert v.prepare_argument() == 0
        return v


ARG_ERRORS = _arg_errors()
# methods whose docstring names an argument-error code, and why they are not in ARG_ERRORS
ARG_ERRORS_EXEMPT = {
    "from_frames": "a constructor from a vector: there is no matrix to leave as it was (test_gpu_mat_frame.py has the codes)",
    "from_vectors": "a constructor from vectors: as from_frames",
    "from_interleaved": "a constructor from a vector: as from_frames (test_gpu_mat_transpose.py has the codes)",
    "prepare_argument_padded": "its 7 is about rows of one point or less, a state no recipe of D1-D4 reaches, not about an argument",
}
ERR_STATES = [(n, c) for (n, c) in DIRTY_STATES if n[:2] in ("D1", "D2", "D3", "D4")]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_argument_errors_leave_a_dirty_matrix_as_it_was(bd, dtype):
    for k, (name, cplx) in enumerate(ERR_STATES):
        for j, (method, label, space, bad, code, good) in enumerate(ARG_ERRORS):
            if space is not None and (space == "complex") != cplx:
                continue
            seed = 5000 + 31 * k + j
            d, w = _build_states(bd, name, cplx, dtype, TIME, (-10, 10), seed)
            what = (method, label, name, "complex" if cplx else "real")
            ctx = _ErrCtx(bd, dtype, cplx, TIME, d.rows(), d.row_points(), seed, True)
            assert bad(d, ctx) == (code(cplx) if callable(code) else code), what
            _same_state(d, w, (what, "after the refused call"))   # bits, metadata and delta as the model left them
            f = _mat(bd, w.data(), cplx, TIME, DELTA)
            fctx = _ErrCtx(bd, dtype, cplx, TIME, d.rows(), d.row_points(), seed, False)
            cd, cf = good(d, ctx), good(f, fctx)
            assert cd == cf == 0, (what, "the good call", cd, cf)
            _same_state(d, f, (what, "after the good call"))


# ---- poisoning calls on a dirty matrix ------------------------------------------------------------------------------
EVEN = "D2-transposed-even"   # 5 x 1000: the symmetric transforms' code 9 needs an even N


def _poisoners():
    """(method, label, is_complex, domain, call, documented code, dirty state): every way the docstrings of matrix.py
    name to poison a matrix (tests/test_mat_model.py checks that no such method is missing), and the undocumented ones the
    other matrix tests pin (conj, complex scale, the complex -> real maps, multiply_frequency_response, the transforms)"""
    D2 = "D2-transposed"
    p = [("conj", "real rows", False, TIME, lambda m, c: m.conj(), -1, D2),
         ("scale", "complex factor, real rows", False, TIME, lambda m, c: m.scale(complex(1, 2)), -1, D2),
         ("to_complex", "complex rows", True, TIME, lambda m, c: m.to_complex(), -1, D2),
         ("mirror", "real time rows", False, TIME, lambda m, c: m.mirror(), -1, D2),
         ("wrap", "complex rows", True, TIME, lambda m, c: m.wrap(7.0), -1, D2),
         ("unwrap", "complex rows", True, TIME, lambda m, c: m.unwrap(7.0), -1, D2),
         ("multiply_complex_exponential", "real rows", False, TIME, lambda m, c: m.multiply_complex_exponential(0.02, 0.3), -1, D2),
         ("multiply_frequency_response", "time domain", True, TIME, lambda m, c: m.multiply_frequency_response(SINC, 0.5), -1, D2),
         ("plain_sifft", "first bin not real", True, FREQ, lambda m, c: m.plain_sifft(), 8, D2),
         ("sifft", "first bin not real", True, FREQ, lambda m, c: m.sifft(), 8, D2),
         ("windowed_sifft", "first bin not real", True, FREQ, lambda m, c: m.windowed_sifft(HAMMING), 8, D2),
         ("correlate", "real rows", False, TIME, lambda m, c: m.correlate(c.vec(1, cplx=True, domain=FREQ)), 5, D2),
         ("correlate", "unprepared argument", True, TIME, lambda m, c: m.correlate(c.vec(1)), 5, D2),
         ("convolve", "frequency domain", True, FREQ, lambda m, c: m.convolve(SINC, 0.25, 12), -1, D2),
         ("convolve_complex", "real rows", False, TIME, lambda m, c: m.convolve_complex(lambda t: 1j, 0.25, 3), -1, D2),
         ("convolve_complex", "frequency domain", True, FREQ, lambda m, c: m.convolve_complex(lambda t: 1j, 0.25, 3), -1, D2),
         ("interpolate_lin", "complex rows", True, TIME, lambda m, c: m.interpolate_lin(2.0), -1, D2),
         ("interpolate_hermite", "complex rows", True, TIME, lambda m, c: m.interpolate_hermite(2.0), -1, D2)]
    for name in ("abs", "ln_approx", "exp_approx", "sin_approx", "cos_approx"):
        p.append((name, "complex rows", True, TIME, lambda m, c, name=name: getattr(m, name)(), -1, D2))
    for name in ("log_approx", "expf_approx", "powf_approx"):
        p.append((name, "complex rows", True, TIME, lambda m, c, name=name: getattr(m, name)(2.0), -1, D2))
    for name in ("plain_sfft", "sfft", "windowed_sfft"):
        call = lambda m, c, name=name: getattr(m, name)(*((HAMMING,) if "windowed" in name else ()))
        p += [(name, "complex rows", True, TIME, call, 5, D2), (name, "frequency domain", False, FREQ, call, 5, D2),
              (name, "even N", False, TIME, call, 9, EVEN)]
    for name in ("plain_sifft", "sifft", "windowed_sifft"):
        call = lambda m, c, name=name: getattr(m, name)(*((HAMMING,) if "windowed" in name else ()))
        p += [(name, "time domain", True, TIME, call, 6, D2), (name, "real rows", False, FREQ, call, 6, D2)]
    for name in ("magnitude", "magnitude_squared", "to_real", "to_imag", "phase"):
        p.append((name, "real rows", False, TIME, lambda m, c, name=name: getattr(m, name)(), -1, D2))
    for name, domain in (("plain_fft", FREQ), ("fft", FREQ), ("windowed_fft", FREQ), ("plain_ifft", TIME), ("ifft", TIME), ("windowed_ifft", TIME)):
        args = (HAMMING,) if "windowed" in name else ()
        p.append((name, "wrong domain", True, domain, lambda m, c, name=name, args=args: getattr(m, name)(*args), -1, D2))
    return p


POISONERS = _poisoners()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_poisoning_calls_poison_a_transposed_matrix_as_documented(bd, dtype):
    for j, (method, label, cplx, domain, call, code, state) in enumerate(POISONERS):
        d, w = _build_states(bd, state, cplx, dtype, domain, (-10, 10), 6000 + j)
        rows = d.rows()
        assert rows == 5 and d.row_points() == (1000 if state == EVEN else 1001)
        ctx = Ctx(bd, dtype, cplx, domain, rows, d.row_points(), 6000 + j, True)
        assert call(d, ctx) == code, (method, label)
        poisoned = lambda: d.rows() == rows and d.row_len() == 0 and d.row_points() == 0 and np.isnan(d.delta()) and d.data().shape == (rows, 0)
        assert poisoned(), (method, label)
        for other in (lambda: d.scale(2.0), d.swap_halves, d.transpose, d.reverse):   # unrelated calls: -1, still poisoned
            assert other() == -1 and poisoned(), (method, label)


# ============================================================================================== part 4: above 65535 rows
BIG_ROWS = 70000
# the first 16, the 16 that straddle 65535, the last 16
BIG_SAMPLE = np.array(list(range(16)) + list(range(65528, 65544)) + list(range(BIG_ROWS - 16, BIG_ROWS)))
BIG_POINTS = (3, 16, 17, 30)
TRANSPOSED_BUILD = (16, 30)   # these two are made by transpose of the wide matrix, the other two are uploaded as they are
_BIG = {}


def _big_data(pts, cplx, dtype, rng=(-10, 10), salt=0):
    key = (pts, cplx, dtype, rng, salt)
    if key not in _BIG:
        x = _fill(BIG_ROWS, pts * (2 if cplx else 1), 90000 + 7 * pts + salt, dtype, *rng)
        x.setflags(write=False)
        _BIG[key] = x
    return _BIG[key]


def _big_mat(bd, x, cplx, domain, pts):
    """70000 rows of pts points; for the lengths of TRANSPOSED_BUILD the wide matrix [pts, 70000] is uploaded and
    transposed on the device"""
    if pts in TRANSPOSED_BUILD:
        e = 2 if cplx else 1
        wide = np.ascontiguousarray(x.reshape(BIG_ROWS, -1, e).transpose(1, 0, 2)).reshape(-1, BIG_ROWS * e)
        m = _mat(bd, wide, cplx, domain, DELTA)
        assert m.transpose() == 0 and m.rows() == BIG_ROWS
        return m
    return _mat(bd, x, cplx, domain, DELTA)


def _big_code(code, what):
    """No docstring and no line of include/basic_dsp_hip.h states a row-count limit for any of these operations, so
    success is the only allowed outcome; wrong data with code 0 is caught by the caller's reference."""
    assert code == 0, (what, "code", code)


BIG_CASES = [(d, p) for d in DTYPES for p in BIG_POINTS]
BIG_IDS = ["%s-%d" % (np.dtype(d).name, p) for d, p in BIG_CASES]


@pytest.mark.parametrize("dtype,pts", BIG_CASES, ids=BIG_IDS)
def test_more_than_65535_rows_transforms(bd, dtype, pts):
    """the six transforms on ALL rows against numpy's FFT in float64 along axis 1, real and complex rows; tolerance of
    test_transforms_of_every_row: per-row rel-L2 < 1e-6 / 1e-12.  17 points is Bluestein: one fused kernel for plain
    complex rows, the pre / transform / post route for real rows and wherever a shift, window or scale is fused in."""
    tol = _tol(dtype, 1e-6, 1e-12)
    for cplx in (False, True):
        x = _big_data(pts, cplx, dtype)
        xc = _to_complex64(x, cplx)
        for name in ("plain_fft", "fft", "windowed_fft", "plain_ifft", "ifft", "windowed_ifft"):
            args = (HAMMING,) if "windowed" in name else ()
            m = _big_mat(bd, x, cplx, FREQ if "ifft" in name else TIME, pts)
            what = (name, "complex" if cplx else "real", pts)
            _big_code(getattr(m, name)(*args), what)
            assert (m.rows(), m.row_points(), m.is_complex(), m.domain()) == (BIG_ROWS, pts, True, TIME if "ifft" in name else FREQ), what
            assert m.delta() == float(dtype(pts) * dtype(DELTA)), what
            _rows_close(m.data(), _fft_ref(xc, name), tol, what)


def _direct_max_taps():
    with open(os.path.join(ROOT, "basic_dsp_amd", "csrc", "capi.cpp")) as f:
        found = re.search(r"MAT_CONV_DIRECT_MAX_TAPS\s*=\s*(\d+)\s*;", f.read())
    assert found, "capi.cpp no longer defines MAT_CONV_DIRECT_MAX_TAPS as `MAT_CONV_DIRECT_MAX_TAPS = <number>;`"
    return int(found.group(1))


def _big_entries(pts):
    """(entry, is_complex) of the operations that are checked row by row on BIG_SAMPLE"""
    K = _direct_max_taps()
    ents = []
    for cplx in (False, True):
        ents += [(Entry("apply_window", lambda m, c: m.apply_window(HAMMING), _chk_window(False)), cplx),
                 (Entry("unapply_window", lambda m, c: m.unapply_window(HAMMING), _chk_window(True)), cplx),
                 (Entry("multiply_frequency_response", lambda m, c: m.multiply_frequency_response(RAISED_COSINE, MFR_RATIO, MFR_ROLLOFF),
                        _chk_mfr(RAISED_COSINE), domain=FREQ, rng=(-1, 1)), cplx),
                 (e_prepare_argument(False), cplx), (e_prepare_argument(True), cplx),
                 (e_resample(("interpolatei", SINC, 0.0, 2)), cplx), (e_resample(("interpolate", RAISED_COSINE, 0.35, 7, 0.25)), cplx),
                 (e_resample(("interpft", 5)), cplx), (e_convolve_signal(3), cplx),
                 (e_convolve(SINC, 0.0, 0.25, (K - 1) // 2), cplx), (e_convolve(SINC, 0.0, 0.25, (K - 1) // 2 + 1), cplx)]
    ents += [(e_correlate(kind, l), True) for kind in ("vector", "matrix") for l in (32, 35)]
    return ents


def _chk_mirror(c, x, got, extras):
    _same_bits(got, _per_row(orc.mirror, x), "mirror")        # test_gpu_mat_sym.py: bit-equal to the oracle


def _chk_decimatei(c, x, got, extras):
    _same_bits(got, _per_row(lambda r: orc.decimatei(r, c.cplx, 3, 1), x), "decimatei")   # test_gpu_mat_resample.py: bit-equal


@pytest.mark.parametrize("dtype,pts", BIG_CASES, ids=BIG_IDS)
def test_more_than_65535_rows_base_operations(bd, dtype, pts):
    """windows, frequency response, prepare_argument(_padded), correlate (vector and matrix argument of 32 and 35
    points), interpolatei / interpolate / interpft / decimatei, mirror, convolve_signal with a shared 3-tap filter and
    convolve(CONV_SINC) with (K - 1) / 2 and (K - 1) / 2 + 1 for K = MAT_CONV_DIRECT_MAX_TAPS -- on rows of at most 30
    points both have more taps than points and stay in the direct kernel; the block route is the test after next: 48
    rows (BIG_SAMPLE) each on its own against the oracle, with the tolerance of the operation's own test (quoted in the
    entry's check)."""
    ents = _big_entries(pts) + [(Entry("mirror", lambda m, c: m.mirror(), _chk_mirror, domain=FREQ), True),
                                (Entry("decimatei", lambda m, c: m.decimatei(3, 1), _chk_decimatei), False),
                                (Entry("decimatei", lambda m, c: m.decimatei(3, 1), _chk_decimatei), True)]
    for k, (entry, cplx) in enumerate(ents):
        x = _big_data(pts, cplx, dtype, entry.rng)
        m = _big_mat(bd, x, cplx, entry.domain, pts)
        ctx = Ctx(bd, dtype, cplx, entry.domain, BIG_ROWS, pts, 8000 + k, False)
        ctx.sel = BIG_SAMPLE
        what = (entry.label, "complex" if cplx else "real", pts)
        code, extras = _run_entry(entry, m, ctx)
        _big_code(code, what)
        assert m.rows() == BIG_ROWS and not np.isnan(m.delta()), what
        with np.errstate(all="ignore"):
            entry.check(ctx, x[BIG_SAMPLE], m.data()[BIG_SAMPLE], extras)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("n", (3, 17))
def test_more_than_65535_rows_symmetric_transforms(bd, dtype, n):
    """plain_sfft / sfft / windowed_sfft of real rows of odd length and their inverses on half spectra of (n + 1) / 2
    bins, ALL rows vectorised against numpy; tolerances of test_gpu_mat_sym.py (in e_sfft / e_sifft)."""
    x = _big_data(n, False, dtype)
    ctx = Ctx(bd, dtype, False, TIME, BIG_ROWS, n, 0, False)
    for name in ("plain_sfft", "sfft", "windowed_sfft"):
        entry = e_sfft(name)
        m = _big_mat(bd, x, False, TIME, n)
        _big_code(_run_entry(entry, m, ctx)[0], name)
        assert (m.rows(), m.row_points(), m.is_complex(), m.domain()) == (BIG_ROWS, n // 2 + 1, True, FREQ)
        entry.check(ctx, x, m.data(), [])
    p = n // 2 + 1
    ctx = Ctx(bd, dtype, True, FREQ, BIG_ROWS, p, 0, False)
    for name in ("plain_sifft", "sifft", "windowed_sifft"):
        h = _big_data(p, True, dtype, salt=1).copy()
        h[:, 1 if name == "plain_sifft" else 2 * (p // 2) + 1] = 0   # the bin the first-bin rule looks at is real
        entry = e_sifft(name)
        m = _big_mat(bd, h, True, FREQ, p)
        _big_code(_run_entry(entry, m, ctx)[0], name)
        assert (m.rows(), m.row_len(), m.is_complex(), m.domain()) == (BIG_ROWS, n, False, TIME)
        with np.errstate(all="ignore"):
            entry.check(ctx, h, m.data(), [])


@pytest.mark.parametrize("dtype,pts", BIG_CASES, ids=BIG_IDS)
def test_more_than_65535_rows_interpolatef(bd, dtype, pts):
    """one launch per row, so on its own: complex rows, integer factor; 48 rows against the float64 oracle, tolerance of
    test_interpolatef_of_every_row (2e-6 / 1e-12)."""
    entry = e_interpolatef(SINC, 0.0, 2.0, 8)
    x = _big_data(pts, True, dtype)
    m = _big_mat(bd, x, True, TIME, pts)
    ctx = Ctx(bd, dtype, True, TIME, BIG_ROWS, pts, 0, False)
    _big_code(_run_entry(entry, m, ctx)[0], "interpolatef")
    assert m.rows() == BIG_ROWS and m.row_points() == 2 * pts
    entry.check(ctx, x[BIG_SAMPLE], m.data()[BIG_SAMPLE], [])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_more_than_65535_rows_convolve_through_the_block_convolution(bd, dtype):
    """Rows of 30 points never leave the direct kernel (2 L + 1 > 30 wraps around the row), so this runs convolve on
    70000 rows of 40 points with MAT_CONV_DIRECT_MAX_TAPS + 2 = 35 taps: the reversed table goes to the batched block
    convolution with batch = rows > 65535.  48 rows against the float64 oracle, tolerance in e_convolve."""
    pts, L = 40, (_direct_max_taps() - 1) // 2 + 1
    assert _direct_max_taps() < 2 * L + 1 <= pts
    for cplx in (False, True):
        entry = e_convolve(SINC, 0.0, 0.25, L)
        x = _big_data(pts, cplx, dtype)
        m = _big_mat(bd, x, cplx, TIME, pts)
        ctx = Ctx(bd, dtype, cplx, TIME, BIG_ROWS, pts, 0, False)
        _big_code(_run_entry(entry, m, ctx)[0], ("convolve, block route", cplx))
        assert (m.rows(), m.row_points(), m.is_complex()) == (BIG_ROWS, pts, cplx)
        entry.check(ctx, x[BIG_SAMPLE], m.data()[BIG_SAMPLE], [])


# ============================================================================================== part 5: caches
@pytest.mark.parametrize("n,other", ((1009, 1013), (1001, 1003), (1000, 1004)))
def test_plans_of_other_lengths_and_precisions_do_not_disturb_a_plan(bd, n, other):
    """plain_fft at n points (1009: Bluestein, 1001: mixed radix, 1000), then another length, the inverse plan at n, the
    same in float64, then plain_fft at n again on the first data: bit-equal to the first result"""
    def run(name, pts, dtype, seed):
        m = _mat(bd, _fill(3, 2 * pts, seed, dtype), True, FREQ if "ifft" in name else TIME)
        assert getattr(m, name)() == 0
        return m.data()
    first = run("plain_fft", n, np.float32, 1)
    _rows_close(first, np.fft.fft(_z(_fill(3, 2 * n, 1, np.float32).astype(np.float64)), axis=1), 1e-6, ("plain_fft", n))
    for dtype in DTYPES:
        run("plain_fft", other, dtype, 2)
        run("plain_ifft", n, dtype, 3)
        run("plain_fft", n, dtype, 4)
    _same_bits(run("plain_fft", n, np.float32, 1), first, ("plain_fft again", n))


def _tap_table_sets():
    """40 (factor, conv_len, rolloff).  The reference evaluates the raised cosine by an expression that loses its digits
    where a tap lands next to the singularity 1 / (2 rolloff) (oracle_lib.exact_weights), so there orc.interpolatef in T
    is no reference at 2e-6: with a tap 0.008 away from it (factor 4, conv_len 9, rolloff 0.3351) two f32 evaluations of
    that expression, the oracle's and the kernel's, are 2.6e-6 apart.  A roll-off is therefore moved on in steps of
    0.0007 until every tap k / factor keeps 0.05 away from the singularity.  (The rule was added after set 38 of the
    first list missed the bound on the device; it changes which roll-offs are used, not the bound.)"""
    out = []
    for k in range(40):
        factor, conv_len, rolloff = float(2 + k % 3), 6 + k % 5, 0.2173 + 0.0031 * k
        while min(abs(j / factor - 1 / (2 * rolloff)) for j in range(int(conv_len * factor) + 2)) < 0.05:
            rolloff += 0.0007
        out.append((factor, conv_len, round(rolloff, 6)))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_interpolatef_tap_table_cached_and_uncached_routes_agree(bd, dtype):
    """40 parameter sets of the integer-factor path with roll-offs no other test uses: new keys, whatever the table
    held before.  The table holds 32 entries over all precisions, so a run that starts with fewer than 32 caches its
    first sets and sends the rest down the uncached route, and a run that finds the table full (the second precision,
    or any run after enough other tests) takes the uncached route alone; which of the two a set takes is not asserted.
    What is: each set twice on equal data, the
    second result is bit-equal to the first, and each is within test_interpolatef_of_every_row's tolerance (2e-6 /
    1e-12, per row) of orc.interpolatef in the matrix's precision -- the reference test_gpu_parity.py's
    test_interpolatef_both_paths holds the raised cosine at integer factors to (the weights are evaluated in T by the
    reference's own expression on both sides; against the float64 oracle the f32 tap table of set 1 is 9.4e-6 away)."""
    x = _fill(3, 2 * 333, 77, dtype)
    sets = _tap_table_sets()
    assert len(sets) == len(set(sets)) == 40
    for k, (factor, conv_len, rolloff) in enumerate(sets):
        outs = []
        for _ in range(2):
            m = _mat(bd, x, True, TIME, 1.0)
            assert m.interpolatef(RAISED_COSINE, factor, 0.0, conv_len, rolloff) == 0
            outs.append(m.data())
        _same_bits(outs[1], outs[0], ("second call", k))
        ref = _per_row(lambda r: orc.interpolatef(r, True, RAISED_COSINE, rolloff, dtype(factor), 0.0, conv_len)[0], x)
        _rows_close(outs[0], ref, _tol(dtype, 2e-6, 1e-12), ("interpolatef set", k))
