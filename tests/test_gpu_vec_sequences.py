"""DspVec under the state it carries from call to call.  Every other vector test builds a fresh vector, calls one method
and compares; here the vector has a history first: its live buffer is not the first allocation, the buffers were traded,
the capacity is not n + n / 8 + 64, the slack behind the valid length was written, the number space was changed.

  * Part 3, test_mover_sequences_*: generated sequences of 16 "movers" (tests/vec_model.py: the operations that only
    rearrange scalars).  After EVERY step the return codes, len / points / is_complex / domain, delta, allocated_len and
    the data -- bit for bit, as unsigned integers, so -0.0, NaN and Inf count -- equal the numpy model's, for the
    sequence's vector and for every other vector the step read or wrote; device_ptr() is non-null and 16-byte aligned
    (ew_map.h and vecmath.hip refuse anything else).  Only the scalars set_len() grew into are skipped.
  * Part 4, test_results_owe_nothing_to_history: every other public method (CATALOGUE) on "dirty" vectors
    (vec_model.DIRTY) and on a fresh vector of the same values and metadata: the same kernel on the same values with the
    same launch geometry, so code, metadata and bits are equal -- no tolerance (the library has no accumulating atomics).
    The fresh result is also held to the CPU oracle once per entry, with the tolerance of the method's own test, quoted as
    file:line next to each check.
  * Part 5, test_argument_errors_* / test_poisoning_calls_*: calls the library rejects on the host before any launch
    (each rejection is a line of capi.cpp) leave a dirty vector as it was, or poison it, as documented.
  * Part 6, test_a_process_that_has_lived_long: tests/vec_long_process.py in a process of its own.

tests/test_vec_model.py checks on the CPU that the model agrees with the oracle, what the sequences cover, that the dirty
recipes reach the states they name and that every public DspVec method is a mover, an accessor or in CATALOGUE."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
import vec_model as vm
from vec_model import FREQ, PAD_SURROUND, TIME

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = (np.float32, np.float64)
HAMMING = 1
SINC, RAISED_COSINE = 0, 1
DELTA = 0.5


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


# ---------------------------------------------------------------------------------------------- helpers
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])


def _same_bits(got, ref, what, skip=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    differ = _bits(got) != _bits(ref)
    if skip is not None:
        differ &= ~skip
    if differ.any():
        bad = np.flatnonzero(differ)
        raise AssertionError((what, "first differing scalars", bad[:4].tolist(), "of", int(bad.size)))


def _meta(v):
    return (v.len(), v.points(), bool(v.is_complex()), v.domain())


def _same_state(got, want, what):
    """metadata, delta (exactly) and data (bit for bit) of two vectors from either side; against a model also the
    capacity, and the scalars the model marks unspecified (and only those) are not compared"""
    assert _meta(got) == _meta(want), (what, _meta(got), _meta(want))
    a, b = got.delta(), want.delta()
    assert a == b or (np.isnan(a) and np.isnan(b)), (what, "delta", a, b)
    assert bool(got.is_erroneous()) == bool(want.is_erroneous()), what
    model = isinstance(want, vm.VecModel)
    if model:
        assert got.allocated_len() == want.allocated_len(), (what, "allocated_len", got.allocated_len(), want.allocated_len())
    _same_bits(got.data(), want.data(), what, want.unspec if model else None)


def _aligned(v, what):
    p = v.device_ptr()
    assert p and p % 16 == 0, (what, "device_ptr", p)


def _vec(bd, a, cplx, domain=TIME, delta=1.0):
    return bd.DspVec(np.ascontiguousarray(a), is_complex=cplx, domain=domain, delta=delta)


class _Api:
    """the GPU side of vec_model.apply_step / build_dirty"""

    def __init__(self, bd):
        self.bd = bd

    def vec(self, a, is_complex, domain, delta):
        return _vec(self.bd, a, is_complex, domain, delta)

    def set_len(self, v, n):
        getattr(self.bd.lib, "set_len" + v._sfx)(v._h, int(n))   # DspVec has no wrapper for the C ABI's set_len


def _fill(n, seed, dtype, lo=-10, hi=10):
    return orc.fill_uniform(n, seed, lo, hi, dtype)


def _as_real(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return np.ascontiguousarray(a.astype(np.complex128)).view(np.float64)
    return a.astype(np.float64)


def rel_l2(got, ref):
    got, ref = _as_real(got).ravel(), _as_real(ref).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def _close(got, ref, tol, what):
    err = rel_l2(got, ref)
    print("%s: rel-L2 %.3e (bound %.1e)" % (what, err, tol))
    assert err < tol, (what, err, tol)


def _z(x):
    return np.ascontiguousarray(np.asarray(x).astype(np.float64)).view(np.complex128)


def _zc(x, cplx):
    """a vector's values as complex128 points (a real vector: zero imaginary parts)"""
    return _z(x) if cplx else np.asarray(x).astype(np.complex128)


def _hamming(n, cplx=True):
    """the oracle's Hamming window of n points, float64"""
    with np.errstate(all="ignore"):
        w = orc.apply_window(np.ones(2 * n if cplx else n), cplx, 1, 0.54)
    return w[0::2] if cplx else w


def _ham_cb(n, length):
    return 0.54 - 0.46 * np.cos(2 * np.pi * n / (length - 1))


def _tol(dtype, f32, f64):
    return f32 if dtype == np.float32 else f64


def tol_for(dtype):
    return _tol(dtype, 1e-6, 1e-12)   # tests/test_gpu_parity.py:33-34


# ============================================================================================== part 3: mover sequences
_SEQ = {}


def _sequence(pts, cplx, seed):
    key = (pts, cplx, seed)
    if key not in _SEQ:
        _SEQ[key] = vm.gen_sequence(*key)[0]
    return _SEQ[key]


def _start_data(pts, cplx, dtype, seed):
    """uniform noise with -0.0, +0.0, a NaN and both infinities planted (as many as the size holds): movers must carry
    them unchanged, conj and mirror flip their sign bit"""
    x = _fill(pts * (2 if cplx else 1), 7000 + seed, dtype)
    n = x.size
    for k, v in ((0, -0.0), (n // 2, np.nan), (n - 1, np.inf), (n // 3, 0.0), (2 * n // 3, -0.0), (n // 5, -np.inf)):
        if k == 0 or n >= 8:
            x[k] = v
    if n == 2:
        x[1] = np.nan
    return x


SEQ_CASES = [(p, c, d, dom) for p in vm.START_POINTS for c in (False, True) for d in DTYPES for dom in (TIME, FREQ)]


@pytest.mark.parametrize("pts,cplx,dtype,domain", SEQ_CASES,
                         ids=["%d-%s-%s-%s" % (p, "complex" if c else "real", np.dtype(d).name, "freq" if dom else "time")
                              for (p, c, d, dom) in SEQ_CASES])
def test_mover_sequences_equal_the_model_at_every_step(bd, pts, cplx, dtype, domain):
    """16 sequences of 16 movers from this start state; nothing is skipped.  The step assertion names the seed, the step
    index and the step: a swap_halves that forgot the buffer trade, or a zero_pad that reserved for the wrong length,
    fails here at that step (data bits in the first case, allocated_len in the second)."""
    api = _Api(bd)
    for seed in vm.SEEDS:
        x = _start_data(pts, cplx, dtype, seed)
        g, w = api.vec(x, cplx, domain, 0.25), vm.VecModel(x, cplx, domain, 0.25)
        _same_state(g, w, (seed, "start"))
        for i, step in enumerate(_sequence(pts, cplx, seed)):
            what = ("seed", seed, "step", i, step)
            g_codes, g, g_side = vm.apply_step(api, g, step)
            w_codes, w, w_side = vm.apply_step(vm.ModelApi, w, step)
            assert g_codes == w_codes, (what, "codes", g_codes, w_codes)
            _same_state(g, w, what)
            _aligned(g, what)
            assert len(g_side) == len(w_side)
            for k, (a, b) in enumerate(zip(g_side, w_side)):   # sources stay as they were, destinations are right
                _same_state(a, b, (what, "side vector", k))
                _aligned(a, (what, "side vector", k))


# ============================================================================================== part 4: the catalogue
class Ctx:
    """what a catalogue entry's call and check see: the state's description and the operands"""

    def __init__(self, bd, dtype, cplx, domain, points, seed, dirty):
        self.bd, self.dtype, self.cplx, self.domain, self.points = bd, dtype, cplx, domain, points
        self.e = 2 if cplx else 1
        self.seed, self.dirty, self.arrays = seed, dirty, {}

    def vec(self, k, points=None, lo=-10, hi=10, scale=1.0, cplx=None, domain=None):
        """operand vector k of `points` points (default: the state's).  Dirty: uploaded zero-interleaved and decimated
        on the device (shrunk, traded); fresh: uploaded as it is.  Equal values either way."""
        cplx = self.cplx if cplx is None else cplx
        domain = self.domain if domain is None else domain
        points = self.points if points is None else points
        e = 2 if cplx else 1
        base = (_fill(points * e, self.seed + 211 * k, self.dtype, lo, hi) * self.dtype(scale)).astype(self.dtype)
        self.arrays[k] = base
        if self.dirty and base.size:
            wide = np.zeros((points, 2, e), self.dtype)
            wide[:, 0, :] = base.reshape(points, e)
            v = _vec(self.bd, wide.reshape(-1), cplx, domain, DELTA)
            assert v.decimatei(2, 0) == 0 and v.points() == points
            return v
        return _vec(self.bd, base, cplx, domain, DELTA)

    def small(self, scalars=5):
        """a destination of another length and delta than anything a getter produces"""
        return _vec(self.bd, np.ones(scalars, self.dtype), False, self.domain, 0.125)

    def divisor(self):
        """the smallest number of points > 1 that divides the state's (its own for a prime, 1 for one point)"""
        p = self.points
        return next((d for d in range(2, p + 1) if p % d == 0), 1)


class Entry:
    def __init__(self, method, call, check=None, label=None, space=None, domain=TIME, rng=(-10, 10), pre=None, prep=None):
        """call(v, ctx) -> code or (code, extras): extras are vectors, arrays, numbers or dicts the call produced.
        check(ctx, x, got, extras): the oracle assertions on values x -> got.  space: "real" / "complex" / None (both):
        a dirty state of the other number space is brought over by to_complex / to_real, two more movers in its history.
        pre(points): the method's precondition on the length.  prep(v): movers that bring the dirty vector into the
        method's domain of definition before the fresh copy is taken."""
        self.method, self.call, self.check, self.label = method, call, check, label or method
        self.space, self.domain, self.rng, self.pre, self.prep = space, domain, rng, pre, prep


def _chk_bits(fn):
    def check(c, x, got, extras):
        _same_bits(got, fn(c, x), "oracle, bit-exact")
    return check


# ---- elementwise -----------------------------------------------------------------------------------------------------
def e_elementwise():
    def chk_divide(c, x, got, extras):   # tests/test_gpu_parity.py:1056-1057: rel-L2 < 1e-6 / 1e-14
        _close(got, _z(x) / (2.0 - 1.5j), _tol(c.dtype, 1e-6, 1e-14), "complex_divide")

    def chk_cexp(c, x, got, extras):
        # tests/test_gpu_parity.py:118-120: rel-L2 < 2e-7 / 1e-14 against the exact float64 phase; a and b are multiplied
        # by delta in T first
        a, b = float(c.dtype(0.02) * c.dtype(DELTA)), float(c.dtype(0.3) * c.dtype(DELTA))
        _close(got, _z(x) * np.exp(1j * (a * np.arange(x.size // 2) + b)), _tol(c.dtype, 2e-7, 1e-14), "multiply_complex_exponential")
    return [  # tests/test_gpu_parity.py:51, :60, :63, :66: bit-equal to the oracle
        Entry("scale", lambda v, c: v.scale(2.5), _chk_bits(lambda c, x: orc.real_scale(x, 2.5))),
        Entry("scale", lambda v, c: v.scale(complex(0.5, -1.5)), _chk_bits(lambda c, x: orc.complex_scale(x, 0.5, -1.5)),
              label="scale(complex)", space="complex"),
        Entry("offset", lambda v, c: v.offset(-1.25), _chk_bits(lambda c, x: orc.real_offset(x, -1.25, c.cplx))),
        Entry("offset", lambda v, c: v.offset(complex(3.0, -2.0)), _chk_bits(lambda c, x: orc.complex_offset(x, 3.0, -2.0)),
              label="offset(complex)", space="complex"),
        Entry("complex_divide", lambda v, c: v.complex_divide(2.0 - 1.5j), chk_divide, space="complex"),
        Entry("multiply_complex_exponential", lambda v, c: v.multiply_complex_exponential(0.02, 0.3), chk_cexp, space="complex")]


def e_binary(name, op, smaller=False):
    method = name + ("_smaller" if smaller else "")

    def call(v, c):   # operands from (1, 10): div stays tame (tests/test_gpu_parity.py:1015)
        return getattr(v, method)(c.vec(1, c.divisor() if smaller else None, 1, 10))

    def check(c, x, got, extras):
        y = c.arrays[1]
        ref = orc.binary(x, np.tile(y, x.size // y.size), c.cplx, op)[1]
        if name == "div" and c.cplx and not smaller:   # tests/test_gpu_parity.py:77: complex division within 4 eps
            np.testing.assert_allclose(got, ref, rtol=4 * np.finfo(c.dtype).eps)
        else:                                          # :79, :1020: everything else bit-equal
            _same_bits(got, ref, method)
    return Entry(method, call, check, pre=(lambda p: p >= 1) if smaller else None)   # (*_smaller: an empty operand is code 7)


def e_complex_to_real(name, kind, getter=False):
    def call(v, c):
        if not getter:
            return getattr(v, name)()
        dst = c.small()
        return getattr(v, name)(dst), [dst]

    def check(c, x, got, extras):
        if getter:
            got = extras[0].data()
        ref = orc.complex_to_real(x, kind)
        if kind == 1:   # tests/test_gpu_parity.py:104, :1419: magnitude_squared bit-equal
            _same_bits(got, ref, name)
        else:
            # :106: magnitude and phase within 4 eps rel and abs.  (:1421 holds the getters to 2e-6 in f32 only; they
            # run the same kernel into another buffer, so the tighter :106 covers them, in both precisions.)
            eps = np.finfo(c.dtype).eps
            np.testing.assert_allclose(got, ref, rtol=4 * eps, atol=4 * eps)
    return Entry(name, call, check, space="complex")


def e_pairs():
    def call_get(v, c):
        mag, ph = c.small(5), c.small(3)
        return v.get_mag_phase(mag, ph), [mag, ph]

    def chk_get(c, x, got, extras):
        # tests/test_gpu_parity.py:1613-1614: magnitudes rel-L2 < tol = 2e-6 / 1e-14, phases within 4 tol absolute
        tol = _tol(c.dtype, 2e-6, 1e-14)
        mag, ph = orc.get_mag_phase(x.astype(np.float64))
        _close(extras[0].data(), mag, tol, "get_mag_phase, magnitudes")
        assert np.max(np.abs(extras[1].data() - ph)) < 4 * tol

    def chk_set(c, x, got, extras):
        # tests/test_gpu_parity.py:1616: rel-L2 < 4 tol, tol = 2e-6 / 1e-14
        _close(got, orc.set_mag_phase(c.arrays[1].astype(np.float64), c.arrays[2].astype(np.float64)),
               4 * _tol(c.dtype, 2e-6, 1e-14), "set_mag_phase")
    return [Entry("get_mag_phase", call_get, chk_get, space="complex"),
            Entry("set_mag_phase", lambda v, c: v.set_mag_phase(c.vec(1, None, 0, 10, cplx=False), c.vec(2, None, -3, 3, cplx=False)),
                  chk_set, space="complex")]


# ---- windows ---------------------------------------------------------------------------------------------------------
def _ulp_of_10(dtype):
    return float(np.spacing(np.asarray(10.0, dtype=dtype)))


def e_windows():
    def chk_window(unapply):
        def check(c, x, got, extras):
            # tests/test_gpu_parity.py:186: Hamming within 4 ulp of 10 absolute; :195-196: unapply within 4 * 4 ulp / 1e-2
            # where the window exceeds 1e-2 (Hamming does everywhere from two points on)
            with np.errstate(all="ignore"):
                ref = orc.apply_window(x, c.cplx, 1, 0.54, unapply=unapply)
            atol = 4 * _ulp_of_10(c.dtype) * (4 / 1e-2 if unapply else 1)
            np.testing.assert_allclose(got.astype(np.float64), ref.astype(np.float64), rtol=0, atol=atol)
        return check

    def chk_custom(c, x, got, extras):
        # tests/test_gpu_parity.py:1028-1029: the callback window equals the built-in Hamming, rel-L2 < 1e-6 / 1e-14
        b = _vec(c.bd, x, c.cplx, c.domain, DELTA)
        assert b.apply_window(HAMMING) == 0
        _close(got, b.data(), _tol(c.dtype, 1e-6, 1e-14), "apply_custom_window")

    def call_round_trip(v, c):
        code = v.apply_custom_window(_ham_cb, True)
        return code or v.unapply_custom_window(_ham_cb, False)

    def chk_round_trip(c, x, got, extras):
        # tests/test_gpu_parity.py:1030-1031: applied and unapplied, back at the input, rel-L2 < 1e-6 / 1e-14
        _close(got, x, _tol(c.dtype, 1e-6, 1e-14), "unapply_custom_window")
    two = lambda p: p != 1   # (one point: the Hamming formula divides by length - 1 = 0)
    return [Entry("apply_window", lambda v, c: v.apply_window(HAMMING), chk_window(False)),
            Entry("unapply_window", lambda v, c: v.unapply_window(HAMMING), chk_window(True), pre=two),
            Entry("apply_custom_window", lambda v, c: v.apply_custom_window(_ham_cb, True), chk_custom, pre=two),
            Entry("unapply_custom_window", call_round_trip, chk_round_trip, label="apply_custom_window -> unapply_custom_window",
                  pre=two)]


# ---- transforms ------------------------------------------------------------------------------------------------------
def _fft_ref(z, name):
    n = z.size
    with np.errstate(all="ignore"):
        if name == "plain_fft":
            return np.fft.fft(z)
        if name == "fft":
            return np.roll(np.fft.fft(z), n // 2)
        if name == "windowed_fft":
            return np.roll(np.fft.fft(z * _hamming(n)), n // 2)
        if name == "plain_ifft":
            return np.fft.ifft(z) * n
        out = np.fft.ifft(np.roll(z, -(n // 2)))   # ifft = scale(1 / n) -> ifft_shift -> plain_ifft
        return out / _hamming(n) if name == "windowed_ifft" else out


def e_fft(name):
    args = (HAMMING,) if "windowed" in name else ()

    def check(c, x, got, extras):
        # tests/test_gpu_parity.py:213, :236 (plain_fft), :271 (fft), :279 (windowed_fft): one transform against the
        # float64 transform within tol_for = 1e-6 / 1e-12.  test_gpu_parity.py checks the inverse forms by round trips
        # only; one inverse transform against numpy is held to the same 1e-6 / 1e-12 by
        # tests/test_gpu_mat_basic.py:96 (test_transforms_of_every_row, the same kernels): that bound is used.
        _close(got, _fft_ref(_zc(x, c.cplx), name), tol_for(c.dtype), name)
    return Entry(name, lambda v, c: getattr(v, name)(*args), check, domain=FREQ if "ifft" in name else TIME)


def e_custom_fft(name, builtin, f32, f64, where, **kw):
    def check(c, x, got, extras):
        b = _vec(c.bd, x, c.cplx, c.domain, DELTA)
        assert getattr(b, builtin)(HAMMING) == 0
        _close(got, b.data(), _tol(c.dtype, f32, f64), "%s against %s (%s)" % (name, builtin, where))
    return Entry(name, lambda v, c: getattr(v, name)(_ham_cb, True), check, **kw)


def e_sfft(name):
    args = (HAMMING,) if "windowed" in name else ()

    def check(c, x, got, extras):
        # tests/test_gpu_parity.py:851 (plain_sfft), :891 (sfft), :898 (windowed_sfft): rel-L2 < 2 tol, tol = 1e-6 / 1e-12
        n = x.size
        p = n // 2 + 1
        xd = x.astype(np.float64)
        if name == "plain_sfft":
            ref = np.fft.fft(xd)[:p]
        else:
            ref = np.roll(np.fft.fft(xd * (_hamming(n, False) if args else 1.0)), n // 2)[:p]
        _close(got, ref, 2 * tol_for(c.dtype), name)
    return Entry(name, lambda v, c: getattr(v, name)(*args), check, space="real", pre=lambda p: p % 2 == 1)


def _real_spectrum(v):
    """imaginary parts <- 0 by two movers: every half spectrum then passes the first-bin rule, shifted or not"""
    assert v.to_real() == 0 and v.to_complex() == 0


def e_sifft(name):
    args = (HAMMING,) if "windowed" in name else ()

    def check(c, x, got, extras):
        # tests/test_gpu_parity.py:912 (sifft: rel-L2 < 2 tol), :917 (windowed_sifft: < 4 tol), tol = 1e-6 / 1e-12;
        # plain_sifft is sifft without its scale and shift and is held to :912 too (:857 has it in a round trip, < 4 tol)
        h = _z(x)
        p = h.size
        n = 2 * p - 1
        if name != "plain_sifft":   # scale(1 / p) and ifft_shift of the HALF spectrum come first
            h = np.roll(h / p, -(p // 2))
        ref = np.real(np.fft.ifft(np.concatenate([h, np.conj(h[:0:-1])])) * n)
        if args:
            ref = ref / _hamming(n, False)
        _close(got, ref, (4 if args else 2) * tol_for(c.dtype), name)
    return Entry(name, lambda v, c: getattr(v, name)(*args), check, space="complex", domain=FREQ, prep=_real_spectrum,
                 pre=lambda p: p >= 1)


# ---- convolution, correlation, frequency responses --------------------------------------------------------------------
def e_convolve_signal(taps):
    def check(c, x, got, extras):
        # tests/test_gpu_parity.py:326 (complex) and :411 (real): rel-L2 < tol_for = 1e-6 / 1e-12 against the direct form
        # in float64, up to 1025 taps (CONV_CASES :308-314 has 1024 and 1025); more taps: :1338, :1357 -- 2e-6 / 1e-11
        # against the direct form
        ref = orc.convolve_direct(x.astype(np.float64), c.arrays[1].astype(np.float64), c.cplx)
        _close(got, ref, tol_for(c.dtype) if taps <= 1025 else _tol(c.dtype, 2e-6, 1e-11), "convolve_signal(%d)" % taps)
    return Entry("convolve_signal", lambda v, c: v.convolve_signal(c.vec(1, taps, -1, 1, 1.0 / taps)), check,
                 label="convolve_signal(%d taps)" % taps, pre=lambda p: p >= taps)


def e_convolve(fid, rolloff, ratio, conv_len, how="builtin"):
    def call(v, c):
        if how == "callable":
            return v.convolve(lambda t: float(np.sinc(t)), ratio, conv_len)
        if how == "complex":
            return v.convolve_complex(lambda t: complex(np.sinc(t), 0.0), ratio, conv_len)
        return v.convolve(fid, ratio, conv_len, rolloff=rolloff)

    def check(c, x, got, extras):
        # tests/test_gpu_parity.py:967, :977 (built-in), :983 (callable): rel-L2 < 2e-6 / 1e-12 against the float64
        # oracle; :1659, :1666-1668 (convolve_complex with a real-valued response): < 5e-6 / 1e-11
        ref = orc.convolve_function(x.astype(np.float64), c.cplx, fid, rolloff, ratio, conv_len)
        _close(got, ref, _tol(c.dtype, 5e-6, 1e-11) if how == "complex" else _tol(c.dtype, 2e-6, 1e-12), "convolve")
    method = "convolve_complex" if how == "complex" else "convolve"
    return Entry(method, call, check, label="%s(%s, %d, L=%d)" % (method, how, fid, conv_len),
                 space="complex" if how == "complex" else None)


MFR_RATIO, MFR_ROLLOFF = 1.7, 0.35


def e_frequency_responses():
    def chk_builtin(fid):
        def check(c, x, got, extras):
            # tests/test_gpu_parity.py:837: float64 within 1e-12 absolute.  test_gpu_parity.py has no float32 bound
            # against the oracle; tests/test_gpu_mat_basic.py:251-252, :288 holds the DspVec path in float32 to 4 ulp of
            # max |reference|: that bound is used
            ref = orc.multiply_frequency_response(x, c.cplx, fid, MFR_ROLLOFF, MFR_RATIO, False)
            if c.dtype == np.float64:
                np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
                return
            top = np.max(np.abs(ref.astype(np.float64)))
            ulp = float(np.spacing(np.asarray(top if top > 0 else 1.0, dtype=ref.dtype)))
            assert float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)))) / ulp <= 4.0
        return check

    def chk_fn(c, x, got, extras):
        # tests/test_gpu_parity.py:1050-1052: the callback equals the built-in raised cosine, rel-L2 < 1e-6 / 1e-13
        b = _vec(c.bd, x, c.cplx, FREQ, DELTA)
        assert b.multiply_frequency_response(RAISED_COSINE, MFR_RATIO, MFR_ROLLOFF) == 0
        _close(got, b.data(), _tol(c.dtype, 1e-6, 1e-13), "multiply_frequency_response_fn")
    fr = lambda t: complex(1.0 / (1.0 + t * t), 0.5 * t)

    def chk_complex(c, x, got, extras):
        # tests/test_gpu_parity.py:1659, :1683-1688: natural-order axis j / max * ratio, scaled by ratio; < 5e-6 / 1e-11
        points = x.size // 2
        maxv = (points - points % 2) / 2
        hh = np.array([0.5 * fr((-maxv + i) / maxv * 0.5) for i in range(points)])
        _close(got, _z(x) * hh, _tol(c.dtype, 5e-6, 1e-11), "multiply_frequency_response_complex")
    out = [Entry("multiply_frequency_response", lambda v, c, fid=fid: v.multiply_frequency_response(fid, MFR_RATIO, MFR_ROLLOFF),
                 chk_builtin(fid), label="multiply_frequency_response(%d)" % fid, domain=FREQ, rng=(-1, 1)) for fid in (SINC, RAISED_COSINE)]
    out.append(Entry("multiply_frequency_response_fn",
                     lambda v, c: v.multiply_frequency_response_fn(lambda t: float(orc.conv_freq(1, MFR_ROLLOFF, t, np.float64)), MFR_RATIO),
                     chk_fn, domain=FREQ, rng=(-1, 1)))
    out.append(Entry("multiply_frequency_response_complex", lambda v, c: v.multiply_frequency_response_complex(fr, 0.5),
                     chk_complex, space="complex", domain=FREQ, pre=lambda p: p >= 2))
    return out


def e_correlation():
    def chk_prepare(padded):
        def check(c, x, got, extras):
            # tests/test_gpu_parity.py:936, :944: rel-L2 < 2e-6 / 1e-12
            z = np.ascontiguousarray(_zc(x, c.cplx)).view(np.float64)
            _close(got, orc.prepare_argument(z, padded)[1], _tol(c.dtype, 2e-6, 1e-12), "prepare_argument")
        return check

    def call_correlate(v, c):
        arg = c.vec(1)
        assert arg.prepare_argument_padded() == 0
        return v.correlate(arg)

    def chk_correlate(c, x, got, extras):
        # tests/test_gpu_parity.py:936, :950: rel-L2 < 2e-6 / 1e-12, the argument from the oracle
        code, ref_arg = orc.prepare_argument(c.arrays[1].astype(np.float64), True)
        code2, ref = orc.correlate(x.astype(np.float64), ref_arg)
        assert code == 0 and code2 == 0
        _close(got, ref, _tol(c.dtype, 2e-6, 1e-12), "correlate")
    two = lambda p: p >= 2
    return [Entry("prepare_argument", lambda v, c: v.prepare_argument(), chk_prepare(False), pre=two),
            Entry("prepare_argument_padded", lambda v, c: v.prepare_argument_padded(), chk_prepare(True), pre=two),
            Entry("correlate", call_correlate, chk_correlate, space="complex", pre=two)]


# ---- interpolation ---------------------------------------------------------------------------------------------------
def _vs_builtin(name, builtin_call, f32, f64, where):
    def check(c, x, got, extras):
        b = _vec(c.bd, x, c.cplx, c.domain, DELTA)
        assert builtin_call(b, c) == 0
        _close(got, b.data(), _tol(c.dtype, f32, f64), "%s against the built-in (%s)" % (name, where))
    return check


def e_interpolatef(fid, rolloff, factor, conv_len):
    def check(c, x, got, extras):
        # tests/test_gpu_parity.py:586, :588-595: rel-L2 < 2e-6 / 1e-13 against the oracle in the vector's precision (these
        # are two of its parameter sets: the tap-table path and the fractional path)
        ref = orc.interpolatef(x, c.cplx, fid, rolloff, c.dtype(factor), 0.0, conv_len)[0]
        assert got.size == ref.size
        _close(got, ref, _tol(c.dtype, 2e-6, 1e-13), "interpolatef")
    return Entry("interpolatef", lambda v, c: v.interpolatef(fid, factor, 0.0, conv_len, rolloff), check,
                 label="interpolatef(%d, %g)" % (fid, factor))


def e_resample(op):
    """op: ("interpolatei", fid, rolloff, factor) | ("interpolate", fid, extra points, delay) | ("interpft", extra
    points) (a negative `extra points`: fewer)"""
    def dest(points):
        return max(points + op[2 if op[0] == "interpolate" else 1], 1)

    def call(v, c):
        if op[0] == "interpolatei":
            return v.interpolatei(op[1], op[3], op[2])
        if op[0] == "interpolate":
            return v.interpolate(op[1], dest(v.points()), op[3])
        return v.interpft(dest(v.points()))

    def check(c, x, got, extras):
        # tests/test_gpu_parity.py:796, :806: interpolatei rel-L2 < 5e-6 / 1e-11; :814 interpolate and :819 interpft
        # < 2e-5 / 1e-10, against the float64 oracle
        points, x64 = x.size // c.e, x.astype(np.float64)
        if op[0] == "interpolatei":
            code, ref = orc.interpolatei(x64, c.cplx, op[1], op[2], op[3])
        elif op[0] == "interpolate":
            code, ref, _ = orc.interpolate(x64, c.cplx, op[1], 0.0, dest(points), op[3], DELTA)
        else:
            code, ref, _ = orc.interpolate(x64, c.cplx, -1, 0.0, dest(points), 0.0, DELTA)
        assert code == 0 and got.size == ref.size
        _close(got, ref, _tol(c.dtype, 5e-6, 1e-11) if op[0] == "interpolatei" else _tol(c.dtype, 2e-5, 1e-10), op[0])
    return Entry(op[0], call, check, label="%s%s" % (op[0], op[1:]), pre=lambda p: p >= 1)


def e_custom_interpolation():
    box = lambda t: 1.0 if abs(t) <= 1.0 else 0.0
    sinc = lambda t: float(np.sinc(t))
    # tests/test_gpu_parity.py:1659: tol = 5e-6 / 1e-11; :1695-1696 interpolatei_custom and :1698-1700 interpolate_custom
    # equal the built-in sinc within tol, :1703-1704 interpolatef_custom within 4 tol
    return [Entry("interpolatei_custom", lambda v, c: v.interpolatei_custom(box, 3),
                  _vs_builtin("interpolatei_custom", lambda b, c: b.interpolatei(SINC, 3), 5e-6, 1e-11, "test_gpu_parity.py:1696"),
                  pre=lambda p: p >= 1),
            Entry("interpolate_custom", lambda v, c: v.interpolate_custom(box, v.points() + 37, 0.0),
                  _vs_builtin("interpolate_custom", lambda b, c: b.interpolate(SINC, b.points() + 37, 0.0), 5e-6, 1e-11,
                              "test_gpu_parity.py:1700"), pre=lambda p: p >= 1),
            # (:1701: factor 4 takes the tap table, 2.5 the path that samples the callback for every output and tap -- on
            # the states of at most 1100 points, for the time that takes)
            Entry("interpolatef_custom", lambda v, c: v.interpolatef_custom(sinc, 4.0, 0.0, 12),
                  _vs_builtin("interpolatef_custom", lambda b, c: b.interpolatef(SINC, 4.0, 0.0, 12), 4 * 5e-6, 4 * 1e-11,
                              "test_gpu_parity.py:1704"), label="interpolatef_custom(4)"),
            Entry("interpolatef_custom", lambda v, c: v.interpolatef_custom(sinc, 2.5, 0.0, 8),
                  _vs_builtin("interpolatef_custom", lambda b, c: b.interpolatef(SINC, 2.5, 0.0, 8), 4 * 5e-6, 4 * 1e-11,
                              "test_gpu_parity.py:1704"), label="interpolatef_custom(2.5)", pre=lambda p: p <= 1100)]


# ---- math family, differences, running sums, phase wrapping (tests/test_gpu_parity.py:1484-1492: the ranges that keep
# the functions real-valued) -------------------------------------------------------------------------------------------
_MATH_DOMAINS = {
    "sqrt": (0.0, 50.0), "square": (-10, 10), "ln": (1e-3, 50.0), "exp": (-10, 10), "sin": (-10, 10), "cos": (-10, 10),
    "tan": (-1.4, 1.4), "asin": (-0.99, 0.99), "acos": (-0.99, 0.99), "atan": (-10, 10), "sinh": (-8, 8),
    "cosh": (-8, 8), "tanh": (-8, 8), "asinh": (-10, 10), "acosh": (1.01, 50.0), "atanh": (-0.99, 0.99),
    "abs": (-10, 10), "ln_approx": (1e-3, 50.0), "exp_approx": (-10, 10), "sin_approx": (-10, 10),
    "cos_approx": (-10, 10)}
_MATH_ARGS = {"powf": ((0.1, 10.0), 2.5), "root": ((0.1, 10.0), 3.0), "log": ((1e-3, 50.0), 10.0),
              "expf": ((-3, 3), 10.0), "wrap": ((-20, 20), 4.0), "log_approx": ((1e-3, 50.0), 10.0),
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
        ref = _oracle_math(x, cplx, name, arg or 0.0)
        if cplx:   # tests/test_gpu_parity.py:1528, :1535, :1539: complex rel-L2 < 2e-5 / 1e-12
            _close(got, ref, _tol(c.dtype, 2e-5, 1e-12), name)
        else:      # :1513, :1520: max |got - ref| / (|ref| + 1) < 3e-6 / 1e-13; :1526: four times that with an argument
            tol = _tol(c.dtype, 3e-6, 1e-13) * (4 if args else 1)
            assert float(np.max(np.abs(got - ref) / (np.abs(ref) + 1.0))) < tol, name
    rng = (-3, 3) if cplx else (_MATH_ARGS[name][0] if args else _MATH_DOMAINS[name])
    return Entry(name, lambda v, c: getattr(v, name)(*args), check, label="%s(%s)" % (name, "complex" if cplx else "real"),
                 space="complex" if cplx else "real", rng=rng)


def e_scan():
    def chk_cum_sum(c, x, got, extras):
        # tests/test_gpu_parity.py:1575-1578: max |got - prefix| / (max |prefix| + 1) < 2e-7 / 1e-13
        ref = np.cumsum(x.astype(np.float64).reshape(-1, c.e), axis=0).reshape(-1)
        assert np.max(np.abs(got - ref)) / (np.max(np.abs(ref)) + 1.0) < _tol(c.dtype, 2e-7, 1e-13)
    return [Entry("diff", lambda v, c: v.diff(), _chk_bits(lambda c, x: orc.diff(x, c.cplx))),   # test_gpu_parity.py:1572: bit-equal
            Entry("diff_with_start", lambda v, c: v.diff_with_start(), _chk_bits(lambda c, x: orc.diff(x, c.cplx, True))),
            Entry("cum_sum", lambda v, c: v.cum_sum(), chk_cum_sum),
            # test_gpu_parity.py:1584-1588: bit-equal (random data in (-30, 30), divisor 7)
            Entry("unwrap", lambda v, c: v.unwrap(c.dtype(7.0)), _chk_bits(lambda c, x: orc.unwrap(x, c.dtype(7.0))),
                  space="real", rng=(-30, 30))]


def e_interpolate_real(name, factor, delay):
    # tests/test_gpu_parity.py:997, :1006: bit-equal to the oracle in the vector's precision
    return Entry(name, lambda v, c: getattr(v, name)(factor, delay), _chk_bits(lambda c, x: getattr(orc, name)(x, factor, delay)),
                 space="real")


# ---- host callbacks ---------------------------------------------------------------------------------------------------
def e_maps():
    def chk_inplace(c, x, got, extras):
        # tests/test_gpu_parity.py:1642-1643 (real) and :1645-1647 (complex): assert_allclose with rtol = 1e-6
        if c.cplx:
            ref = _z(x) * 1j + np.arange(x.size // 2)
            np.testing.assert_allclose(_z(got), ref, rtol=1e-6)
        else:
            np.testing.assert_allclose(got, x * 2 + np.arange(x.size), rtol=1e-6)

    def call_aggregate(v, c):
        code, best = v.map_aggregate(lambda val, i: (abs(val), i), max)
        return code, [np.array(best if best is not None else (-1.0, -1), np.float64)]

    def chk_aggregate(c, x, got, extras):
        # tests/test_gpu_parity.py:1651-1652: the index of the largest magnitude, exactly (the callback sees every value
        # in T, the fold is Python's)
        mags = np.abs(_z(x)) if c.cplx else np.abs(x.astype(np.float64))
        assert int(extras[0][1]) == int(np.argmax(mags))
    return [Entry("map_inplace", lambda v, c: v.map_inplace((lambda val, i: val * 1j + i) if c.cplx else (lambda val, i: val * 2 + i)),
                  chk_inplace),
            Entry("map_aggregate", call_aggregate, chk_aggregate)]


# ---- reductions (tests/test_gpu_parity.py:1445: tol = 2e-5 / 1e-12) ---------------------------------------------------
def _stat_arrays(st):
    return {k: np.array(v, np.complex128 if isinstance(v, complex) else np.float64) for k, v in st.items()}


def e_reductions():
    def chk_stats(prec):
        def check(c, x, got, extras):
            st = extras[0]
            ref = (orc.complex_statistics if c.cplx else orc.real_statistics)(x.astype(np.float64))
            assert st["count"] == ref["count"]
            for key in ("min", "max", "min_index", "max_index"):   # tests/test_gpu_parity.py:1458-1459: equal
                assert st[key] == ref[key], key
            if prec:   # :1460-1461: the sum of statistics(prec) within 1e-9 max(1, |sum|), a thousand times that in f32
                assert abs(st["sum"] - ref["sum"]) <= 1e-9 * max(1.0, abs(ref["sum"])) * (1e3 if c.dtype == np.float32 else 1)
                return
            for key in ("sum", "average", "rms"):                  # :1456-1457: within 50 tol max(1, |ref|)
                assert abs(st[key] - ref[key]) <= 50 * _tol(c.dtype, 2e-5, 1e-12) * max(1.0, abs(ref[key])), key
        return check

    def chk_split(c, x, got, extras):
        # tests/test_gpu_parity.py:1469-1475: counts and indices equal, sums within 50 tol max(1, |ref|)
        for b in range(3):
            rb = (orc.complex_statistics if c.cplx else orc.real_statistics)(x.astype(np.float64), b, 3)
            pb = {k: v[b] for k, v in extras[0].items()}
            assert pb["count"] == rb["count"] and pb["max_index"] == rb["max_index"] and pb["min_index"] == rb["min_index"]
            assert abs(pb["sum"] - rb["sum"]) <= 50 * _tol(c.dtype, 2e-5, 1e-12) * max(1.0, abs(rb["sum"]))

    def chk_sum(squared):
        def check(c, x, got, extras):
            # tests/test_gpu_parity.py:1462-1464: sum within 50 tol max(1, |ref|), sum_sq within 50 tol |ref|
            ref = orc.vec_sum(x.astype(np.float64), c.cplx, squared)
            assert abs(complex(extras[0]) - ref) <= 50 * _tol(c.dtype, 2e-5, 1e-12) * (abs(ref) if squared else max(1.0, abs(ref)))
        return check

    def e_dot(prec):
        def call(v, c):
            code, d = v.dot_product(c.vec(1, None, -1, 1), prec=prec)
            return code, [np.array(d)]

        def check(c, x, got, extras):
            # tests/test_gpu_parity.py:1465-1468: within 50 tol max(1, |ref|), the operand from (-1, 1)
            ref = orc.dot(x.astype(np.float64), c.arrays[1].astype(np.float64), c.cplx)
            assert abs(complex(extras[0]) - ref) <= 50 * _tol(c.dtype, 2e-5, 1e-12) * max(1.0, abs(ref))
        return Entry("dot_product", call, check, label="dot_product" + ("(prec)" if prec else ""))

    def split(v, prec):
        code, parts = v.statistics_split(3, prec=prec)
        keys = parts[0].keys() if parts else ()
        return code, [{k: np.array([p[k] for p in parts]) for k in keys}]
    out = []
    for prec in (False, True):
        tag = "(prec)" if prec else ""
        out += [Entry("statistics", lambda v, c, prec=prec: (0, [_stat_arrays(v.statistics(prec=prec))]), chk_stats(prec), label="statistics" + tag),
                Entry("statistics_split", lambda v, c, prec=prec: split(v, prec), chk_split, label="statistics_split" + tag,
                      pre=lambda p: p >= 3),
                Entry("sum", lambda v, c, prec=prec: (0, [np.array(v.sum(prec=prec))]), chk_sum(False), label="sum" + tag),
                Entry("sum_sq", lambda v, c, prec=prec: (0, [np.array(v.sum_sq(prec=prec))]), chk_sum(True), label="sum_sq" + tag),
                e_dot(prec)]
    return out


def _catalogue():
    cat = e_elementwise()
    for op, name in enumerate(("add", "sub", "mul", "div")):
        cat += [e_binary(name, op), e_binary(name, op, True)]
    cat += [e_complex_to_real("magnitude", 0), e_complex_to_real("magnitude_squared", 1), e_complex_to_real("phase", 4),
            e_complex_to_real("get_magnitude", 0, True), e_complex_to_real("get_magnitude_squared", 1, True),
            e_complex_to_real("get_phase", 4, True)]
    cat += e_pairs() + e_windows()
    cat += [e_fft(n) for n in ("plain_fft", "fft", "windowed_fft", "plain_ifft", "ifft", "windowed_ifft")]
    # tests/test_gpu_parity.py:1033-1036: the callback window equals the built-in Hamming -- forward < 2e-6 / 1e-12, inverse
    # < 2e-5 / 1e-10; :1039-1040 the same for windowed_custom_sfft.  test_gpu_parity.py has no test of
    # windowed_custom_sifft: it is held to :1036, the bound of the other inverse pair (windowed_custom_ifft).
    cat += [e_custom_fft("windowed_custom_fft", "windowed_fft", 2e-6, 1e-12, "test_gpu_parity.py:1034", pre=lambda p: p != 1),
            e_custom_fft("windowed_custom_ifft", "windowed_ifft", 2e-5, 1e-10, "test_gpu_parity.py:1036", domain=FREQ, pre=lambda p: p != 1),
            e_custom_fft("windowed_custom_sfft", "windowed_sfft", 2e-6, 1e-12, "test_gpu_parity.py:1040", space="real",
                         pre=lambda p: p % 2 == 1 and p != 1),
            e_custom_fft("windowed_custom_sifft", "windowed_sifft", 2e-5, 1e-10, "test_gpu_parity.py:1036", space="complex", domain=FREQ,
                         prep=_real_spectrum, pre=lambda p: p >= 2)]
    cat += [e_sfft(n) for n in ("plain_sfft", "sfft", "windowed_sfft")] + [e_sifft(n) for n in ("plain_sifft", "sifft", "windowed_sifft")]
    cat += [e_convolve_signal(t) for t in (5, 300, 1024, 1026)]
    cat += [e_convolve(SINC, 0.0, 0.25, 12), e_convolve(RAISED_COSINE, 0.35, 0.25, 12), e_convolve(SINC, 0.0, 0.25, 12, "callable"),
            e_convolve(SINC, 0.0, 0.25, 12, "complex")]
    cat += e_frequency_responses() + e_correlation()
    cat += [e_interpolatef(RAISED_COSINE, 0.35, 4.0, 12), e_interpolatef(SINC, 0.0, 13.0 / 6.0, 8)]
    cat += [e_resample(("interpolatei", SINC, 0.0, 2)), e_resample(("interpolatei", RAISED_COSINE, 0.4, 3)),
            e_resample(("interpolate", SINC, 37, 0.0)), e_resample(("interpolate", SINC, 500, 0.3)),
            e_resample(("interpolate", SINC, -300, 0.0)), e_resample(("interpft", 37)), e_resample(("interpft", -300))]
    cat += e_custom_interpolation()
    cat += [e_interpolate_real("interpolate_lin", 2.5, 0.0), e_interpolate_real("interpolate_hermite", 3.0, 0.25)]
    cat += [e_math(n, None, False) for n in _MATH_DOMAINS] + [e_math(n, a, False) for n, (_, a) in _MATH_ARGS.items()]
    cat += [e_math(n, None, True) for n in _COMPLEX_MATH0] + [e_math(n, a, True) for n, a in _COMPLEX_MATH1]
    cat += e_scan() + e_maps() + e_reductions()
    return cat


CATALOGUE = _catalogue()
assert len({e.label for e in CATALOGUE}) == len(CATALOGUE)

# (state, the number space it is built in) of every dirty state
DIRTY_STATES = [(name, c) for name, d in vm.DIRTY.items() for c in ((False, True) if d["is_complex"] is None else (d["is_complex"],))]


def _to_space(v, space):
    """a state of the other number space than the entry's is brought over: two more movers in its history"""
    if space == "complex" and not v.is_complex():
        assert v.to_complex() == 0
    elif space == "real" and v.is_complex():
        assert v.to_real() == 0
    return v


def _build(api, name, cplx, dtype, entry, seed):
    fill = lambda n, k: _fill(n, seed + 53 * k, dtype, *entry.rng)
    return _to_space(vm.build_dirty(api, name, fill, cplx, entry.domain, DELTA), entry.space)


def model_state(name, cplx, dtype, entry, seed=0):
    """the dirty state an entry meets, on the model: the CPU test counts the (entry, state) pairs from it"""
    return _build(vm.ModelApi, name, cplx, dtype, entry, seed)


def applies(entry, w):
    return entry.pre is None or bool(entry.pre(w.points()))


def _run_entry(entry, v, ctx):
    res = entry.call(v, ctx)
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
    """the method on every dirty state it is defined on, and on a fresh vector of the same values and metadata: equal
    code, metadata and bits (for reductions: bit-equal results).  The comparison names the dirty state: an interpolatei
    that reserved for half its result, or a kernel that read a packet past the valid length into stale scalars, makes the
    dirty vector differ from its fresh copy here.  Then the fresh result against the oracle, once, on the first state with
    data that was built in the entry's number space."""
    api = _Api(bd)
    ran, checked = 0, False
    for k, (name, cplx) in enumerate(DIRTY_STATES):
        seed = 3000 + 17 * k
        w = model_state(name, cplx, dtype, entry, seed)
        if not applies(entry, w):
            continue
        d = _build(api, name, cplx, dtype, entry, seed)
        _same_state(d, w, (name, "the recipe's result"))   # the dirty content is known exactly, capacity included
        if entry.prep is not None:
            entry.prep(d)
        x = d.data()
        f = _vec(bd, x, d.is_complex(), d.domain(), d.delta())
        _same_state(f, d, (name, "fresh copy"))
        what = (entry.label, name, "complex" if cplx else "real")
        ctxs = [Ctx(bd, dtype, d.is_complex(), entry.domain, d.points(), seed, dirty) for dirty in (True, False)]
        code_d, extra_d = _run_entry(entry, d, ctxs[0])
        code_f, extra_f = _run_entry(entry, f, ctxs[1])
        assert code_d == code_f, (what, "codes", code_d, code_f)
        _same_state(d, f, what)
        _aligned(d, what)
        _same_extras(extra_d, extra_f, what)
        ran += 1
        # (the oracle's inputs are the test's own noise: a state that was brought over from the other number space has
        # zero imaginary parts, and tan or atanh on the real axis are not what the tolerances were set on)
        native = entry.space is None or (entry.space == "complex") == cplx
        if not checked and x.size and native:
            assert code_f in (0, 9), (what, code_f)   # (9: the getters' convert_void)
            with np.errstate(all="ignore"):
                entry.check(ctxs[1], x, f.data(), extra_f)
            checked = True
    assert ran >= 2 and checked, (entry.label, ran, checked)


# ============================================================================================== part 5: errors, poisoning
def _other_dot(v, other):
    """dot_product through the C entry point of the OTHER number space: DspVec.dot_product picks the entry point by
    is_complex(), so the codes 4 (must be real) and 3 (must be complex) of its docstring exist at this level only"""
    return v._fn(("real" if v.is_complex() else "complex") + "_dot_product")(v._h, other._h).result_code


def _arg_errors():
    """(method, label, space, bad call -> code, the documented code (or cplx -> code)): every rejection that capi.cpp makes
    on the host before any launch and that leaves the vector alone -- op_binary (1, 2), op_binary_smaller (7, 2),
    op_zero_pad (7), op_decimatei (7), op_convolve_signal (2, 5, 7), op_set_pair (7), op_interpolate (7), op_split_into
    (7, 13), op_merge (7, 13), stats_split (7), dot (2, 4, 3), op_map_aggregate (3 / 4 through the other entry point is not
    reachable from the wrapper), overwrite_data (7), op_correlate's zero_pad (7), set_len of a complex vector to an odd
    length (ignored)."""
    t = [
        ("zero_pad", "to the current length", None, lambda v, c: v.zero_pad(v.points()), 7),
        ("zero_pad", "to fewer points", None, lambda v, c: v.zero_pad(v.points() - 1, PAD_SURROUND), 7),
        ("decimatei", "by 0", None, lambda v, c: v.decimatei(0, 0), 7),
        ("overwrite_data", "more scalars than the vector has", None, lambda v, c: v.overwrite_data(np.zeros(v.len() + 2, c.dtype)), 7),
        ("set_len", "odd length of a complex vector", "complex", lambda v, c: _Api(c.bd).set_len(v, v.len() - 1), None),
        ("convolve_signal", "filter longer than the vector", None, lambda v, c: v.convolve_signal(c.vec(1, c.points + 1)), 7),
        ("convolve_signal", "other number space", None, lambda v, c: v.convolve_signal(c.vec(1, 6, cplx=not c.cplx)), 2),
        ("convolve_signal", "filter of the other domain", None, lambda v, c: v.convolve_signal(c.vec(1, 6, domain=FREQ)), 2),
        ("set_real_imag", "unequal parts", "complex", lambda v, c: v.set_real_imag(c.vec(1, cplx=False), c.vec(2, c.points - 1, cplx=False)), 7),
        ("set_mag_phase", "unequal parts", "complex", lambda v, c: v.set_mag_phase(c.vec(1, None, 0, 10, cplx=False), c.vec(2, c.points - 1, cplx=False)), 7),
        ("interpolate", "to 0 points", None, lambda v, c: v.interpolate(SINC, 0), 7),
        ("interpft", "to 0 points", None, lambda v, c: v.interpft(0), 7),
        ("interpolate_custom", "to 0 points", None, lambda v, c: v.interpolate_custom(lambda t: 1.0, 0), 7),
        ("split_into", "no targets", None, lambda v, c: v.split_into([]), 7),
        ("split_into", "a count that does not divide", None, lambda v, c: v.split_into([c.small() for _ in range(_non_divisor(v.len()))]), 7),
        ("merge", "no sources", None, lambda v, c: v.merge([]), 7),
        ("merge", "sources of unequal lengths", None, lambda v, c: v.merge([c.vec(1, 4), c.vec(2, 6)]), 7),
        ("merge", "an odd scalar count into a complex vector", "complex", lambda v, c: v.merge([c.vec(1, 3, cplx=False)]), 13),
        ("statistics_split", "more than 16 parts", None, lambda v, c: v.statistics_split(17)[0], 7),
        ("correlate", "argument not longer than the vector", "complex", lambda v, c: v.correlate(_prepared(c.vec(1))), 7),
        ("dot_product", "complex vector, real operand", "complex", lambda v, c: v.dot_product(c.vec(1, cplx=False))[0], 2),
        ("dot_product", "complex vector, operand of the other domain", "complex", lambda v, c: v.dot_product(c.vec(1, domain=FREQ))[0], 2),
        ("dot_product", "entry point of the other number space", None, lambda v, c: _other_dot(v, c.vec(1)), lambda cplx: 4 if cplx else 3),
    ]
    for name in ("add", "sub", "mul", "div"):   # tests/test_gpu_parity.py:82-91: 1 lengths, 2 metadata
        t += [(name, "operand of another length", None, lambda v, c, name=name: getattr(v, name)(c.vec(1, c.points - 1)), 1),
              (name, "operand of the other domain", None, lambda v, c, name=name: getattr(v, name)(c.vec(1, domain=FREQ)), 2)]
        sm = name + "_smaller"
        t += [(sm, "operand whose length does not divide", None, lambda v, c, sm=sm: getattr(v, sm)(c.vec(1, _non_divisor(c.points))), 7),
              (sm, "empty operand", None, lambda v, c, sm=sm: getattr(v, sm)(c.vec(1, 0)), 7),
              (sm, "operand of the other domain", None, lambda v, c, sm=sm: getattr(v, sm)(c.vec(1, c.divisor(), domain=FREQ)), 2)]
    return t


def _non_divisor(n):
    return next(d for d in range(2, n + 2) if n % d)


def _prepared(arg):
    assert arg.prepare_argument() == 0
    return arg


ARG_ERRORS = _arg_errors()
# the states with stale scalars behind the valid length, traded buffers, no slack, a reallocation
ERR_STATES = [(n, c) for (n, c) in DIRTY_STATES if n in ("shrunk-even", "odd-trades-odd", "exact-fit-real", "exact-fit-complex", "regrown")]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_argument_errors_leave_a_dirty_vector_as_it_was(bd, dtype):
    api = _Api(bd)
    entry = Entry("none", None)
    for k, (name, cplx) in enumerate(ERR_STATES):
        for j, (method, label, space, bad, code) in enumerate(ARG_ERRORS):
            if space is not None and (space == "complex") != cplx:
                continue
            seed = 5000 + 31 * k + j
            d, w = _build(api, name, cplx, dtype, entry, seed), model_state(name, cplx, dtype, entry, seed)
            what = (method, label, name, "complex" if cplx else "real")
            ctx = Ctx(bd, dtype, cplx, TIME, d.points(), seed, True)
            assert bad(d, ctx) == (code(cplx) if callable(code) else code), what
            _same_state(d, w, (what, "after the refused call"))   # bits, metadata, delta, capacity as the model left them
            _aligned(d, what)
            f = _vec(bd, w.data(), cplx, TIME, DELTA)
            assert d.scale(2.0) == 0 and f.scale(2.0) == 0        # and it goes on working as a fresh one does
            _same_state(d, f, (what, "after the good call"))


def _poisoners():
    """(method, label, is_complex, domain, call, the code, odd length?): every call that capi.cpp answers by poisoning the
    vector before any launch.  -1 is the facade's code for a poisoned vector; 5 / 6 / 9 / 8 are the symmetric transforms'
    and correlate's own (op_sfft, op_sifft, op_correlate)."""
    p = [("conj", "real vector", False, TIME, lambda v, c: v.conj(), -1),
         ("scale", "complex factor, real vector", False, TIME, lambda v, c: v.scale(complex(1, 2)), -1),
         ("offset", "complex value, real vector", False, TIME, lambda v, c: v.offset(complex(1, 2)), -1),
         ("complex_divide", "real vector", False, TIME, lambda v, c: v.complex_divide(1 + 2j), -1),
         ("to_complex", "complex vector", True, TIME, lambda v, c: v.to_complex(), -1),
         ("mirror", "real time-domain vector", False, TIME, lambda v, c: v.mirror(), -1),
         ("unwrap", "complex vector", True, TIME, lambda v, c: v.unwrap(7.0), -1),
         ("multiply_complex_exponential", "real vector", False, TIME, lambda v, c: v.multiply_complex_exponential(0.02, 0.3), -1),
         ("multiply_frequency_response", "time domain", True, TIME, lambda v, c: v.multiply_frequency_response(SINC, 0.5), -1),
         ("multiply_frequency_response_fn", "time domain", True, TIME, lambda v, c: v.multiply_frequency_response_fn(lambda t: 1.0, 0.5), -1),
         ("multiply_frequency_response_complex", "time domain", True, TIME, lambda v, c: v.multiply_frequency_response_complex(lambda t: 1j, 0.5), -1),
         ("multiply_frequency_response_complex", "real vector", False, FREQ, lambda v, c: v.multiply_frequency_response_complex(lambda t: 1j, 0.5), -1),
         ("correlate", "real vector", False, TIME, lambda v, c: v.correlate(c.vec(1, cplx=True, domain=FREQ)), 5),
         ("correlate", "unprepared argument", True, TIME, lambda v, c: v.correlate(c.vec(1)), 5),
         ("convolve", "frequency domain", True, FREQ, lambda v, c: v.convolve(SINC, 0.25, 12), -1),
         ("convolve_complex", "real vector", False, TIME, lambda v, c: v.convolve_complex(lambda t: 1j, 0.25, 3), -1),
         ("interpolate_lin", "complex vector", True, TIME, lambda v, c: v.interpolate_lin(2.0), -1),
         ("interpolate_hermite", "complex vector", True, TIME, lambda v, c: v.interpolate_hermite(2.0), -1),
         ("windowed_custom_fft", "frequency domain", True, FREQ, lambda v, c: v.windowed_custom_fft(_ham_cb), -1),
         ("windowed_custom_ifft", "time domain", True, TIME, lambda v, c: v.windowed_custom_ifft(_ham_cb), -1),
         ("windowed_custom_sfft", "complex vector", True, TIME, lambda v, c: v.windowed_custom_sfft(_ham_cb), 5),
         ("windowed_custom_sfft", "even length", False, TIME, lambda v, c: v.windowed_custom_sfft(_ham_cb), 9, False),
         ("windowed_custom_sifft", "time domain", True, TIME, lambda v, c: v.windowed_custom_sifft(_ham_cb), 6)]
    for name in ("abs", "ln_approx", "exp_approx", "sin_approx", "cos_approx"):
        p.append((name, "complex vector", True, TIME, lambda v, c, name=name: getattr(v, name)(), -1))
    for name in ("wrap", "log_approx", "expf_approx", "powf_approx"):
        p.append((name, "complex vector", True, TIME, lambda v, c, name=name: getattr(v, name)(2.0), -1))
    for name in ("plain_sfft", "sfft", "windowed_sfft"):
        call = lambda v, c, name=name: getattr(v, name)(*((HAMMING,) if "windowed" in name else ()))
        p += [(name, "complex vector", True, TIME, call, 5), (name, "frequency domain", False, FREQ, call, 5),
              (name, "even length", False, TIME, call, 9, False)]
    for name in ("plain_sifft", "sifft", "windowed_sifft"):
        call = lambda v, c, name=name: getattr(v, name)(*((HAMMING,) if "windowed" in name else ()))
        p += [(name, "time domain", True, TIME, call, 6), (name, "real vector", False, FREQ, call, 6)]
    # (the first-bin rule of plain_sifft reads four scalars back and rejects on the host; sifft and windowed_sifft scale and
    # shift on the device first, so their code 8 is no host-side rejection and stays with test_gpu_parity.py:919-922)
    p.append(("plain_sifft", "first bin not real", True, FREQ, lambda v, c: (v.set_value(1, 5.0), v.plain_sifft())[1], 8))
    for name in ("magnitude", "magnitude_squared", "to_real", "to_imag", "phase"):
        p.append((name, "real vector", False, TIME, lambda v, c, name=name: getattr(v, name)(), -1))
    for name, domain in (("plain_fft", FREQ), ("fft", FREQ), ("windowed_fft", FREQ), ("plain_ifft", TIME), ("ifft", TIME), ("windowed_ifft", TIME)):
        args = (HAMMING,) if "windowed" in name else ()
        p.append((name, "wrong domain", True, domain, lambda v, c, name=name, args=args: getattr(v, name)(*args), -1))
    return p


POISONERS = _poisoners()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_poisoning_calls_poison_a_dirty_vector_as_documented(bd, dtype):
    """on the regrown state (reallocated once, traded twice; 2001 points, or 2000 where the call needs an even length): the
    documented code, then length 0 and a NaN delta in an allocation that stays what it was, and -1 to every later call"""
    api = _Api(bd)
    for j, row in enumerate(POISONERS):
        method, label, cplx, domain, call, code = row[:6]
        state = "regrown-odd" if len(row) == 6 or row[6] else "regrown"
        entry = Entry("none", None, domain=domain)
        d, w = _build(api, state, cplx, dtype, entry, 6000 + j), model_state(state, cplx, dtype, entry, 6000 + j)
        _same_state(d, w, (method, label, "the recipe's result"))
        cap = d.allocated_len()
        ctx = Ctx(bd, dtype, cplx, domain, d.points(), 6000 + j, True)
        assert call(d, ctx) == code, (method, label)
        poisoned = lambda: d.len() == 0 and d.points() == 0 and np.isnan(d.delta()) and d.is_erroneous() and d.data().size == 0 \
            and d.allocated_len() == cap
        assert poisoned(), (method, label)
        _aligned(d, (method, label))
        for other in (lambda: d.scale(2.0), d.swap_halves, d.reverse, lambda: d.zero_interleave(3), lambda: d.decimatei(2, 0),
                      lambda: d.apply_window(HAMMING), d.cum_sum, d.sqrt):
            assert other() == -1 and poisoned(), (method, label)   # unrelated calls: -1, still poisoned


# ============================================================================================== part 6: a long-lived process
# One measured run on an MI355X, wall time of the child with its start-up: walk 2.4 s, evict 6.4 s.  The limit is ten times
# that plus a minute: the interpreter's and the runtime's start-up on a loaded host varies more than the work does.
WALK_MEASURED_S, EVICT_MEASURED_S = 2.4, 6.4


@pytest.mark.parametrize("scenario,measured", (("walk", WALK_MEASURED_S), ("evict", EVICT_MEASURED_S)), ids=("walk", "evict"))
def test_a_process_that_has_lived_long(scenario, measured):
    """tests/vec_long_process.py in a child of its own: `walk` requests every twiddle table the library can form (816 from
    the mixed-radix lengths; the module's docstring derives the count and why it stays below the 1024 at which admission
    would close) and runs six probe lengths before and after, bit-equal; `evict` runs four Bluestein lengths just above
    2^22 points forward and back -- eight plans of 160 MiB against the 1 GiB cache, the smallest shapes that evict --
    and the first length again, bit-equal.  Every result is held to numpy / the DFT sum in float64 inside the child."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "vec_long_process.py"), scenario], capture_output=True, text=True,
                       timeout=60 + 10 * measured)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("ok " + scenario), (scenario, r.returncode)
