"""zoom_fft: the chirp-z transform of a frequency band of a DspVec and of every row of a DspMat, through the C ABI.

    X[k] = sum_{n<N} x[n] exp(-2 pi i (start + k step) n),   k = 0 .. bins-1

Nothing of it is in the reference, so the model is numpy and the definition itself: the phases are formed in
np.longdouble (63 mantissa bits at least) and reduced modulo 1 before the cast to float64, the sum is taken in
complex128.  (start + k step) n = start n + k step n: the model forms the two products in longdouble, reduces each modulo
1, and multiplies the two unit phasors -- one rounding of 1e-16 more than a single table of phases, and the k step n table
is shared by all rows, row counts, starts and precisions of a shape.  |start| <= 1 everywhere, where the model is exact
to 1e-15 (with start = 1e6 + 0.1234 it would itself be good to 1e-10 only).

Inputs are seeded white noise plus a tone inside the band.  Tolerance per row: rel-L2 1e-6 (f32), 1e-12 (f64) -- the
project's figures for every transform, Bluestein lengths included; a numpy emulation of the arithmetic
gave 1.3-1.5e-7 and 7-9e-16 on these shapes, the host simulation (tests/host_sim/sim_zoom_fft.cpp) 0.5-2.0e-7 and
1-8e-16.  Every row and every bin is compared.

Shapes (N -> bins): 1 -> 1, 2 -> 3, 100 -> 37, 300 -> 213 (L exactly 512), 300 -> 214 (L = 1024), 1000 -> 64 at step
1/16000, 1001 -> 501 (odd real rows: rows that do not start on 16 bytes), 2048 -> 2049 (L exactly 4096, the last fused
size), 2049 -> 2049 (general path, L = 8192), 5000 -> 100, 100 -> 5000 (bins > N; the call grows the buffers); each in f32
and f64, complex and real rows, with 1, 3, 17 and one more row than a workgroup of the fused kernel holds."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME, FREQ = 0, 1
UNSUPPORTED = -102
TOL = {np.float32: 1e-6, np.float64: 1e-12}
VARIANTS = [(np.float32, True), (np.float32, False), (np.float64, True), (np.float64, False)]
VARIANT_IDS = ["f32-complex", "f32-real", "f64-complex", "f64-real"]

# (N, bins, start, step); the second and third use dyadic start and step (denominators <= 2^20): their phases are exact
# in plain float64 as well
SHAPES = [
    (1, 1, 0.25, 0.125),
    (2, 3, -5.0 / 8.0, 3.0 / 1024.0),
    (100, 37, 3.0 / 16.0, 5.0 / 4096.0),
    (300, 213, 0.1234, 1.0 / 1700.0),
    (300, 214, -0.98, 1.0 / 1300.0),
    (1000, 64, 0.3, 1.0 / 16000.0),
    (1001, 501, -0.41, 1.0 / 2003.0),
    (2048, 2049, 0.77, 1.0 / 4099.0),
    (2049, 2049, -0.2, 1.0 / 4099.0),
    (5000, 100, 0.05, 1.0 / 80000.0),
    (100, 5000, 1.0, 1.0 / 5000.0),
]
SHAPE_IDS = ["%d-%d" % (s[0], s[1]) for s in SHAPES]


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    assert np.finfo(np.longdouble).nmant >= 63
    return b


def conv_len(n, bins):
    l = 512
    while l < n + bins - 1:
        l *= 2
    return l


def row_counts(n, bins):
    l = conv_len(n, bins)
    per_wg = 256 // (l // 16) if l <= 4096 else 1
    return sorted({1, 3, per_wg + 1, 17})


def frac_phasor(f, n):
    """exp(-2 pi i frac(f n)) for the float64 array f and n = 0 .. n-1: product and reduction in longdouble"""
    p = np.multiply.outer(np.asarray(f, dtype=np.longdouble), np.arange(n, dtype=np.longdouble))
    p = np.fmod(p, np.longdouble(1)).astype(np.float64)
    return np.exp(-2j * np.pi * p)


@functools.lru_cache(maxsize=8)
def band_matrix(n, bins, step):
    """E[k, n] = exp(-2 pi i frac(k step n)): shared by every row, start and precision of a shape; read only"""
    k = np.arange(bins, dtype=np.longdouble) * np.longdouble(step)
    p = np.fmod(np.multiply.outer(k, np.arange(n, dtype=np.longdouble)), np.longdouble(1)).astype(np.float64)
    e = np.exp(-2j * np.pi * p)
    e.setflags(write=False)
    return e


def model(x, cplx, starts, step, bins):
    """rows of x (float array [rows, N or 2N]) -> complex128 [rows, bins]; starts: one per row"""
    z = x.astype(np.float64)
    z = z[:, 0::2] + 1j * z[:, 1::2] if cplx else z.astype(np.complex128)
    n = z.shape[1]
    w = frac_phasor(np.asarray(starts, dtype=np.float64), n)  # [rows, n]
    return (z * w) @ band_matrix(n, bins, float(step)).T


def make_rows(rows, n, cplx, dtype, seed, tone):
    """seeded white noise, plus a tone at `tone` cycles per sample (inside the band) unless tone is None"""
    rng = np.random.default_rng(seed)
    t, amp = np.arange(n), 0.0 if tone is None else 2.0
    tone = tone or 0.0
    if cplx:
        z = rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)) + amp * np.exp(2j * np.pi * tone * t)
        out = np.empty((rows, 2 * n))
        out[:, 0::2], out[:, 1::2] = z.real, z.imag
    else:
        out = rng.standard_normal((rows, n)) + amp * np.cos(2 * np.pi * tone * t)
    return np.ascontiguousarray(out.astype(dtype))


def as_complex(data, rows):
    d = np.asarray(data, dtype=np.float64).reshape(rows, -1)
    return d[:, 0::2] + 1j * d[:, 1::2]


def row_errors(got, ref):
    return np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check_rows(label, got, ref, dtype):
    err = row_errors(got, ref)
    print("%s: rel-L2 per row max %.3e (row %d)" % (label, err.max(), int(err.argmax())))
    assert got.shape == ref.shape
    assert np.all(err <= TOL[dtype]), (label, err.max(), int(err.argmax()))


# ---------------------------------------------------------------------------------------------- against the model
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_one_start_for_all_rows_against_the_definition(bd, shape, dtype, cplx):
    n, bins, start, step = shape
    tone = start + (bins // 2) * step
    for rows in row_counts(n, bins):
        x = make_rows(rows, n, cplx, dtype, 1000 + rows, tone)
        ref = model(x, cplx, [start] * rows, step, bins)
        m = bd.DspMat(x, is_complex=cplx, dtype=dtype, delta=0.5)
        assert bd.zoom_fft(m, start, step, bins) == 0
        assert (m.rows(), m.row_points(), m.is_complex(), m.domain()) == (rows, bins, True, FREQ)
        assert m.delta() == dtype(step / 0.5)
        check_rows("%d -> %d, %d rows" % (n, bins, rows), as_complex(m.data(), rows), ref, dtype)
        if rows == 1:  # the vector entry point on the same row
            v = bd.DspVec(x[0], is_complex=cplx, delta=0.5)
            assert bd.zoom_fft(v, start, step, bins) == 0
            assert (v.points(), v.is_complex(), v.domain()) == (bins, True, FREQ) and v.delta() == dtype(step / 0.5)
            check_rows("%d -> %d, vector" % (n, bins), as_complex(v.data(), 1), ref, dtype)


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_one_start_per_row_against_the_definition(bd, shape, dtype, cplx):
    n, bins, _, step = shape
    for rows in (3, 17):
        starts = np.linspace(-1.0, 1.0, rows)  # spread over [-1, 1], both ends included
        x = make_rows(rows, n, cplx, dtype, 2000 + rows, None)
        t = np.arange(n)
        for r in range(rows):  # every row's tone inside its own band
            f = starts[r] + (bins // 2) * step
            if cplx:
                x[r, 0::2] += (2.0 * np.cos(2 * np.pi * f * t)).astype(dtype)
                x[r, 1::2] += (2.0 * np.sin(2 * np.pi * f * t)).astype(dtype)
            else:
                x[r] += (2.0 * np.cos(2 * np.pi * f * t)).astype(dtype)
        ref = model(x, cplx, starts, step, bins)
        m = bd.DspMat(x, is_complex=cplx, dtype=dtype)
        assert bd.zoom_fft(m, starts, step, bins) == 0
        assert (m.rows(), m.row_points(), m.is_complex(), m.domain()) == (rows, bins, True, FREQ)
        check_rows("%d -> %d, %d rows, per-row starts" % (n, bins, rows), as_complex(m.data(), rows), ref, dtype)


@pytest.mark.parametrize("dtype,cplx", [(np.float32, True), (np.float64, False)], ids=["f32-complex", "f64-real"])
def test_more_rows_than_a_grid_dimension_holds(bd, dtype, cplx):
    rows, n, bins, start, step = 70000, 3, 5, -0.3, 0.11
    x = make_rows(rows, n, cplx, dtype, 7, start + 2 * step)
    m = bd.DspMat(x, is_complex=cplx, dtype=dtype)
    assert bd.zoom_fft(m, start, step, bins) == 0
    check_rows("70000 rows, 3 -> 5", as_complex(m.data(), rows), model(x, cplx, [start] * rows, step, bins), dtype)
    starts = np.linspace(-1.0, 1.0, rows)
    m = bd.DspMat(x, is_complex=cplx, dtype=dtype)
    assert bd.zoom_fft(m, starts, step, bins) == 0
    check_rows("70000 rows, 3 -> 5, per-row starts", as_complex(m.data(), rows), model(x, cplx, starts, step, bins), dtype)


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("step", [0.0, -1.0 / 700.0], ids=["step0", "negative"])
def test_zero_and_negative_step(bd, step, dtype, cplx):
    n, bins, start, rows = 100, 37, 0.21, 3
    x = make_rows(rows, n, cplx, dtype, 11, start + 18 * step)
    m = bd.DspMat(x, is_complex=cplx, dtype=dtype)
    assert bd.zoom_fft(m, start, step, bins) == 0
    assert m.delta() == dtype(step / 1.0)
    got = as_complex(m.data(), rows)
    check_rows("100 -> 37, step %g" % step, got, model(x, cplx, [start] * rows, step, bins), dtype)
    if step == 0.0:  # every bin is the same sum, computed by the same arithmetic or not: the model decides, not equality
        assert np.all(row_errors(got[:, 1:], got[:, :1].repeat(bins - 1, axis=1)) <= 2 * TOL[dtype])


# ---------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(100, 37), (300, 214), (2048, 2049), (2049, 2049), (5000, 100)],
                         ids=["100-37", "300-214", "2048-2049", "2049-2049", "5000-100"])
def test_a_row_of_the_matrix_call_is_the_vector_call_on_it_and_calls_repeat_bit_for_bit(bd, shape, dtype):
    n, bins = shape
    start, step = 0.31, 1.0 / (3.0 * bins)
    for cplx, rows in ((True, 3), (False, row_counts(n, bins)[-2])):
        x = make_rows(rows, n, cplx, dtype, 21, start)
        m = bd.DspMat(x, is_complex=cplx, dtype=dtype)
        assert bd.zoom_fft(m, start, step, bins) == 0
        got = m.data().reshape(rows, 2 * bins)
        for r in sorted({0, rows // 2, rows - 1}):
            v = bd.DspVec(x[r], is_complex=cplx)
            assert bd.zoom_fft(v, start, step, bins) == 0
            assert np.array_equal(bits(v.data()), bits(got[r])), (cplx, r)
        again = bd.DspMat(x, is_complex=cplx, dtype=dtype)  # determinism: a fresh copy, the same bytes
        assert bd.zoom_fft(again, start, step, bins) == 0
        assert np.array_equal(bits(again.data()), bits(m.data()))
        starts = np.linspace(-1.0, 1.0, rows)
        a, b = bd.DspMat(x, is_complex=cplx, dtype=dtype), bd.DspMat(x, is_complex=cplx, dtype=dtype)
        assert bd.zoom_fft(a, starts, step, bins) == 0 and bd.zoom_fft(b, starts, step, bins) == 0
        assert np.array_equal(bits(a.data()), bits(b.data()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1000, 2048])
def test_the_whole_circle_is_plain_fft(bd, n, dtype):
    x = make_rows(3, n, True, dtype, 31, 0.1)
    m, f = bd.DspMat(x, is_complex=True, dtype=dtype), bd.DspMat(x, is_complex=True, dtype=dtype)
    assert bd.zoom_fft(m, 0.0, 1.0 / n, n) == 0 and f.plain_fft() == 0
    err = row_errors(as_complex(m.data(), 3), as_complex(f.data(), 3))
    print("identity %d: %.3e" % (n, err.max()))
    assert np.all(err <= 2 * TOL[dtype])
    assert (m.row_points(), m.domain(), m.is_complex()) == (f.row_points(), f.domain(), f.is_complex())


# ---------------------------------------------------------------------------------------------- codes and metadata
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_codes_and_metadata(bd, dtype):
    sfx = "32" if dtype == np.float32 else "64"
    lib = bd.lib
    vec_fn, mat_fn, starts_fn = (getattr(lib, n + sfx) for n in
                                 ("bdsp_hip_zoom_fft", "bdsp_hip_mat_zoom_fft", "bdsp_hip_mat_zoom_fft_starts"))
    x = make_rows(3, 100, True, dtype, 41, 0.1)

    def untouched(m):
        return ((m.rows(), m.row_points(), m.is_complex(), m.domain(), m.delta()) == (3, 100, True, TIME, dtype(0.25))
                and np.array_equal(bits(m.data()), bits(x)))

    # argument errors come first and leave the data alone: 7
    m = bd.DspMat(x, is_complex=True, dtype=dtype, delta=0.25)
    v = bd.DspVec(x[0], is_complex=True, delta=0.25)
    for start, step, bins in ((0.1, 0.01, 0), (np.nan, 0.01, 8), (np.inf, 0.01, 8), (0.1, np.nan, 8), (0.1, -np.inf, 8)):
        assert bd.zoom_fft(m, start, step, bins) == 7 and bd.zoom_fft(v, start, step, bins) == 7
    assert bd.zoom_fft(m, [0.1, 0.2], 0.01, 8) == 7 and bd.zoom_fft(m, [0.1, 0.2, 0.3, 0.4], 0.01, 8) == 7   # count != rows
    assert bd.zoom_fft(m, [0.1, np.nan, 0.3], 0.01, 8) == 7 and bd.zoom_fft(m, [0.1, 0.2, 0.3], 0.01, 0) == 7
    assert starts_fn(m._h, None, 3, 0.01, 8) == 7                                                            # null starts
    assert untouched(m) and np.array_equal(bits(v.data()), bits(x[0])) and v.domain() == TIME
    # ... also on a frequency-domain or poisoned input: the argument error is answered before the state is looked at
    fm = bd.DspMat(x, is_complex=True, dtype=dtype, domain=FREQ)
    assert bd.zoom_fft(fm, 0.1, 0.01, 0) == 7 and bd.zoom_fft(fm, [0.1], 0.01, 8) == 7
    # frequency-domain input: 5, untouched
    assert bd.zoom_fft(fm, 0.1, 0.01, 8) == 5 and bd.zoom_fft(fm, [0.1, 0.2, 0.3], 0.01, 8) == 5
    assert fm.domain() == FREQ and fm.row_points() == 100 and np.array_equal(bits(fm.data()), bits(x))
    fv = bd.DspVec(x[0], is_complex=True, domain=FREQ)
    assert bd.zoom_fft(fv, 0.1, 0.01, 8) == 5 and np.array_equal(bits(fv.data()), bits(x[0]))
    # a poisoned matrix: -1; a poisoned vector: what plain_fft answers on one
    pm = bd.DspMat(x, is_complex=True, dtype=dtype)
    assert pm.plain_ifft() == -1   # the inverse transform of time-domain rows poisons them
    assert bd.zoom_fft(pm, 0.1, 0.01, 8) == -1 and bd.zoom_fft(pm, [0.1, 0.2, 0.3], 0.01, 8) == -1
    assert pm.plain_fft() == -1 and pm.row_points() == 0
    pv, pw = bd.DspVec(x[0], is_complex=True), bd.DspVec(x[0], is_complex=True)
    assert pv.plain_ifft() == -1 and pw.plain_ifft() == -1
    assert bd.zoom_fft(pv, 0.1, 0.01, 8) == pw.plain_fft() == -1
    # rows * bins beyond the address space, and a convolution length above 2^30: BDSP_ERR_UNSUPPORTED, nothing touched
    assert mat_fn(m._h, 0.1, 0.01, 1 << 61) == UNSUPPORTED and "address space" in bd.last_error()
    assert starts_fn(m._h, (C.c_double * 3)(0.1, 0.2, 0.3), 3, 0.01, 1 << 61) == UNSUPPORTED
    assert vec_fn(v._h, 0.1, 0.01, 1 << 30) == UNSUPPORTED and "2^30" in bd.last_error()
    assert untouched(m) and np.array_equal(bits(v.data()), bits(x[0]))
    # no rows, and rows of no points: as plain_fft leaves them
    for rows, row_len in ((0, 8), (3, 0)):
        a = bd.DspMat(rows=rows, row_len=row_len, is_complex=True, dtype=dtype)
        b = bd.DspMat(rows=rows, row_len=row_len, is_complex=True, dtype=dtype)
        assert bd.zoom_fft(a, 0.1, 0.01, 8) == b.plain_fft() == 0
        assert (a.rows(), a.row_len(), a.is_complex(), a.domain()) == (b.rows(), b.row_len(), b.is_complex(), b.domain())
        c = bd.DspMat(rows=rows, row_len=row_len, is_complex=True, dtype=dtype)
        assert bd.zoom_fft(c, [0.1] * rows, 0.01, 8) == 0 and (c.rows(), c.row_len(), c.domain()) == (a.rows(), a.row_len(), a.domain())
    e, f = bd.DspVec(np.zeros(0, dtype=dtype), is_complex=True), bd.DspVec(np.zeros(0, dtype=dtype), is_complex=True)
    assert bd.zoom_fft(e, 0.1, 0.01, 8) == f.plain_fft() and (e.points(), e.domain()) == (f.points(), f.domain())
    # a good call on real rows: complex, frequency domain, bins points, delta = step / delta_before; the call needed more
    # capacity than the matrix had (100 real -> 5000 complex per row) and every row is right
    xr = make_rows(3, 100, False, dtype, 43, 0.2)
    g = bd.DspMat(xr, dtype=dtype, delta=0.25)
    assert bd.zoom_fft(g, 0.2, 1.0 / 5000.0, 5000) == 0
    assert (g.rows(), g.row_points(), g.row_len(), g.is_complex(), g.domain()) == (3, 5000, 10000, True, FREQ)
    assert g.delta() == dtype((1.0 / 5000.0) / float(dtype(0.25)))
    check_rows("100 -> 5000 real, grown", as_complex(g.data(), 3), model(xr, False, [0.2] * 3, 1.0 / 5000.0, 5000), dtype)
    # the result is in the frequency domain: a second call answers 5
    assert bd.zoom_fft(g, 0.2, 0.001, 10) == 5


# ---------------------------------------------------------------------------------------------- graph capture
def test_graph_capture_replays_the_same_bits_once_the_plan_is_warm(bd):
    """zoom_fft writes into the trade buffer, so a sequence a graph may hold needs a second trade (swap_halves here); with
    64 -> 64 bins the inverse transform in between brings the vector back to the time domain, and the sequence can run
    again on its own result.  The capture of a cold plan answers BDSP_ERR_UNSUPPORTED with bs_plan's message."""
    x = make_rows(1, 64, True, np.float32, 51, 0.1)[0] / np.float32(8)
    v, w = bd.DspVec(x, is_complex=True), bd.DspVec(x, is_complex=True)

    def seq(u):
        return lambda: (bd._lib.check(bd.zoom_fft(u, 0.0, 1.0 / 64, 64)), bd._lib.check(u.plain_ifft()),
                        bd._lib.check(u.swap_halves()))
    g = bd.Graph.capture(seq(v))       # one warm-up run (the plan is built there), then the capture, which runs nothing
    g.launch()
    g.launch()
    for _ in range(3):
        assert seq(w)() == (0, 0, 0)
    assert v.points() == w.points() == 64
    assert np.array_equal(bits(v.data()), bits(w.data()))
    assert np.all(np.isfinite(v.data())) and np.any(v.data() != 0)
    cold = bd.DspVec(x, is_complex=True)
    with pytest.raises(bd.BackendError, match="warm the plan"):
        bd.Graph.capture(lambda: bd._lib.check(bd.zoom_fft(cold, 0.123, 1.0 / 77, 64)), warmup=False)
    assert cold.domain() == TIME and np.array_equal(bits(cold.data()), bits(x))   # refused before anything was touched
    assert bd.zoom_fft(cold, 0.123, 1.0 / 77, 64) == 0                            # and the library is usable
    del g


# ---------------------------------------------------------------------------------------------- the README's snippet
@pytest.mark.parametrize("f", [200.3, 77.81])
def test_readme_zoom_snippet(bd, f):
    """The README's snippet as written: a tone f bins (not a whole number) into a 1024-point frame, coarse windowed_fft ->
    the strongest bin of every row -> zoom_fft of the original frames, every row around its own peak, two coarse bins
    wide in 64 steps.  The spectrum of a real signal has the tone at -f and at +f; whichever of the two a row's coarse
    peak picked, the estimate is that frequency to within a tenth of a coarse bin (the zoom's own grid is 1/32 bin)."""
    with open(os.path.join(ROOT, "README.md")) as fh:
        text = fh.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "zoom_fft(" in b]
    assert len(blocks) == 1
    code = blocks[0]
    assert "windowed_fft(V.WINDOW_HANN) == 0" in code and 'statistics()["max_index"]' in code
    assert "(peak - 1 - N // 2) / N" in code and "2 / (N * bins)" in code
    env = {"np": np, "f": f, "DspVec": bd.DspVec, "DspMat": bd.DspMat, "V": bd.vector}
    exec(code, env)
    tone = np.asarray(env["tone"], dtype=np.float64)
    assert tone.shape == (61,)
    err = np.abs(np.abs(tone) * 1024 - f)
    print("tone estimate: worst error %.4f coarse bins" % err.max())
    assert np.all(err < 0.1)
