"""DspMat.transpose, from_interleaved, to_interleaved and zero_interleave: every case in f32 and f64, real and complex.
Everything here is a copy, so every comparison is bit for bit (as unsigned integers of the scalar's width): no
tolerance anywhere.

  * transpose against numpy's .T of the matrix viewed in elements (a complex pair stays together), on shapes that cross
    a tile edge in each direction for any tile of 16 .. 64, put f32 rows on odd 4-byte boundaries, go down the thin path
    both ways round and exceed 65535 rows; the state after the call, with the next kernel (fft, statistics) as witness;
  * from_interleaved against the reshaped vector and against DspVec.split_into; to_interleaved against the transposed
    matrix and against DspVec.merge of the rows; the round trip;
  * zero_interleave against numpy and against DspVec.zero_interleave on the rows;
  * the codes, poisoned and empty sources;
  * the README's two snippets."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME, FREQ = 0, 1
CONV_SINC = 0
VARIANTS = [(np.float32, False), (np.float32, True), (np.float64, False), (np.float64, True)]
VARIANT_IDS = ["f32-real", "f32-complex", "f64-real", "f64-complex"]

TRANSPOSE_SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (63, 65), (64, 64), (65, 63), (127, 129), (257, 100), (100, 257),
                    (1025, 33), (33, 1025), (70000, 3), (3, 70000)]                            # (rows, points)
BIG_SHAPES = [(4194305, 1), (1, 4194305)]                                                      # f32 real only: 16 MB
INTERLEAVED_CASES = [(1, 1), (6, 2), (6, 3), (10, 5), (1000, 8), (210000, 3), (4099, 4099), (12, 1)]   # (points, channels)
MERGE_SHAPES = [s for s in TRANSPOSE_SHAPES if s[0] * s[1] <= 1025 * 33]
ZERO_SHAPES = [(3, 5), (257, 100), (70000, 3)]
FACTORS = [0, 1, 2, 3, 7]


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(_bits(got), _bits(ref))


_NOISE = {}


def _noise(scalars, dtype):
    """read-only uniform(-10, 10) scalars; computed once per (size, dtype) and shared"""
    key = (scalars, np.dtype(dtype).name)
    if key not in _NOISE:
        x = np.random.default_rng(scalars).uniform(-10, 10, scalars).astype(dtype)
        x.setflags(write=False)
        _NOISE[key] = x
    return _NOISE[key]


def _t(a, rows, points, e):
    """[rows, points * e] scalars -> the transposed [points, rows * e]: elements of e scalars stay together"""
    return np.ascontiguousarray(a.reshape(rows, points, e).transpose(1, 0, 2)).reshape(points, rows * e)


def _poisoned_mat(bd, dtype, cplx):
    m = bd.DspMat(np.ones((2, 4), dtype), is_complex=cplx)
    assert m.multiply_frequency_response(CONV_SINC, 0.5) == -1   # the time domain has no frequency response: poisoned
    assert _mat_is_poisoned(m)
    return m


def _poisoned_vec(bd, dtype, cplx):
    v = bd.DspVec(np.ones(4, dtype), is_complex=cplx)
    assert v.multiply_frequency_response(CONV_SINC, 0.5) == -1 and v.is_erroneous()
    return v


def _mat_is_poisoned(m):
    return m.row_len() == 0 and np.isnan(m.delta())


# ---------------------------------------------------------------------------------------------- transpose
def _check_transpose(bd, dtype, cplx, rows, points):
    e = 2 if cplx else 1
    x = _noise(rows * points * e, dtype).reshape(rows, points * e)
    m = bd.DspMat(x, is_complex=cplx, domain=FREQ, delta=0.25)
    assert m.transpose() == 0
    assert m.rows() == points and m.row_points() == rows and m.row_len() == rows * e
    assert m.is_complex() == cplx and m.domain() == FREQ and m.delta() == 0.25
    got = m.data()
    _same(got, _t(x, rows, points, e))
    if cplx:   # the issue's wording: the complex view against .T
        ct = np.complex64 if dtype == np.float32 else np.complex128
        _same(got.view(ct).view(dtype), np.ascontiguousarray(x.view(ct).T).view(dtype))
    assert m.transpose() == 0   # and back
    assert m.rows() == rows and m.row_points() == points
    _same(m.data(), x)


@pytest.mark.parametrize("rows,points", TRANSPOSE_SHAPES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_transpose(bd, dtype, cplx, rows, points):
    _check_transpose(bd, dtype, cplx, rows, points)


@pytest.mark.parametrize("rows,points", BIG_SHAPES)
def test_transpose_more_than_65535_tiles(bd, rows, points):
    _check_transpose(bd, np.float32, False, rows, points)


@pytest.mark.parametrize("rows,points", [(63, 65), (257, 100)])
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_the_next_call_sees_the_transposed_matrix(bd, dtype, cplx, rows, points):
    """transpose then fft / statistics is the same kernel on the same input as on a matrix uploaded transposed: the
    trade buffers and the lengths are coherent for the next call"""
    e = 2 if cplx else 1
    x = _noise(rows * points * e, dtype).reshape(rows, points * e)
    xt = _t(x, rows, points, e)
    m, ref = bd.DspMat(x, is_complex=cplx), bd.DspMat(xt, is_complex=cplx)
    assert m.transpose() == 0 and m.fft() == 0 and ref.fft() == 0
    assert m.rows() == ref.rows() == points and m.row_points() == ref.row_points() == rows and m.is_complex()
    _same(m.data(), ref.data())
    m, ref = bd.DspMat(x, is_complex=cplx), bd.DspMat(xt, is_complex=cplx)
    assert m.transpose() == 0
    got, want = m.statistics(), ref.statistics()
    assert got["max_index"].shape == (points,) and np.array_equal(got["max_index"], want["max_index"])
    assert np.array_equal(got["min_index"], want["min_index"])


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_transpose_of_empty_and_poisoned_matrices(bd, dtype, cplx):
    for rows, row_len in ((0, 0), (5, 0), (0, 8)):
        m = bd.DspMat(rows=rows, row_len=row_len, is_complex=cplx, dtype=dtype, delta=0.5)
        assert m.transpose() == 0
        assert m.rows() == 0 and m.row_points() == 0 and m.delta() == 0.5 and not _mat_is_poisoned(m)
        assert m.transpose() == 0 and m.rows() == 0   # the row count does not come back
    m = _poisoned_mat(bd, dtype, cplx)
    assert m.transpose() == -1
    assert _mat_is_poisoned(m) and m.rows() == 2 and m.is_complex() == cplx


# ---------------------------------------------------------------------------------------------- from_interleaved
@pytest.mark.parametrize("points,channels", INTERLEAVED_CASES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_from_interleaved(bd, dtype, cplx, points, channels):
    e = 2 if cplx else 1
    x = _noise(points * e, dtype)
    v = bd.DspVec(x, is_complex=cplx, domain=FREQ, delta=0.25)
    code, m = bd.DspMat.from_interleaved(v, channels)
    assert code == 0 and m is not None
    per = points // channels
    assert m.rows() == channels and m.row_points() == per and m.row_len() == per * e
    assert m.is_complex() == cplx and m.domain() == FREQ and m.delta() == 0.25 and m.dtype == dtype
    got = m.data()
    _same(got, _t(x.reshape(per, channels * e), per, channels, e))   # x.reshape(P // C, C).T in elements
    _same(v.data(), x)   # the source is as it was
    if channels <= 8:    # row by row against split_into with `channels` targets
        targets = [bd.DspVec(dtype=dtype, length=0, is_complex=cplx) for _ in range(channels)]
        assert v.split_into(targets) == 9
        for c in range(channels):
            _same(got[c], targets[c].data())
    code, back = m.to_interleaved()   # and the round trip is the identity
    assert code == 0 and back.points() == points and back.is_complex() == cplx
    assert back.domain() == FREQ and back.delta() == 0.25
    _same(back.data(), x)


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_from_interleaved_codes(bd, dtype, cplx):
    e = 2 if cplx else 1
    v = bd.DspVec(_noise(7 * e, dtype), is_complex=cplx)
    assert bd.DspMat.from_interleaved(v, 2) == (7, None)
    assert bd.DspMat.from_interleaved(v, 0) == (7, None)
    code, m = bd.DspMat.from_interleaved(bd.DspVec(dtype=dtype, length=0, is_complex=cplx, delta=0.5), 4)
    assert code == 0 and m.rows() == 4 and m.row_points() == 0 and m.delta() == 0.5 and not _mat_is_poisoned(m)
    assert m.is_complex() == cplx and m.data().shape == (4, 0)
    code, m = bd.DspMat.from_interleaved(_poisoned_vec(bd, dtype, cplx), 2)
    assert code == -1 and m is not None and _mat_is_poisoned(m) and m.rows() == 2


# ---------------------------------------------------------------------------------------------- to_interleaved
@pytest.mark.parametrize("rows,points", MERGE_SHAPES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_to_interleaved(bd, dtype, cplx, rows, points):
    e = 2 if cplx else 1
    x = _noise(rows * points * e, dtype).reshape(rows, points * e)
    m = bd.DspMat(x, is_complex=cplx, domain=FREQ, delta=0.25)
    code, y = m.to_interleaved()
    assert code == 0 and y is not None
    assert y.points() == rows * points and len(y) == rows * points * e
    assert y.is_complex() == cplx and y.domain() == FREQ and y.delta() == 0.25
    got = y.data()
    _same(got, _t(x, rows, points, e).reshape(-1))   # a.T.reshape(-1) in elements
    merged = bd.DspVec(dtype=dtype, length=0, is_complex=cplx)
    assert merged.merge([m.get_row(r) for r in range(rows)]) == 0
    _same(got, merged.data())
    _same(m.data(), x)   # the matrix is as it was
    assert m.rows() == rows


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_to_interleaved_of_empty_and_poisoned_matrices(bd, dtype, cplx):
    code, y = bd.DspMat(rows=0, row_len=0, is_complex=cplx, dtype=dtype, delta=0.5).to_interleaved()
    assert code == 0 and len(y) == 0 and y.delta() == 0.5 and y.is_complex() == cplx and not y.is_erroneous()
    code, y = _poisoned_mat(bd, dtype, cplx).to_interleaved()
    assert code == -1 and y is not None and y.is_erroneous()


# ---------------------------------------------------------------------------------------------- zero_interleave
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("rows,points", ZERO_SHAPES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_zero_interleave(bd, dtype, cplx, rows, points, factor):
    e = 2 if cplx else 1
    x = _noise(rows * points * e, dtype).reshape(rows, points * e)
    m = bd.DspMat(x, is_complex=cplx, domain=FREQ, delta=0.25)
    assert m.zero_interleave(factor) == 0
    f = max(factor, 1)
    assert m.rows() == rows and m.row_points() == points * f and m.row_len() == points * f * e
    assert m.is_complex() == cplx and m.domain() == FREQ and m.delta() == 0.25
    ref = np.zeros((rows, points, f, e), dtype)
    ref[:, :, 0, :] = x.reshape(rows, points, e)
    got = m.data()
    _same(got, ref.reshape(rows, points * f * e))
    if rows <= 257:   # every row as the vector call on it
        src = bd.DspMat(x, is_complex=cplx)
        for r in range(rows):
            v = src.get_row(r)
            assert v.zero_interleave(factor) == 0
            _same(got[r], v.data())


@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_zero_interleave_of_a_poisoned_matrix(bd, dtype, cplx):
    for factor in (1, 3):
        m = _poisoned_mat(bd, dtype, cplx)
        assert m.zero_interleave(factor) == -1 and _mat_is_poisoned(m) and m.rows() == 2
    m = bd.DspMat(rows=3, row_len=0, is_complex=cplx, dtype=dtype)
    assert m.zero_interleave(4) == 0 and m.rows() == 3 and m.row_points() == 0


# ---------------------------------------------------------------------------------------------- the README's snippets
def _readme_block(marker):
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if marker in b]
    assert len(blocks) == 1, marker
    return blocks[0]


@pytest.mark.parametrize("delay,doppler", [(17, 5), (30, -9)])
def test_readme_range_doppler_snippet(bd, delay, doppler):
    """The README's snippet as written, on 64 pulses x 100 -> 256 points: every pulse is the template -- a 64-point
    linear FM chirp -- delayed by `delay` samples, and pulse r carries the phase exp(2 pi i doppler r / 64), a Doppler
    shift of a whole bin.  correlate leaves lag 0 at index 128 of every row, so the range peak sits at 128 + delay;
    after transpose every row is one range bin over the 64 pulses, and windowed_fft leaves the fft_shift layout (bin b at
    index b + 32), so the peak of the whole map is the cell (128 + delay, 32 + doppler)."""
    code = _readme_block("pulses.transpose()")
    assert "pulses.correlate(template) == 0" in code and "pulses.windowed_fft(V.WINDOW_HANN) == 0" in code
    assert "pulses.magnitude() == 0" in code
    rows, n, l = 64, 100, 256
    t = np.arange(64)
    chirp = np.exp(1j * np.pi * 0.9 * (t - 32.0) ** 2 / 64.0)
    z = np.zeros((rows, n), np.complex64)
    z[:, delay:delay + 64] = chirp[None, :] * np.exp(2j * np.pi * doppler * np.arange(rows) / rows)[:, None]
    tmpl = np.zeros(n, np.complex64)
    tmpl[:64] = chirp
    template = bd.DspVec(tmpl.view(np.float32), is_complex=True)
    assert template.zero_pad(l, 1) == 0 and template.prepare_argument() == 0
    pulses = bd.DspMat(z.view(np.float32), is_complex=True)
    env = {"np": np, "pulses": pulses, "template": template, "V": bd.vector}
    exec(code, env)
    assert pulses.rows() == l and pulses.row_points() == rows and not pulses.is_complex()
    rd = pulses.data()
    assert np.unravel_index(np.argmax(rd), rd.shape) == (l // 2 + delay, rows // 2 + doppler)
    assert pulses.statistics()["max_index"][l // 2 + delay] == rows // 2 + doppler


def test_readme_interleaved_channels_snippet(bd):
    """The README's snippet as written: interleaved channels -> one row per channel -> fft of every channel -> interleaved
    again; against the same transform of the matrix uploaded channel by channel."""
    code = _readme_block("DspMat.from_interleaved(")
    assert "ch.fft() == 0" in code and "ch.to_interleaved()" in code
    env = {"np": np, "DspVec": bd.DspVec, "DspMat": bd.DspMat, "V": bd.vector}
    exec(code, env)
    ch, spectra = env["ch"], env["spectra"]
    assert env["code"] == 0 and ch.rows() == 8 and ch.row_points() == 4096 and spectra.points() == 8 * 4096
    ref = bd.DspMat(_t(env["rec"].data().reshape(4096, 16), 4096, 8, 2), is_complex=True)   # rec is as it was
    assert ref.fft() == 0
    _same(ch.data(), ref.data())
    _same(spectra.data(), _t(ch.data(), 8, 4096, 2).reshape(-1))
    assert spectra.domain() == FREQ and spectra.is_complex()
