"""DspMat.from_frames, overlap_add, from_vectors and the batched zero_pad / swap_halves / fft_shift / ifft_shift: every
case in f32 and f64, real and complex, against numpy -- and the index moves also against the vector call on get_row.
Everything here is a copy or an ordered add, so every comparison is bit for bit (as unsigned integers of the scalar's
width): no tolerance anywhere.

  * from_frames against numpy.lib.stride_tricks.sliding_window_view of the zero-extended input, sliced [::hop];
  * overlap_add against the ascending-row accumulation y[r * H : r * H + F] += m[r] in the matrix's dtype; two runs
    agree; from_frames(pad_tail=True) -> overlap_add(H) equals the input added up once per covering frame, accumulated
    the same way;
  * from_vectors against the stacked data() of the vectors;
  * the codes, poisoned and empty sources;
  * the README's STFT snippet."""
import os
import re

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from test_gpu_mat_ew import _vector_path_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME, FREQ = 0, 1
META_DATA = 2  # BDSP_ERR_META_DATA, the code mat_binary_vector returns when the meta data disagree
VARIANTS = [(np.float32, False), (np.float32, True), (np.float64, False), (np.float64, True)]
VARIANT_IDS = ["f32-real", "f32-complex", "f64-real", "f64-complex"]

FRAME_CASES = [(1, 1, 1), (10, 4, 2), (10, 4, 3), (11, 4, 3), (10, 4, 5), (3, 4, 1), (1000, 127, 1), (1025, 256, 128),
               (70002, 3, 1)]                                                                    # (P, F, H)
OLA_CASES = [(1, 1, 1), (3, 4, 2), (3, 4, 3), (3, 4, 5), (4, 4, 4), (5, 127, 1), (257, 100, 25), (9, 1025, 512),
             (2, 4097, 4096), (70000, 3, 1)]                                                     # (rows, F, H)
VECTOR_CASES = [(1, 1), (3, 5), (5, 7), (257, 100), (9, 1025), (300, 3)]                         # (rows, scalars)
PAD_CASES = [(70000, 3, 4), (257, 100, 128), (5, 1025, 2048), (3, 1, 2)]                         # (rows, points, new points)
SWAP_CASES = [(3, 1), (3, 2), (4, 127), (4, 128), (9, 1025), (70000, 3)]                         # (rows, points)


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


def _noise(scalars, dtype, seed=0):
    """read-only uniform(-10, 10) scalars; computed once per (size, dtype, seed) and shared"""
    key = (scalars, np.dtype(dtype).name, seed)
    if key not in _NOISE:
        x = np.random.default_rng(1000 * seed + scalars).uniform(-10, 10, scalars).astype(dtype)
        x.setflags(write=False)
        _NOISE[key] = x
    return _NOISE[key]


def _rows_expected(P, F, H, pad_tail):
    if not pad_tail:
        return (P - F) // H + 1 if P >= F else 0
    return 0 if P == 0 else (-((P - F) // -H) + 1 if P > F else 1)


def _frames_ref(x, e, F, H, rows):
    """x: P * e scalars -> [rows, F * e]: the sliding windows of the zero-extended input, every H-th"""
    pts = x.reshape(-1, e)
    need = (rows - 1) * H + F
    if need > len(pts):
        pts = np.concatenate([pts, np.zeros((need - len(pts), e), x.dtype)])
    win = sliding_window_view(pts, F, axis=0)[::H][:rows]  # [rows, e, F]
    return np.ascontiguousarray(win.transpose(0, 2, 1)).reshape(rows, F * e)


def _ola_ref(m, e, F, H):
    """the ascending-row accumulation in the matrix's dtype"""
    rows = m.shape[0]
    y = np.zeros(((rows - 1) * H + F, e), m.dtype)
    for r in range(rows):
        y[r * H:r * H + F] += m[r].reshape(F, e)
    return y.reshape(-1)


def _poisoned_vec(bd, dtype):
    v = bd.DspVec(np.ones(4, dtype))
    assert v.magnitude() == -1 and v.is_erroneous()  # a real vector has no magnitude: poisoned
    return v


def _poisoned_mat(bd, dtype):
    m = bd.DspMat(np.ones((2, 4), dtype))
    assert m.conj() == -1
    return m


def _mat_is_poisoned(m):
    return m.row_len() == 0 and np.isnan(m.delta())


# ---------------------------------------------------------------------------------------------- from_frames
@pytest.mark.parametrize("pad_tail", [False, True], ids=["whole", "pad_tail"])
@pytest.mark.parametrize("P,F,H", FRAME_CASES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_from_frames(bd, dtype, cplx, P, F, H, pad_tail):
    e = 2 if cplx else 1
    x = _noise(P * e, dtype)
    v = bd.DspVec(x, is_complex=cplx, domain=FREQ if P % 2 else TIME, delta=0.25)
    code, m = bd.DspMat.from_frames(v, F, H, pad_tail)
    rows = _rows_expected(P, F, H, pad_tail)
    assert code == 0 and m is not None
    assert m.rows() == rows
    assert m.row_points() == (F if rows else 0) and m.row_len() == (F * e if rows else 0)
    assert m.is_complex() == cplx and m.domain() == v.domain() and m.delta() == 0.25 and m.dtype == dtype
    got = m.data()
    if rows:
        _same(got, _frames_ref(x, e, F, H, rows))
    else:
        assert got.size == 0
    _same(v.data(), x)  # the source is as it was
    assert len(v) == P * e and v.delta() == 0.25


# ---------------------------------------------------------------------------------------------- overlap_add
@pytest.mark.parametrize("rows,F,H", OLA_CASES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_overlap_add(bd, dtype, cplx, rows, F, H):
    e = 2 if cplx else 1
    x = _noise(rows * F * e, dtype, seed=1).reshape(rows, F * e)
    m = bd.DspMat(x, is_complex=cplx, domain=FREQ, delta=0.5)
    code, y = m.overlap_add(H)
    assert code == 0 and y is not None
    assert y.points() == (rows - 1) * H + F and len(y) == y.points() * e
    assert y.is_complex() == cplx and y.domain() == FREQ and y.delta() == 0.5 and y.dtype == dtype
    got = y.data()
    _same(got, _ola_ref(x, e, F, H))
    code2, y2 = m.overlap_add(H)  # deterministic: a second run agrees bit for bit
    assert code2 == 0
    _same(y2.data(), got)
    _same(m.data(), x)  # the matrix is as it was
    if H > F:
        gaps = got.reshape(-1, e)[F:H]
        assert gaps.size and not gaps.any()
    if H == F:
        _same(got, x.reshape(-1))  # the flatten


@pytest.mark.parametrize("P,F,H", FRAME_CASES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_frames_then_overlap_add_is_the_input_times_its_coverage(bd, dtype, cplx, P, F, H):
    """every point comes back once per frame that covers it: the input added up, frame after frame in ascending order,
    in the vector's dtype (count * x in one rounding per addition -- accumulated the same way, so bit for bit)"""
    e = 2 if cplx else 1
    x = _noise(P * e, dtype)
    code, m = bd.DspMat.from_frames(bd.DspVec(x, is_complex=cplx), F, H, True)
    assert code == 0
    rows = m.rows()
    code, y = m.overlap_add(H)
    assert code == 0
    n = (rows - 1) * H + F
    assert y.points() == n >= P
    xz = np.concatenate([x.reshape(-1, e), np.zeros((n - P, e), dtype)])
    acc = np.zeros((n, e), dtype)
    count = np.zeros(n, np.int64)
    for r in range(rows):
        acc[r * H:r * H + F] += xz[r * H:r * H + F]
        count[r * H:r * H + F] += 1
    _same(y.data(), acc.reshape(-1))
    if H <= F:
        assert count[:P].min() >= 1  # pad_tail and no gaps between frames: every input point lies in a frame
    once = count == 1
    _same(y.data().reshape(n, e)[once], xz[once])


# ---------------------------------------------------------------------------------------------- from_vectors
@pytest.mark.parametrize("rows,scalars", VECTOR_CASES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_from_vectors(bd, dtype, cplx, rows, scalars):
    e = 2 if cplx else 1
    x = _noise(rows * scalars * e, dtype, seed=2).reshape(rows, scalars * e)
    vs = [bd.DspVec(x[r], is_complex=cplx, domain=FREQ, delta=0.125 if r == 0 else 1.0) for r in range(rows)]
    code, m = bd.DspMat.from_vectors(vs)
    assert code == 0 and m is not None
    assert m.rows() == rows and m.row_len() == scalars * e and m.row_points() == scalars
    assert m.is_complex() == cplx and m.domain() == FREQ and m.delta() == 0.125 and m.dtype == dtype  # the first vector's
    _same(m.data(), np.stack([v.data() for v in vs]))
    _same(m.data(), x)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_from_vectors_codes(bd, dtype):
    code, m = bd.DspMat.from_vectors([], dtype=dtype)
    assert code == 0 and m.rows() == 0 and m.row_len() == 0 and m.dtype == dtype and m.data().size == 0
    a, b = bd.DspVec(np.ones(6, dtype)), bd.DspVec(np.ones(8, dtype))
    assert bd.DspMat.from_vectors([a, b]) == (7, None)
    assert bd.DspMat.from_vectors([a, a, b]) == (7, None)
    c = bd.DspVec(np.ones(6, dtype), is_complex=True)
    assert bd.DspMat.from_vectors([a, c]) == (META_DATA, None)  # real with complex
    f = bd.DspVec(np.ones(6, dtype), domain=FREQ)
    assert bd.DspMat.from_vectors([a, f]) == (META_DATA, None)  # time with frequency
    assert bd.DspMat.from_vectors([f, a]) == (META_DATA, None)
    code, m = bd.DspMat.from_vectors([a, _poisoned_vec(bd, dtype), a])
    assert code == -1 and m is not None and _mat_is_poisoned(m)
    code, m = bd.DspMat.from_vectors([_poisoned_vec(bd, dtype)])
    assert code == -1 and _mat_is_poisoned(m)
    # empty vectors: rows without points
    z = bd.DspVec(np.zeros(0, dtype))
    code, m = bd.DspMat.from_vectors([z, z])
    assert code == 0 and m.rows() == 2 and m.row_len() == 0
    _same(a.data(), np.ones(6, dtype))


# ---------------------------------------------------------------------------------------------- codes
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_frame_codes(bd, dtype, cplx):
    e = 2 if cplx else 1
    v = bd.DspVec(_noise(10 * e, dtype), is_complex=cplx)
    assert bd.DspMat.from_frames(v, 0, 2) == (7, None)
    assert bd.DspMat.from_frames(v, 4, 0) == (7, None)
    assert bd.DspMat.from_frames(v, 0, 0, True) == (7, None)
    m = bd.DspMat(_noise(3 * 4 * e, dtype).reshape(3, 4 * e), is_complex=cplx)
    assert m.overlap_add(0) == (7, None)
    # poisoned sources: -1 and a poisoned result
    code, pm = bd.DspMat.from_frames(_poisoned_vec(bd, dtype), 4, 2)
    assert code == -1 and pm is not None and pm.rows() == 0 and _mat_is_poisoned(pm)
    code, pm = bd.DspMat.from_frames(_poisoned_vec(bd, dtype), 4, 2, True)
    assert code == -1 and _mat_is_poisoned(pm)
    code, pv = _poisoned_mat(bd, dtype).overlap_add(2)
    assert code == -1 and pv is not None and pv.is_erroneous()
    # empty sources: empty results
    empty = bd.DspVec(np.zeros(0, dtype), is_complex=cplx, delta=2.0)
    for pad_tail in (False, True):
        code, em = bd.DspMat.from_frames(empty, 4, 2, pad_tail)
        assert code == 0 and em.rows() == 0 and em.row_len() == 0 and em.delta() == 2.0 and em.is_complex() == cplx
        code, ev = em.overlap_add(2)
        assert code == 0 and len(ev) == 0 and not ev.is_erroneous() and ev.is_complex() == cplx
    # a hop past the end of the vector
    code, hm = bd.DspMat.from_frames(v, 4, 1000, True)
    assert code == 0 and hm.rows() == 2
    ref = np.zeros((2, 4 * e), dtype)
    ref[0] = v.data()[:4 * e]
    _same(hm.data(), ref)


# ---------------------------------------------------------------------------------------------- batched index moves
def _pad_ref(x, e, p, points, option):
    """zero_pad per row: End, Surround (right = diff // 2), Center (the first ceil(p / 2) points stay, the last
    floor(p / 2) move to the end)"""
    rows = x.shape[0]
    pts = x.reshape(rows, p, e)
    out = np.zeros((rows, points, e), x.dtype)
    if option == 0:
        out[:, :p] = pts
    elif option == 1:
        diff = points - p
        left = diff - diff // 2
        out[:, left:left + p] = pts
    else:
        right = p // 2
        out[:, :p - right] = pts[:, :p - right]
        out[:, points - right:] = pts[:, p - right:]
    return out.reshape(rows, points * e)


@pytest.mark.parametrize("option", [0, 1, 2], ids=["end", "surround", "center"])
@pytest.mark.parametrize("rows,p,points", PAD_CASES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_zero_pad(bd, dtype, cplx, rows, p, points, option):
    e = 2 if cplx else 1
    x = _noise(rows * p * e, dtype, seed=3).reshape(rows, p * e)
    m = bd.DspMat(x, is_complex=cplx, delta=0.5)
    assert m.zero_pad(points, option) == 0
    assert m.rows() == rows and m.row_points() == points and m.delta() == 0.5 and m.is_complex() == cplx
    got = m.data()
    _same(got, _pad_ref(x, e, p, points, option))
    src = bd.DspMat(x, is_complex=cplx, delta=0.5)
    for r in _vector_path_rows(rows):
        v = src.get_row(r)
        assert v.zero_pad(points, option) == 0
        _same(got[r], v.data())


@pytest.mark.parametrize("name", ["swap_halves", "fft_shift", "ifft_shift"])
@pytest.mark.parametrize("rows,p", SWAP_CASES)
@pytest.mark.parametrize("dtype,cplx", VARIANTS, ids=VARIANT_IDS)
def test_swaps(bd, dtype, cplx, rows, p, name):
    e = 2 if cplx else 1
    x = _noise(rows * p * e, dtype, seed=4).reshape(rows, p * e)
    m = bd.DspMat(x, is_complex=cplx, delta=0.5)
    assert getattr(m, name)() == 0
    assert m.rows() == rows and m.row_points() == p and m.delta() == 0.5
    got = m.data()
    shift = p // 2 if name == "ifft_shift" else p - p // 2  # out[i] = in[(i + shift) mod p]
    _same(got, np.roll(x.reshape(rows, p, e), -shift, axis=1).reshape(rows, p * e))
    if name == "fft_shift":
        _same(got, np.fft.fftshift(x.reshape(rows, p, e), axes=1).reshape(rows, p * e))
    if name == "ifft_shift":
        _same(got, np.fft.ifftshift(x.reshape(rows, p, e), axes=1).reshape(rows, p * e))
    src = bd.DspMat(x, is_complex=cplx, delta=0.5)
    for r in _vector_path_rows(rows):
        v = src.get_row(r)
        assert getattr(v, name)() == 0
        _same(got[r], v.data())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_moves_keep_a_poisoned_matrix_poisoned(bd, dtype):
    for call in (lambda m: m.zero_pad(8), lambda m: m.zero_pad(8, 1), lambda m: m.zero_pad(8, 2), lambda m: m.swap_halves(),
                 lambda m: m.fft_shift(), lambda m: m.ifft_shift()):
        m = _poisoned_mat(bd, dtype)
        assert call(m) == -1
        assert _mat_is_poisoned(m)
    m = bd.DspMat(np.ones((2, 4), dtype))
    assert m.zero_pad(4) == 7 and m.zero_pad(3, 1) == 7  # not longer than the rows: the argument error, as before
    _same(m.data(), np.ones((2, 4), dtype))
    e = bd.DspMat(rows=0, row_len=0, dtype=dtype)
    assert e.swap_halves() == 0 and e.rows() == 0


# ---------------------------------------------------------------------------------------------- the README's snippet
@pytest.mark.parametrize("k", [200, 512])
def test_readme_stft_snippet(bd, k):
    """The README's snippet as written: a tone at bin k of a 1024-point frame in a 16 384-point real vector ->
    from_frames(x, 1024, 256) -> windowed_fft(HANN) -> magnitude -> statistics()["max_index"] is that bin in every row.
    windowed_fft leaves the fft_shift layout (bin b at index (b + 512) mod 1024) and the spectrum of a real signal is
    conjugate symmetric, so bin k shows as the pair of indices 512 - k and 512 + k with equal magnitudes in exact
    arithmetic; which of the two rounding leaves a last bit ahead is not a property of the tone.  k = 200: the peak is
    200 bins from the centre in every row.  k = 512, the Nyquist bin, is its own mirror image: one index, 0, and the
    equality is exact.  Then the synthesis half: pad_tail frames, a window, overlap_add -- against the numpy
    accumulation of the downloaded frames, bit for bit."""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "from_frames" in b]
    assert len(blocks) == 1
    code = blocks[0]
    assert "DspMat.from_frames(x, 1024, 256)" in code and "frames.windowed_fft(V.WINDOW_HANN) == 0" in code
    assert 'peak = frames.statistics()["max_index"]' in code and "frames.overlap_add(256)" in code
    F, H, rows = 1024, 256, 61
    env = {"np": np, "k": k, "DspVec": bd.DspVec, "DspMat": bd.DspMat, "V": bd.vector}
    exec(code, env)
    peak = env["peak"]
    assert peak.shape == (rows,)
    if k == F // 2:
        assert np.array_equal(peak, np.full(rows, (k + F // 2) % F))
    else:
        assert np.array_equal(np.abs(peak - F // 2), np.full(rows, k))
    frames, y = env["frames"], env["y"]
    assert env["code"] == 0 and frames.rows() == rows and y.points() == (rows - 1) * H + F == 16384
    assert not y.is_complex() and y.domain() == TIME
    _same(y.data(), _ola_ref(frames.data(), 1, F, H))
