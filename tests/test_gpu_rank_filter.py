"""rank_filter and medfilt: sliding order statistics along a DspVec or along every row of a DspMat on the device, through
the Python functions.

The result is one of the input values, so every comparison is equality of the bit patterns (view(uint)), never a
tolerance.  The numpy model is written here: it builds the padded row by the boundary rule, takes sliding_window_view,
deletes the guard columns, maps the bits to integer keys in IEEE totalOrder (-NaN < -inf < ... < -0 < +0 < ... < +inf <
+NaN), sorts along the window, takes column `rank` and maps back.  The shapes are tests/rank_filter_shapes.txt, which the
host simulation (tests/host_sim/sim_rank_filter.cpp) reads too; each line runs in f32 and f64, on data with heavy ties
(16 levels) and on data seeded with +-0, +-inf, +-NaN with payloads and denormals."""
import functools
import os
import re

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = [np.float32, np.float64]
PREC_IDS = ["f32", "f64"]


def read_constants():
    with open(os.path.join(ROOT, "basic_dsp_amd", "csrc", "rank_filter_core.h")) as f:
        return {k: int(v) for k, v in re.findall(r"^constexpr int (RANK_\w+) = (\d+);", f.read(), re.M)}


def read_shapes():
    out = []
    with open(os.path.join(ROOT, "tests", "rank_filter_shapes.txt")) as f:
        for line in f:
            w = line.split("#")[0].split()
            if w:
                out.append((int(w[0]), int(w[1]), int(w[2]), int(w[3]), None if w[4] == "none" else int(w[4]), w[5]))
    return out


K = read_constants()
TILE, MAX_HALF = K["RANK_TILE"], K["RANK_MAX_HALF"]
CROSS = {np.float32: K["RANK_CROSS_F32"], np.float64: K["RANK_CROSS_F64"]}
SHAPES = read_shapes()
SHAPE_IDS = ["-".join(str(w) for w in s) for s in SHAPES]


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def uint_of(dtype):
    return np.uint32 if np.dtype(dtype) == np.float32 else np.uint64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(uint_of(a.dtype))


def to_keys(b):
    top = b.dtype.type(1) << b.dtype.type(8 * b.dtype.itemsize - 1)
    return np.where(b & top != 0, ~b, b ^ top)


def from_keys(k):
    top = k.dtype.type(1) << k.dtype.type(8 * k.dtype.itemsize - 1)
    return np.where(k & top != 0, k ^ top, ~k)


def window_size(half, guard):
    return 2 * half + 1 if guard is None else 2 * (half - guard)


def windows(a, half, guard, boundary):
    """[rows, n, W]: the windows of every point of every row of a ([rows, n], any dtype), the guard columns deleted"""
    rows, n = a.shape
    pos = np.arange(-half, n + half)
    if boundary == "zero":
        padded = np.zeros((rows, n + 2 * half), a.dtype)  # +0.0: all bits clear
        padded[:, half:half + n] = a
    elif boundary == "wrap":
        padded = a[:, pos % n]
    else:
        assert boundary == "nearest"
        padded = a[:, np.clip(pos, 0, n - 1)]
    win = sliding_window_view(padded, 2 * half + 1, axis=1)
    if guard is not None:
        win = np.delete(win, np.arange(half - guard, half + guard + 1), axis=2)
    return win


def model(x, half, rank, guard, boundary):
    """the bits of the result, [rows, n] unsigned"""
    keys = np.sort(to_keys(windows(bits(x), half, guard, boundary)), axis=2)
    assert keys.shape[2] == window_size(half, guard)
    return from_keys(keys[:, :, rank])


def special_bits(dtype):
    """+-0, +-inf, +-NaN (quiet, signalling, with payloads), +-denormals, as bit patterns"""
    u = uint_of(dtype)
    e, m = (8, 23) if u == np.uint32 else (11, 52)
    emax, mmax, quiet = (1 << e) - 1, (1 << m) - 1, 1 << (m - 1)
    pos = [0, 1, 77, mmax, emax << m, (emax << m) | 1, (emax << m) | quiet, (emax << m) | quiet | 12345, (emax << m) | mmax]
    return np.array(pos + [p | (1 << (e + m)) for p in pos], dtype=u)


def draw(seed, rows, n, dtype, kind):
    """ties: 16 levels, both signs.  special: the same with three values in ten replaced by a special bit pattern.
    plain: 16 levels, finite, no zero of either sign."""
    rng = np.random.default_rng(seed)
    level = rng.integers(0, 16, (rows, n))
    if kind == "plain":
        return ((level - 8) * 0.25 + 0.125).astype(dtype)
    x = ((level - 8) * 0.25).astype(dtype)
    if kind == "special":
        sp = special_bits(dtype)
        mask = rng.random((rows, n)) < 0.3
        b = bits(x).copy()
        b[mask] = sp[rng.integers(0, len(sp), int(mask.sum()))]
        x = b.view(dtype)
    return x


@functools.lru_cache(maxsize=None)
def case(line, prec, kind):
    """(x, the model's bits) of a shapes line: computed once, shared and never written to"""
    rows, n, half, rank, guard, boundary = SHAPES[line]
    x = draw(4000 + 7 * line + prec, rows, n, PRECS[prec], kind)
    want = model(x, half, rank, guard, boundary)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def same_bits(got, want_bits):
    return got.shape == want_bits.shape and np.array_equal(bits(got), want_bits)


@pytest.mark.parametrize("kind", ["ties", "special"])
@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
@pytest.mark.parametrize("line", range(len(SHAPES)), ids=SHAPE_IDS)
def test_every_shape_line_equals_the_model_bit_for_bit(bd, line, prec, kind):
    rows, n, half, rank, guard, boundary = SHAPES[line]
    x, want = case(line, prec, kind)
    m = bd.DspMat(x, delta=0.5)
    assert bd.rank_filter(m, half, rank, guard, boundary) == 0
    assert (m.rows(), m.row_len(), m.is_complex(), m.domain(), m.delta()) == (rows, n, False, 0, 0.5)
    got = m.data()
    assert same_bits(got, want), np.argwhere(bits(got) != want)[:5]
    # the vector call on the last row (the lines of one row: the whole line through DspVec): the same bits
    v = bd.DspVec(x[rows - 1], delta=0.5)
    assert bd.rank_filter(v, half, rank, guard=guard, boundary=boundary) == 0
    assert (len(v), v.is_complex(), v.domain(), v.delta()) == (n, False, 0, 0.5)
    assert same_bits(v.data(), want[rows - 1])


def test_the_lines_around_each_crossover_take_both_selectors(bd):
    """W = crossover - 1, crossover, crossover + 1 of each precision: at and below the crossover that precision counts,
    above it bisects; both precisions run every such line against the same model."""
    for dtype in PRECS:
        for w in (CROSS[dtype] - 1, CROSS[dtype], CROSS[dtype] + 1):
            lines = [i for i, s in enumerate(SHAPES) if window_size(s[2], s[4]) == w]
            assert lines, (dtype, w)
            for line in lines:
                rows, n, half, rank, guard, boundary = SHAPES[line]
                for prec in (0, 1):
                    for kind in ("ties", "special"):
                        x, want = case(line, prec, kind)
                        m = bd.DspMat(x)
                        assert bd.rank_filter(m, half, rank, guard, boundary) == 0
                        assert same_bits(m.data(), want), (SHAPES[line], prec, kind)


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_every_row_is_bit_equal_to_the_vector_call_and_independent_of_the_row_count(bd, prec):
    dtype = PRECS[prec]
    for n, half, rank, guard, boundary in ((2 * TILE + 17, 16, 5, None, "wrap"), (TILE + 1, 40, 3, 7, "nearest"), (3, 7, 6, None, "zero")):
        x = draw(90 + n, 7, n, dtype, "special")
        m = bd.DspMat(x)
        assert bd.rank_filter(m, half, rank, guard, boundary) == 0
        got = m.data()
        for r in range(7):
            v = bd.DspVec(x[r].copy())
            assert bd.rank_filter(v, half, rank, guard, boundary) == 0
            assert np.array_equal(bits(v.data()), bits(got[r])), (n, r)
        # one row against seven rows of the same content
        same = np.tile(x[3], (7, 1))
        m7, m1 = bd.DspMat(same), bd.DspMat(same[:1])
        assert bd.rank_filter(m7, half, rank, guard, boundary) == 0 and bd.rank_filter(m1, half, rank, guard, boundary) == 0
        g7, g1 = m7.data(), m1.data()
        for r in range(7):
            assert np.array_equal(bits(g7[r]), bits(g1[0])) and np.array_equal(bits(g7[r]), bits(got[3]))


def test_a_row_count_of_1_and_of_7_on_the_shapes_lines(bd):
    pairs = [(i, j) for i, a in enumerate(SHAPES) for j, b in enumerate(SHAPES) if a[0] == 7 and b[0] == 1 and a[1:] == b[1:]]
    assert pairs
    for seven, one in pairs:
        rows, n, half, rank, guard, boundary = SHAPES[seven]
        for dtype in PRECS:
            row = draw(5, 1, n, dtype, "special")
            m7, m1 = bd.DspMat(np.tile(row, (7, 1))), bd.DspMat(row)
            assert bd.rank_filter(m7, half, rank, guard, boundary) == 0 and bd.rank_filter(m1, half, rank, guard, boundary) == 0
            assert np.array_equal(bits(m7.data()), np.tile(bits(m1.data()), (7, 1)))
            assert same_bits(m1.data(), model(row, half, rank, guard, boundary))


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_identity_min_max_and_the_float_model(bd, prec):
    dtype = PRECS[prec]
    # rank_filter(x, 0, 0) is the identity, special values included
    x = draw(1, 3, TILE + 1, dtype, "special")
    for boundary in ("zero", "wrap", "nearest"):
        m, v = bd.DspMat(x), bd.DspVec(x[1].copy())
        assert bd.rank_filter(m, 0, 0, boundary=boundary) == 0 and bd.rank_filter(v, 0, 0, boundary=boundary) == 0
        assert np.array_equal(bits(m.data()), bits(x)) and np.array_equal(bits(v.data()), bits(x[1]))
    # rank 0 and rank W - 1 are the sliding minimum and maximum of the keys
    for half, guard, boundary in ((4, None, "wrap"), (20, 3, "zero"), (70, 0, "nearest")):
        w = window_size(half, guard)
        keys = to_keys(windows(bits(x), half, guard, boundary))
        lo, hi = bd.DspMat(x), bd.DspMat(x)
        assert bd.rank_filter(lo, half, 0, guard, boundary) == 0 and bd.rank_filter(hi, half, w - 1, guard, boundary) == 0
        assert np.array_equal(bits(lo.data()), from_keys(keys.min(axis=2))) and np.array_equal(bits(hi.data()), from_keys(keys.max(axis=2)))
    # on finite data without zeros of either sign under wrap and nearest, np.sort on the floats gives the same bits
    p = draw(2, 3, TILE + 1, dtype, "plain")
    assert np.all(np.isfinite(p)) and not np.any(p == 0)
    for half, rank, guard, boundary in ((1, 1, None, "nearest"), (16, 9, None, "wrap"), (40, 11, 8, "nearest"), (33, 0, 0, "wrap")):
        want = np.sort(windows(p, half, guard, boundary), axis=2)[:, :, rank]
        m = bd.DspMat(p)
        assert bd.rank_filter(m, half, rank, guard, boundary) == 0
        assert np.array_equal(bits(m.data()), bits(want)) and same_bits(m.data(), model(p, half, rank, guard, boundary))
    # and under zero, where the float model's padding is +0.0 and the data hold no other zero
    want = np.sort(windows(p, 12, None, "zero"), axis=2)[:, :, 12]
    m = bd.DspMat(p)
    assert bd.medfilt(m, 25) == 0 and np.array_equal(bits(m.data()), bits(want))


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_medfilt_equals_scipy_bit_for_bit(bd, prec):
    signal = pytest.importorskip("scipy.signal")
    dtype = PRECS[prec]
    x = draw(3, 3, TILE + 1, dtype, "plain")  # (no zero of either sign: scipy orders -0 and +0 as equal)
    for k in (1, 3, 9, 33, 129):
        want = np.stack([signal.medfilt(row, k) for row in x]).astype(dtype)
        m, v = bd.DspMat(x), bd.DspVec(x[2].copy())
        assert bd.medfilt(m, k) == 0 and bd.medfilt(v, kernel_size=k, boundary="zero") == 0
        assert np.array_equal(bits(m.data()), bits(want)), k
        assert np.array_equal(bits(v.data()), bits(want[2])), k
    d = bd.DspMat(x)
    assert bd.medfilt(d) == 0 and np.array_equal(bits(d.data()), bits(np.stack([signal.medfilt(row) for row in x]).astype(dtype)))


def _poisoned_vec(bd, dtype):
    v = bd.DspVec(np.ones(4, dtype))
    assert v.magnitude() == -1 and v.is_erroneous()
    return v


def _poisoned_mat(bd, dtype):
    m = bd.DspMat(np.ones((2, 4), dtype))
    assert m.conj() == -1
    return m


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_codes_and_edge_cases(bd, prec):
    dtype = PRECS[prec]
    x = draw(11, 3, 40, dtype, "special")

    def fresh():
        return bd.DspMat(x), bd.DspVec(x[0].copy())

    def untouched(m, v):
        assert np.array_equal(bits(m.data()), bits(x)) and np.array_equal(bits(v.data()), bits(x[0]))

    m, v = fresh()
    # 7, the data untouched: rank = W, guard = half, an unknown boundary, an even kernel size
    for half, rank, guard, boundary in ((2, 5, None, "zero"), (0, 1, None, "wrap"), (3, 4, 1, "nearest"), (3, 0, 3, "zero"), (0, 0, 0, "wrap"),
                                        (2, 0, 5, "zero"), (2, 0, None, "reflect"), (2, 0, None, ""), (MAX_HALF + 1, 2 * MAX_HALF + 3, None, "zero")):
        assert bd.rank_filter(m, half, rank, guard, boundary) == 7 and bd.rank_filter(v, half, rank, guard, boundary) == 7
        untouched(m, v)
    for code in (3, -1, 99):  # an unknown boundary at the C entry
        assert getattr(bd.lib, "bdsp_hip_mat_rank_filter" + m._sfx)(m._h, 1, 0, -1, code) == 7
        assert getattr(bd.lib, "bdsp_hip_rank_filter" + v._sfx)(v._h, 1, 0, -1, code) == 7
        assert getattr(bd.lib, "bdsp_hip_rank_filter" + v._sfx)(v._h, 2, 0, -2, 0) == 7  # a guard below -1
    untouched(m, v)
    for k in (0, 2, 4, 40):
        assert bd.medfilt(m, k) == 7 and bd.medfilt(v, k) == 7
    untouched(m, v)
    # the largest rank and the largest guard are accepted
    assert bd.rank_filter(m, 2, 4) == 0 and bd.rank_filter(v, 3, 1, guard=2) == 0
    # 4: complex data, untouched; an argument error comes first
    cm, cv = bd.DspMat(x, is_complex=True), bd.DspVec(x[0].copy(), is_complex=True)
    assert bd.rank_filter(cm, 1, 1) == 4 and bd.rank_filter(cv, 1, 1) == 4 and bd.medfilt(cm, 3) == 4
    assert bd.rank_filter(cm, 1, 3) == 7 and bd.rank_filter(cv, 1, 0, boundary="?") == 7
    assert np.array_equal(bits(cm.data()), bits(x)) and np.array_equal(bits(cv.data()), bits(x[0]))
    # -1: a poisoned operand; an argument error comes first, the number kind after
    assert bd.rank_filter(_poisoned_mat(bd, dtype), 1, 1) == -1 and bd.rank_filter(_poisoned_vec(bd, dtype), 1, 1) == -1
    assert bd.medfilt(_poisoned_mat(bd, dtype)) == -1 and bd.medfilt(_poisoned_vec(bd, dtype), 5) == -1
    assert bd.rank_filter(_poisoned_mat(bd, dtype), 1, 3) == 7 and bd.rank_filter(_poisoned_vec(bd, dtype), 1, 3) == 7
    # half above RANK_MAX_HALF: the unsupported code, raised as _lib.check raises every backend code; the data untouched
    m, v = fresh()
    for obj in (m, v):
        with pytest.raises(bd.BackendError, match="-102"):
            bd.rank_filter(obj, MAX_HALF + 1, 0)
        with pytest.raises(bd.BackendError, match="-102"):
            bd.medfilt(obj, 2 * MAX_HALF + 3)
    untouched(m, v)
    assert bd.rank_filter(m, MAX_HALF, 0) == 0 and bd.medfilt(v, 2 * MAX_HALF + 1) == 0  # the maximum itself is accepted
    # an empty vector, 0 x n and rows x 0 matrices: 0 and nothing changes
    ev = bd.DspVec(np.zeros(0, dtype))
    assert bd.rank_filter(ev, 2, 1) == 0 and bd.medfilt(ev) == 0 and len(ev) == 0
    for empty in (bd.DspMat(np.zeros((0, 8), dtype)), bd.DspMat(np.zeros((3, 0), dtype))):
        rows = empty.rows()
        assert bd.rank_filter(empty, 2, 1, boundary="wrap") == 0 and bd.medfilt(empty, 5, "nearest") == 0
        assert (empty.rows(), empty.row_len()) == (rows, 0 if rows else empty.row_len())
    # TypeError for anything that is not a DspVec or DspMat
    for bad in (x, [1.0, 2.0], None):
        with pytest.raises(TypeError):
            bd.rank_filter(bad, 1, 1)
        with pytest.raises(TypeError):
            bd.medfilt(bad)


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_domain_and_delta_stay_on_a_frequency_domain_real_matrix(bd, prec):
    dtype = PRECS[prec]
    x = np.abs(draw(21, 4, 300, dtype, "ties"))
    m, v = bd.DspMat(x, domain=1, delta=0.25), bd.DspVec(x[1].copy(), domain=1, delta=0.25)
    assert bd.rank_filter(m, 12, 17, guard=2, boundary="wrap") == 0 and bd.rank_filter(v, 12, 17, guard=2, boundary="wrap") == 0
    assert (m.rows(), m.row_len(), m.is_complex(), m.domain(), m.delta()) == (4, 300, False, 1, 0.25)
    assert (len(v), v.is_complex(), v.domain(), v.delta()) == (300, False, 1, 0.25)
    want = model(x, 12, 17, 2, "wrap")
    assert same_bits(m.data(), want) and same_bits(v.data(), want[1])
    # the call trades the buffers: a second call works on the first call's result
    assert bd.medfilt(m, 5, "nearest") == 0
    assert same_bits(m.data(), model(want.view(dtype), 2, 2, None, "nearest"))


def test_readme_despike_and_os_cfar_snippet(bd):
    """The README's snippet as written, on 8 pulses x 100 -> 256 points: correlate and magnitude, medfilt of 5 points, a
    copy that stays on the device (zeros plus the magnitudes), the OS-CFAR floor (the 24th smallest of 2 x 16 training
    cells, 2 guard cells a side, circular), scale, sub.  Every step is exact in f32 (a product with 4.0, one rounded
    subtraction), so the result equals the numpy model of the same steps bit for bit."""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "rank_filter(" in b]
    assert len(blocks) == 1
    code = blocks[0]
    for line in ("from basic_dsp_amd import medfilt, rank_filter", "medfilt(pulses, 5) == 0", "floor.add(pulses) == 0",
                 'rank_filter(floor, half=T + G, rank=k, guard=G, boundary="wrap") == 0', "floor.scale(alpha) == 0 and pulses.sub(floor) == 0"):
        assert line in code, line
    rng = np.random.default_rng(5)
    x = rng.random((8, 2 * 100)).astype(np.float32)
    t = rng.random(2 * 100).astype(np.float32)

    def operands():
        pulses, template = bd.DspMat(x, is_complex=True), bd.DspVec(t, is_complex=True)
        assert template.zero_pad(256, 1) == 0 and template.prepare_argument() == 0
        return pulses, template

    ref, template = operands()
    assert ref.correlate(template) == 0 and ref.magnitude() == 0
    mags = ref.data()
    assert mags.shape == (8, 256)
    pulses, template = operands()
    env = {"np": np, "DspVec": bd.DspVec, "DspMat": bd.DspMat, "pulses": pulses, "template": template}
    exec(code, env)
    despiked = model(mags, 2, 2, None, "zero").view(np.float32)
    floor = model(despiked, 18, 24, 2, "wrap").view(np.float32)
    want = despiked - floor * np.float32(4.0)
    assert same_bits(env["floor"].data(), bits(floor * np.float32(4.0)))
    assert same_bits(pulses.data(), bits(want))
    assert (pulses.rows(), pulses.row_len(), pulses.is_complex()) == (8, 256, False)
