"""detect and argrelmax: the cells of a DspVec, or of every row of a DspMat, that stand above a threshold and are strict
local maxima, as one compact list in row-major order, through the Python functions.

Indices are integers and values are copied bits, so every comparison is equality (view(uint) for the values), never a
tolerance.  The numpy model is written here: the threshold comparison of the kind, then for every d with 0 < |d| <= order
the comparison x[j] > x[j + d] with the neighbour read by the boundary rule (open: skipped outside the row; wrap: index
mod n; nearest: the end point), all IEEE >, then np.nonzero.  The shapes are tests/detect_shapes.txt, which the host
simulation (tests/host_sim/sim_detect.cpp) reads too; each line runs in f32 and f64, on data with heavy ties (16 levels
of both signs, so plateaus and +-0 against a threshold of 0.0 occur) and on data seeded with +-0, +-inf, +-NaN with
payloads and denormals; the lines with a long order run on a ramp with a few spikes, so that peaks exist."""
import functools
import importlib
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = [np.float32, np.float64]
PREC_IDS = ["f32", "f64"]
KINDS = ("none", "scalar", "scalar-inf", "row", "profile", "cell")
ROW_THRESHOLDS = (-0.5, 0.0, 0.25, -1.0, 0.5, 0.0, -0.25)


def read_constants():
    with open(os.path.join(ROOT, "basic_dsp_amd", "csrc", "detect_core.h")) as f:
        return {k: int(v) for k, v in re.findall(r"^constexpr int (DETECT_\w+) = (\d+);", f.read(), re.M)}


def read_shapes():
    out = []
    with open(os.path.join(ROOT, "tests", "detect_shapes.txt")) as f:
        for line in f:
            w = line.split("#")[0].split()
            if w:
                assert w[3] in ("open", "wrap", "nearest") and w[4] in KINDS, line
                out.append((int(w[0]), int(w[1]), int(w[2]), w[3], w[4]))
    return out


K = read_constants()
TILE, MAX_ORDER, CHUNK = K["DETECT_TILE"], K["DETECT_MAX_ORDER"], K["DETECT_SCAN_CHUNK"]
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


def special_bits(dtype):
    """+-0, +-inf, +-NaN (quiet, signalling, with payloads), +-denormals, as bit patterns"""
    u = uint_of(dtype)
    e, m = (8, 23) if u == np.uint32 else (11, 52)
    emax, mmax, quiet = (1 << e) - 1, (1 << m) - 1, 1 << (m - 1)
    pos = [0, 1, 77, mmax, emax << m, (emax << m) | 1, (emax << m) | quiet, (emax << m) | quiet | 12345, (emax << m) | mmax]
    return np.array(pos + [p | (1 << (e + m)) for p in pos], dtype=u)


def draw(seed, rows, n, dtype, kind):
    """ties: 16 levels of both signs, -0 among them.  special: the same with three cells in ten replaced by a special bit
    pattern.  ramp: ascending, with a spike of its own height every 413 cells."""
    rng = np.random.default_rng(seed)
    if kind == "ramp":
        j = np.arange(n, dtype=np.float64)
        x = np.tile(j - n / 2, (rows, 1))
        spikes = np.arange(7, n, 413)
        x[:, spikes] += 5000.0 + spikes + np.arange(rows)[:, None]
        return x.astype(dtype)
    level = rng.integers(0, 16, (rows, n))
    x = ((level - 8) * 0.25).astype(dtype)
    x[(level == 8) & (rng.random((rows, n)) < 0.5)] = -0.0
    if kind == "special":
        sp = special_bits(dtype)
        mask = rng.random((rows, n)) < 0.3
        b = bits(x).copy()
        b[mask] = sp[rng.integers(0, len(sp), int(mask.sum()))]
        x = b.view(dtype)
    return x


def above(x, kind, t):
    """the threshold comparison of the kind: a bool array shaped like x"""
    with np.errstate(invalid="ignore"):
        if kind == "none":
            return np.ones(x.shape, bool)
        if kind in ("scalar", "scalar-inf"):
            return x.astype(np.float64) > np.float64(t)
        if kind == "row":
            return x.astype(np.float64) > np.asarray(t, np.float64)[:, None]
        if kind == "profile":
            return x > t[None, :]
        assert kind == "cell"
        return x > t


def model_mask(x, kind, t, order, boundary):
    rows, n = x.shape
    ok = above(x, kind, t)
    j = np.arange(n)
    with np.errstate(invalid="ignore"):
        for d in range(1, order + 1):
            for pos in (j - d, j + d):
                if boundary == "open":
                    inside = (pos >= 0) & (pos < n)
                    ok &= (x > x[:, np.clip(pos, 0, n - 1)]) | ~inside[None, :]
                elif boundary == "wrap":
                    ok &= x > x[:, pos % n]
                else:
                    assert boundary == "nearest"
                    ok &= x > x[:, np.clip(pos, 0, n - 1)]
    return ok


def model(x, kind, t, order, boundary):
    """(count[rows], row[k], index[k]) in row-major order"""
    mask = model_mask(x, kind, t, order, boundary)
    row, index = np.nonzero(mask)
    return mask.sum(axis=1).astype(np.int64), row.astype(np.int64), index.astype(np.int64)


def empty_by_construction(n, order, boundary):
    """wrap with order >= n compares every cell with itself.  nearest blocks the two end points only (a cell in between is
    never compared with itself, whatever the order), so it is empty by construction for rows of one or two points."""
    return (boundary == "wrap" and order >= n) or (boundary == "nearest" and order >= 1 and n <= 2)


def threshold_of(line, prec, data, rows, n, kind):
    """the host form of a line's threshold: None, a float, a list of rows floats, an array of n or of rows x n"""
    dtype = PRECS[prec]
    if kind == "none":
        return None
    if kind == "scalar":
        return 0.0
    if kind == "scalar-inf":
        return -np.inf
    if kind == "row":
        return [ROW_THRESHOLDS[r % len(ROW_THRESHOLDS)] for r in range(rows)]
    t = draw(9000 + 7 * line + prec, 1 if kind == "profile" else rows, n, dtype, "special" if data == "special" else "ties")
    return t[0].copy() if kind == "profile" else t


@functools.lru_cache(maxsize=None)
def case(line, prec, data):
    """(x, t, (count, row, index)) of a shapes line: computed once, shared and never written to"""
    rows, n, order, boundary, kind = SHAPES[line]
    x = draw(4000 + 7 * line + prec, rows, n, PRECS[prec], "ramp" if order > 64 else data)
    t = threshold_of(line, prec, data, rows, n, kind)
    if order <= 64:  # one certain peak at the start of row 0, so that a line of few cells cannot be empty by chance
        k = min(n, 3)
        x[0, :k] = ((3.0,), (-1.0, 3.0), (-1.0, 3.0, -1.0))[k - 1]
        if kind == "profile":
            t[:k] = -2.0
        elif kind == "cell":
            t[0, :k] = -2.0
    want = model(x, kind, t, order, boundary)
    for a in (x,) + want + ((t,) if isinstance(t, np.ndarray) else ()):
        a.setflags(write=False)
    return x, t, want


def device_threshold(bd, kind, t):
    """the argument of detect for a host threshold (kept alive by the caller); a device operand carries the data's delta"""
    if kind == "profile":
        return bd.DspVec(np.array(t), delta=0.5)
    if kind == "cell":
        return bd.DspMat(np.array(t), delta=0.5)
    return t


def check_matrix(det, x, want):
    count, row, index = want
    assert set(det) == {"count", "row", "index", "value"}
    assert det["count"].dtype == np.int64 and det["row"].dtype == np.int64 and det["index"].dtype == np.int64 and det["value"].dtype == x.dtype
    assert np.array_equal(det["count"], count)
    assert np.array_equal(det["row"], row) and np.array_equal(det["index"], index)
    assert np.array_equal(bits(det["value"]), bits(x[row, index]))


def check_vector(det, xrow, count, index):
    assert set(det) == {"count", "index", "value"} and isinstance(det["count"], int)
    assert det["count"] == count and det["index"].dtype == np.int64 and det["value"].dtype == xrow.dtype
    assert np.array_equal(det["index"], index) and np.array_equal(bits(det["value"]), bits(xrow[index]))


@pytest.mark.parametrize("data", ["ties", "special"])
@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
@pytest.mark.parametrize("line", range(len(SHAPES)), ids=SHAPE_IDS)
def test_every_shape_line_equals_the_model(bd, line, prec, data):
    rows, n, order, boundary, kind = SHAPES[line]
    x, t, want = case(line, prec, data)
    count, row, index = want
    # an empty list cannot pass by accident
    if empty_by_construction(n, order, boundary):
        assert count.sum() == 0
    else:
        assert count.sum() > 0, "the model finds nothing on this line"
    if kind == "scalar-inf" and order == 0:
        assert count.sum() == int((~np.isnan(x) & ~(np.isinf(x) & (x < 0))).sum())  # dense: every cell but NaN and -inf
    m = bd.DspMat(x, delta=0.5)
    keep = device_threshold(bd, kind, t)
    code, det = bd.detect(m, keep, order, boundary)
    assert code == 0
    check_matrix(det, x, want)
    assert (m.rows(), m.row_len(), m.is_complex(), m.domain(), m.delta()) == (rows, n, False, 0, 0.5)
    # the vector call on the last row gives that row's list
    last = rows - 1
    v = bd.DspVec(x[last].copy(), delta=0.5)
    tv = t[last] if kind == "row" else bd.DspVec(np.array(t[last]), delta=0.5) if kind == "cell" else keep
    code, dv = bd.detect(v, tv, order=order, boundary=boundary)
    assert code == 0
    check_vector(dv, x[last], int(count[last]), index[row == last])
    if kind == "row":  # a sequence of one number on a vector means one value
        code, dv = bd.detect(v, [t[last]], order, boundary)
        assert code == 0
        check_vector(dv, x[last], int(count[last]), index[row == last])


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_every_row_equals_the_vector_call_and_seven_equal_rows_equal_one(bd, prec):
    dtype = PRECS[prec]
    for n, order, boundary in ((2 * TILE + 17, 2, "wrap"), (TILE + 1, 1, "nearest"), (3, 1, "open")):
        x = draw(90 + n, 7, n, dtype, "special")
        count, row, index = model(x, "scalar", -0.25, order, boundary)
        code, det = bd.detect(bd.DspMat(x), -0.25, order, boundary)
        assert code == 0
        check_matrix(det, x, (count, row, index))
        for r in range(7):
            code, dv = bd.detect(bd.DspVec(x[r].copy()), -0.25, order, boundary)
            assert code == 0
            check_vector(dv, x[r], int(count[r]), index[row == r])
            assert np.array_equal(dv["index"], det["index"][det["row"] == r])
            assert np.array_equal(bits(dv["value"]), bits(det["value"][det["row"] == r]))
        same = np.tile(x[3], (7, 1))
        code7, d7 = bd.detect(bd.DspMat(same), -0.25, order, boundary)
        code1, d1 = bd.detect(bd.DspMat(same[:1]), -0.25, order, boundary)
        assert code7 == 0 and code1 == 0 and d1["count"][0] == count[3]
        assert np.array_equal(d7["count"], np.repeat(d1["count"], 7))
        assert np.array_equal(d7["index"], np.tile(d1["index"], 7)) and np.array_equal(bits(d7["value"]), np.tile(bits(d1["value"]), 7))
        assert np.array_equal(d7["row"], np.repeat(np.arange(7), d1["count"][0]))


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_per_row_and_per_cell_thresholds(bd, prec):
    dtype = PRECS[prec]
    n = TILE + 1
    x = draw(31, 7, n, dtype, "special")
    m = bd.DspMat(x)
    # a per-row list with a NaN and a +inf entry: those rows are empty
    t = [0.0, np.nan, -0.5, np.inf, 0.25, -np.inf, 0.0]
    for arg in (t, np.array(t), np.array(t, np.float32), tuple(t)):
        code, det = bd.detect(m, arg)
        assert code == 0
        check_matrix(det, x, model(x, "row", t, 0, "open"))
        assert det["count"][1] == 0 and det["count"][3] == 0 and det["count"][0] > 0 and det["count"][5] > 0
    # a matrix threshold equal to x detects nothing
    code, det = bd.detect(m, bd.DspMat(x))
    assert code == 0 and det["count"].sum() == 0 and det["index"].size == 0 and det["row"].size == 0 and det["value"].size == 0
    code, det = bd.detect(m, m)  # the same object
    assert code == 0 and det["count"].sum() == 0
    # one ulp below x: everything that is not NaN or -inf
    below = np.nextafter(x, dtype(-np.inf))
    code, det = bd.detect(m, bd.DspMat(below))
    assert code == 0
    everything = ~np.isnan(x) & ~(np.isinf(x) & (x < 0))
    assert det["count"].sum() == everything.sum() > 0
    check_matrix(det, x, model(x, "cell", below, 0, "open"))
    assert np.array_equal(np.stack([det["row"], det["index"]]), np.stack(np.nonzero(everything)))
    # a profile: one vector for all rows; -0 is not above +0
    zeros = np.zeros(n, dtype)
    code, det = bd.detect(m, bd.DspVec(zeros), 1, "wrap")
    assert code == 0
    check_matrix(det, x, model(x, "profile", zeros, 1, "wrap"))
    assert not np.any(bits(det["value"]) == bits(np.array([-0.0], dtype))[0])
    # a scalar threshold is compared in double: a float32 cell against a double between two float32 values
    if dtype == np.float32:
        y = np.array([[1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 0.5]], np.float32)
        code, det = bd.detect(bd.DspMat(y), 1.0 + 2.0 ** -30)
        assert code == 0 and det["index"].tolist() == [1]


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_capacity(bd, prec, monkeypatch):
    dtype = PRECS[prec]
    n = 2 * TILE + 17
    x = draw(57, 7, n, dtype, "ties")
    count, row, index = model(x, "scalar", 0.0, 1, "open")
    total = int(count.sum())
    # a cut inside tile 1 of row 3, inside a wave's 64 cells
    cut = TILE + 100
    seg = (cut // 64) * 64
    in_row = index[row == 3]
    assert np.any((in_row >= seg) & (in_row < cut)) and np.any((in_row >= cut) & (in_row < seg + 64))
    inside = int(count[:3].sum() + (in_row < cut).sum())
    m, v = bd.DspMat(x), bd.DspVec(x[3].copy())
    for capacity in (0, 1, total - 1, total, total + 5, inside, 10 ** 15):
        code, det = bd.detect(m, 0.0, 1, "open", capacity)
        assert code == 0
        k = min(capacity, total)
        assert np.array_equal(det["count"], count)  # the counts stay true
        assert det["row"].shape == det["index"].shape == det["value"].shape == (k,)
        assert np.array_equal(det["row"], row[:k]) and np.array_equal(det["index"], index[:k])
        assert np.array_equal(bits(det["value"]), bits(x[row[:k], index[:k]]))
    for capacity in (0, int((in_row < cut).sum()), int(count[3]) + 5):
        code, dv = bd.detect(v, 0.0, 1, "open", capacity=capacity)
        assert code == 0 and dv["count"] == count[3] and np.array_equal(dv["index"], in_row[:capacity])
    # capacity=None returns everything, also where the first call's lists are too short
    module = importlib.import_module("basic_dsp_amd.detect")
    assert module.FIRST_CAPACITY == 65536
    monkeypatch.setattr(module, "FIRST_CAPACITY", 5)
    code, det = bd.detect(m, 0.0, 1, "open")
    assert code == 0 and total > 5
    check_matrix(det, x, (count, row, index))
    code, dv = bd.detect(v, 0.0, 1)
    assert code == 0
    check_vector(dv, x[3], int(count[3]), in_row)
    # at the C entry: capacity 0 with NULL lists writes the counts only
    import ctypes as C
    counts = np.full(7, -1, np.int64)
    assert getattr(bd.lib, "bdsp_hip_mat_detect" + m._sfx)(m._h, 0, None, 1, 0, 0, counts.ctypes.data_as(C.c_void_p), None, None) == 0
    assert np.array_equal(counts, model(x, "none", None, 1, "open")[0])


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_argrelmax_equals_scipy(bd, prec):
    signal = pytest.importorskip("scipy.signal")
    dtype = PRECS[prec]
    x = draw(3, 3, TILE + 1, dtype, "ties")
    rng = np.random.default_rng(8)
    x[rng.random(x.shape) < 0.05] = np.nan
    x[rng.random(x.shape) < 0.05] = np.inf
    x[rng.random(x.shape) < 0.03] = -np.inf
    m, v = bd.DspMat(x), bd.DspVec(x[2].copy())
    found = 0
    for order in (1, 2, 5):
        for mode in ("clip", "wrap"):
            with np.errstate(invalid="ignore"):
                want = signal.argrelmax(x, axis=-1, order=order, mode=mode)
                want_row = signal.argrelmax(x[2], order=order, mode=mode)
            code, got = bd.argrelmax(m, order, mode)
            assert code == 0 and len(got) == 2
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (order, mode)
            code, got = bd.argrelmax(v, order=order, mode=mode)
            assert code == 0 and len(got) == 1 and np.array_equal(got[0], want_row[0])
            found += len(want[0])
    assert found > 0
    code, got = bd.argrelmax(v)  # the defaults: order 1, mode "clip"
    assert code == 0 and np.array_equal(got[0], signal.argrelmax(x[2])[0])
    for bad in ((0, "clip"), (-1, "clip"), (1.0, "clip"), (1, "nearest"), (1, None)):
        assert bd.argrelmax(m, *bad) == (7, None) and bd.argrelmax(v, *bad) == (7, None)


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_x_and_the_operand_are_untouched_in_any_domain(bd, prec):
    dtype = PRECS[prec]
    x = draw(21, 4, 300, dtype, "special")
    t = draw(22, 4, 300, dtype, "special")
    m, tm = bd.DspMat(x, domain=1, delta=0.25), bd.DspMat(t, domain=1, delta=0.25)
    v, tv = bd.DspVec(x[1].copy(), domain=1, delta=0.25), bd.DspVec(t[1].copy(), domain=1, delta=0.25)
    code, det = bd.detect(m, tm, 2, "wrap")
    assert code == 0
    check_matrix(det, x, model(x, "cell", t, 2, "wrap"))
    code, dv = bd.detect(v, tv, 2, "wrap")
    want = model(x[1:2], "profile", t[1], 2, "wrap")
    assert code == 0
    check_vector(dv, x[1], int(want[0][0]), want[2])
    code, det = bd.detect(m, tv, 1, "nearest")
    assert code == 0
    check_matrix(det, x, model(x, "profile", t[1], 1, "nearest"))
    assert (m.rows(), m.row_len(), m.is_complex(), m.domain(), m.delta()) == (4, 300, False, 1, 0.25)
    assert (tm.rows(), tm.row_len(), tm.is_complex(), tm.domain(), tm.delta()) == (4, 300, False, 1, 0.25)
    assert (len(v), v.is_complex(), v.domain(), v.delta()) == (300, False, 1, 0.25)
    assert (len(tv), tv.is_complex(), tv.domain(), tv.delta()) == (300, False, 1, 0.25)
    assert np.array_equal(bits(m.data()), bits(x)) and np.array_equal(bits(tm.data()), bits(t))
    assert np.array_equal(bits(v.data()), bits(x[1])) and np.array_equal(bits(tv.data()), bits(t[1]))


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
    import ctypes as C
    dtype = PRECS[prec]
    x = draw(11, 3, 40, dtype, "special")
    m, v = bd.DspMat(x), bd.DspVec(x[0].copy())
    mfn, vfn = getattr(bd.lib, "bdsp_hip_mat_detect" + m._sfx), getattr(bd.lib, "bdsp_hip_detect" + v._sfx)
    counts, index, value = np.full(3, -7, np.int64), np.full(8, -7, np.int64), np.full(8, 7, dtype)
    pc, pi, pv = (a.ctypes.data_as(C.c_void_p) for a in (counts, index, value))
    one = np.array([0.0])
    pt = one.ctypes.data_as(C.c_void_p)

    def nothing_written():
        assert np.all(counts == -7) and np.all(index == -7) and np.all(value == 7)

    # 7, with nothing written: an unknown kind or boundary, a NULL counts, NULL lists with capacity > 0, a NULL threshold
    # of a kind that has one, kind 4 on a vector
    for fn, h in ((mfn, m._h), (vfn, v._h)):
        for kind in (-1, 5, 99):
            assert fn(h, kind, pt, 0, 0, 8, pc, pi, pv) == 7
        for boundary in (-1, 3, 99):
            assert fn(h, 0, None, 0, boundary, 8, pc, pi, pv) == 7
        assert fn(h, 0, None, 0, 0, 8, None, pi, pv) == 7
        assert fn(h, 0, None, 0, 0, 8, pc, None, pv) == 7 and fn(h, 0, None, 0, 0, 8, pc, pi, None) == 7
        for kind in (1, 2, 3, 4):
            assert fn(h, kind, None, 0, 0, 8, pc, pi, pv) == 7
        nothing_written()
    assert vfn(v._h, 4, C.c_void_p(m._h), 0, 0, 8, pc, pi, pv) == 7
    nothing_written()
    assert bd.detect(v, m) == (7, None)
    # the Python side: 7 for an argument that is no index, a negative one, an unknown boundary, a sequence of the wrong length
    for obj in (m, v):
        for kwargs in ({"order": -1}, {"order": 1.0}, {"order": "1"}, {"capacity": -1}, {"capacity": 2.5}, {"boundary": "zero"},
                       {"boundary": 0}, {"boundary": None}, {"threshold": [0.0, 1.0]}, {"threshold": np.zeros(5)}, {"threshold": np.zeros((3, 1))}):
            assert bd.detect(obj, **kwargs) == (7, None), kwargs
    # an argument error comes before everything else
    cm, cv = bd.DspMat(x, is_complex=True), bd.DspVec(x[0].copy(), is_complex=True)
    assert bd.detect(_poisoned_mat(bd, dtype), boundary="?") == (7, None) and bd.detect(cm, order=-1) == (7, None)
    assert mfn(_poisoned_mat(bd, dtype)._h, 9, None, 0, 0, 8, pc, pi, pv) == 7 and mfn(cm._h, 0, None, 0, 9, 8, pc, pi, pv) == 7
    # -1: a poisoned x, a poisoned operand; before the number kind
    assert bd.detect(_poisoned_mat(bd, dtype)) == (-1, None) and bd.detect(_poisoned_vec(bd, dtype), 0.0, 1) == (-1, None)
    assert bd.detect(m, _poisoned_mat(bd, dtype)) == (-1, None) and bd.detect(m, _poisoned_vec(bd, dtype)) == (-1, None)
    assert bd.detect(v, _poisoned_vec(bd, dtype)) == (-1, None)
    assert bd.detect(cm, _poisoned_mat(bd, dtype)) == (-1, None) and bd.detect(_poisoned_mat(bd, dtype), cm) == (-1, None)
    assert bd.argrelmax(_poisoned_mat(bd, dtype)) == (-1, None)
    # 4: a complex x, a complex operand; before the size and meta-data checks
    assert bd.detect(cm) == (4, None) and bd.detect(cv, 0.0) == (4, None) and bd.argrelmax(cv) == (4, None)
    assert bd.detect(m, cm) == (4, None) and bd.detect(m, cv) == (4, None) and bd.detect(v, cv) == (4, None)
    assert bd.detect(m, bd.DspMat(x[:2], is_complex=True)) == (4, None)
    # the codes of add for an operand of another size (7 for the row count, then 1) or other meta data (2), in add's order
    other_rows, other_len = bd.DspMat(x[:2]), bd.DspMat(np.ascontiguousarray(x[:, :39]))
    assert bd.detect(m, other_rows) == (7, None) and m.add(other_rows) == 7
    assert bd.detect(m, other_len) == (1, None) and bd.DspMat(x).add(other_len) == 1
    assert bd.detect(m, bd.DspVec(x[0, :39].copy())) == (1, None) and bd.detect(v, bd.DspVec(x[0, :39].copy())) == (1, None)
    for meta in ({"domain": 1}, {"delta": 2.0}):
        assert bd.detect(m, bd.DspMat(x, **meta)) == (2, None) and bd.DspMat(x).add(bd.DspMat(x, **meta)) == 2
        assert bd.detect(m, bd.DspVec(x[0].copy(), **meta)) == (2, None) and bd.detect(v, bd.DspVec(x[0].copy(), **meta)) == (2, None)
    assert bd.detect(m, bd.DspMat(np.ascontiguousarray(x[:, :39]), domain=1)) == (1, None)  # the size before the meta data
    # an operand of the other precision: 2, before any device call
    other = np.float64 if dtype == np.float32 else np.float32
    assert bd.detect(m, bd.DspMat(x.astype(other))) == (2, None) and bd.detect(v, bd.DspVec(x[0].astype(other))) == (2, None)
    # order above DETECT_MAX_ORDER: the unsupported code, raised as _lib.check raises every backend code; after the others
    for obj in (m, v):
        with pytest.raises(bd.BackendError, match="-102"):
            bd.detect(obj, None, MAX_ORDER + 1)
        with pytest.raises(bd.BackendError, match="-102"):
            bd.argrelmax(obj, MAX_ORDER + 1)
        code, det = bd.detect(obj, None, MAX_ORDER, "open")  # the maximum itself is accepted
        assert code == 0
    assert bd.detect(cm, None, MAX_ORDER + 1) == (4, None) and bd.detect(m, other_len, MAX_ORDER + 1) == (1, None)
    assert np.array_equal(bits(m.data()), bits(x)) and np.array_equal(bits(v.data()), bits(x[0]))
    # an empty vector, 0 x n and rows x 0 matrices: 0, zero counts, empty lists
    code, det = bd.detect(bd.DspVec(np.zeros(0, dtype)), 0.0, 1)
    assert code == 0 and det["count"] == 0 and det["index"].shape == (0,) and det["value"].shape == (0,) and det["value"].dtype == dtype
    for empty, rows in ((bd.DspMat(np.zeros((0, 8), dtype)), 0), (bd.DspMat(np.zeros((3, 0), dtype)), 3)):
        code, det = bd.detect(empty, None, 2, "wrap", capacity=4)
        assert code == 0 and det["count"].shape == (rows,) and not det["count"].any()
        assert det["row"].shape == det["index"].shape == det["value"].shape == (0,)
        code, got = bd.argrelmax(empty)
        assert code == 0 and got[0].shape == got[1].shape == (0,)
    counts[:] = -7
    empty = bd.DspMat(np.zeros((3, 0), dtype))
    assert mfn(empty._h, 0, None, 0, 0, 0, pc, None, None) == 0 and np.all(counts == 0)
    # TypeError for an x that is not a DspVec or DspMat and for a threshold of no known kind
    for bad in (x, [1.0, 2.0], None, 1.0):
        with pytest.raises(TypeError):
            bd.detect(bad)
        with pytest.raises(TypeError):
            bd.argrelmax(bad)
    for bad in ("0.0", b"1", {"t": 1.0}, 1j, [1j], ["a"], True, object()):
        with pytest.raises(TypeError):
            bd.detect(m, bad)
        with pytest.raises(TypeError):
            bd.detect(v, bad, order=-1)  # (the type comes before the arguments)


def test_readme_detection_snippet(bd):
    """The README's snippet as written, after the steps of the OS-CFAR snippet before it up to the floor, on 8 pulses x 100
    -> 256 points: scale the floor, detect the cells above it that are circular local maxima; compared with np.nonzero of
    the numpy model of the same steps (one rounded f32 product on both sides).  The pulses are noise without a target, so
    the threshold factor is 1.25 here, not the 4.0 of the snippet before: a few cells of noise then pass, and the list is
    not empty."""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "detect(" in b]
    assert len(blocks) == 1
    code = blocks[0]
    for line in ("from basic_dsp_amd import detect", "floor.scale(alpha) == 0", 'code, det = detect(pulses, floor, order=1, boundary="wrap")'):
        assert line in code, line
    rng = np.random.default_rng(5)
    x = rng.random((8, 2 * 100)).astype(np.float32)
    t = rng.random(2 * 100).astype(np.float32)
    pulses, template = bd.DspMat(x, is_complex=True), bd.DspVec(t, is_complex=True)
    assert template.zero_pad(256, 1) == 0 and template.prepare_argument() == 0
    assert pulses.correlate(template) == 0 and pulses.magnitude() == 0
    assert bd.medfilt(pulses, 5) == 0
    floor = bd.DspMat(rows=pulses.rows(), row_len=pulses.row_len())
    assert floor.add(pulses) == 0
    assert bd.rank_filter(floor, half=18, rank=24, guard=2, boundary="wrap") == 0
    mags, level = pulses.data(), floor.data()
    assert mags.shape == (8, 256)
    env = {"np": np, "DspVec": bd.DspVec, "DspMat": bd.DspMat, "pulses": pulses, "floor": floor, "alpha": 1.25}
    exec(code, env)
    assert env["code"] == 0
    want = model(mags, "cell", level * np.float32(1.25), 1, "wrap")
    assert want[0].sum() > 0
    check_matrix(env["det"], mags, want)
    rows, cells = np.nonzero(model_mask(mags, "cell", level * np.float32(1.25), 1, "wrap"))
    assert np.array_equal(env["det"]["row"], rows) and np.array_equal(env["det"]["index"], cells)
    assert np.array_equal(bits(pulses.data()), bits(mags))  # x is untouched
