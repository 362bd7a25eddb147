"""sort, argsort, top_k, quantile and median: the order statistics of a DspVec or of every row of a DspMat on the device,
through the Python functions.

Every output is one of the input values or an index, so every comparison is equality: of the bit patterns (view(uint)) for
values, of integers for indices, of float64 for the quantiles (one line of double arithmetic on two selected values, done
the same way here).  The numpy model is written here: key(a) = the uint view with the key map of IEEE totalOrder (-NaN <
-inf < ... < -0 < +0 < ... < +inf < +NaN); ascending is np.argsort(key, kind="stable"), descending is np.argsort(~key,
kind="stable").  The shapes are tests/sort_shapes.txt, which the host simulation (tests/host_sim/sim_sort.cpp) reads too;
each line runs in f32 and f64, in both directions, on six classes of data."""
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = [np.float32, np.float64]
PREC_IDS = ["f32", "f64"]
KINDS = ["uniform", "ties16", "equal", "sorted", "reversed", "edge"]
QS = [0.0, 0.1, 0.25, 0.5, 0.9, 0.999, 1.0]
METHODS = ["linear", "lower", "higher"]


def read_shapes():
    out = []
    with open(os.path.join(ROOT, "tests", "sort_shapes.txt")) as f:
        for line in f:
            w = line.split("#")[0].split()
            if w:
                out.append((int(w[0]), int(w[1])))
    return out


SHAPES = read_shapes()
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]


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


def special_bits(dtype):
    """+-0, +-inf, +-NaN (quiet, signalling, with distinct payloads), +-denormals, +-max, as bit patterns"""
    u = uint_of(dtype)
    e, m = (8, 23) if u == np.uint32 else (11, 52)
    emax, mmax, quiet = (1 << e) - 1, (1 << m) - 1, 1 << (m - 1)
    pos = [0, 1, 77, mmax, ((emax - 1) << m) | mmax, emax << m, (emax << m) | 1, (emax << m) | quiet, (emax << m) | quiet | 12345,
           (emax << m) | mmax]
    return np.array(pos + [p | (1 << (e + m)) for p in pos], dtype=u)


def draw(seed, rows, n, dtype, kind):
    rng = np.random.default_rng(seed)
    if kind == "ties16":
        return ((rng.integers(0, 16, (rows, n)) - 8) * 0.25).astype(dtype)  # 16 values, -0 never, +0 among them
    if kind == "equal":
        return np.full((rows, n), 1.5, dtype)
    x = rng.standard_normal((rows, n)).astype(dtype)
    if kind == "sorted":
        return np.sort(x, axis=1)
    if kind == "reversed":
        return np.ascontiguousarray(np.sort(x, axis=1)[:, ::-1])
    if kind == "edge":
        sp = special_bits(dtype)
        mask = rng.random((rows, n)) < 0.5
        b = bits(x).copy()
        b[mask] = sp[rng.integers(0, len(sp), int(mask.sum()))]
        return b.view(dtype)
    return x


def model_order(x, descending):
    key = to_keys(bits(x))
    return np.argsort(~key if descending else key, axis=1, kind="stable")


@functools.lru_cache(maxsize=None)
def case(line, prec, kind):
    """(x, ascending permutation, descending permutation) of a shapes line: computed once, shared and never written to"""
    rows, n = SHAPES[line]
    x = draw(9000 + 13 * line + prec, rows, n, PRECS[prec], kind)
    out = (x, model_order(x, False), model_order(x, True))
    for a in out:
        a.setflags(write=False)
    return out


def take(x, order):
    return np.take_along_axis(bits(x), order, axis=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
@pytest.mark.parametrize("line", range(len(SHAPES)), ids=SHAPE_IDS)
def test_every_shape_line_equals_the_model(bd, line, prec, kind):
    rows, n = SHAPES[line]
    x, asc, desc = case(line, prec, kind)
    src = bd.DspMat(x, delta=0.5)
    for descending, order in ((False, asc), (True, desc)):
        want = take(x, order)
        m = bd.DspMat(x, delta=0.5)
        assert bd.sort(m, descending) == 0
        assert (m.rows(), m.row_len(), m.is_complex(), m.domain(), m.delta()) == (rows, n, False, 0, 0.5)
        got = bits(m.data())
        assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5]
        code, index = bd.argsort(src, descending)
        assert code == 0 and index.dtype == np.int64 and index.shape == (rows, n)
        assert np.array_equal(index, order), np.argwhere(index != order)[:5]
        for k in sorted({1, min(n, 8), n}):
            code, top = bd.top_k(src, k, largest=descending)
            assert code == 0 and top["index"].dtype == np.int64 and top["value"].dtype == x.dtype
            assert top["index"].shape == (rows, k) and top["value"].shape == (rows, k)
            assert np.array_equal(top["index"], order[:, :k]) and np.array_equal(bits(top["value"]), want[:, :k])
    assert np.array_equal(bits(src.data()), bits(x))  # x is untouched
    # the vector call on the last row: the same bits and indices
    v = bd.DspVec(x[rows - 1].copy(), delta=0.5)
    code, index = bd.argsort(v, True)
    assert code == 0 and index.shape == (n,) and np.array_equal(index, desc[rows - 1])
    code, top = bd.top_k(v, min(n, 8))
    assert code == 0 and top["index"].shape == (min(n, 8),) and np.array_equal(top["index"], desc[rows - 1][:min(n, 8)])
    assert np.array_equal(bits(top["value"]), take(x, desc)[rows - 1][:min(n, 8)])
    assert np.array_equal(bits(v.data()), bits(x[rows - 1]))
    assert bd.sort(v) == 0 and (len(v), v.is_complex(), v.domain(), v.delta()) == (n, False, 0, 0.5)
    assert np.array_equal(bits(v.data()), take(x, asc)[rows - 1])


def test_the_model_orders_the_edge_values_as_totalorder_does():
    x = np.array([[np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0]], dtype=np.float32)
    x = (bits(x) | np.array([[0, 0x80000000, 0, 0, 0, 0, 0, 0]], dtype=np.uint32)).view(np.float32)  # (the sign of -nan, whatever numpy made)
    assert list(model_order(x, False)[0]) == [1, 3, 7, 5, 4, 6, 2, 0] and list(model_order(x, True)[0]) == [0, 2, 6, 4, 5, 7, 3, 1]


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_every_row_equals_the_vector_call_and_does_not_depend_on_the_row_count(bd, prec):
    dtype = PRECS[prec]
    for n in (65, 100, 2049, 4097, 8209):
        x = draw(77 + n, 7, n, dtype, "ties16")
        code, whole = bd.argsort(bd.DspMat(x))
        assert code == 0
        m = bd.DspMat(x)
        assert bd.sort(m, True) == 0
        sorted_rows = bits(m.data())
        for r in (0, 3, 6):
            code, one = bd.argsort(bd.DspVec(x[r].copy()))
            assert code == 0 and np.array_equal(one, whole[r])
            code, alone = bd.argsort(bd.DspMat(x[r:r + 1].copy()))
            assert code == 0 and np.array_equal(alone[0], whole[r])
            v = bd.DspVec(x[r].copy())
            assert bd.sort(v, True) == 0 and np.array_equal(bits(v.data()), sorted_rows[r])


def model_quantile(v, q, method):
    """v: one sorted row (the model's order); the formula of the documentation, in Python floats (doubles)"""
    n = len(v)
    p = float(q) * float(n - 1)
    lo = int(np.floor(p))
    hi = min(lo + 1, n - 1)
    g = p - lo
    if method == "lower":
        return np.float64(v[lo])
    if method == "higher":
        return np.float64(v[int(np.ceil(p))])
    if g == 0.0 or bits(v[lo:lo + 1])[0] == bits(v[hi:hi + 1])[0]:
        return np.float64(v[lo])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float64(v[lo]) + (np.float64(v[hi]) - np.float64(v[lo])) * np.float64(g)


@pytest.mark.parametrize("kind", ["uniform", "ties16", "edge"])
@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_quantile_equals_the_exact_model(bd, prec, kind):
    dtype = PRECS[prec]
    for rows, n in ((1, 1), (7, 2), (7, 3), (7, 100), (3, 2049), (7, 4097), (1, 8209)):
        x = draw(500 + n, rows, n, dtype, kind)
        v = take(x, model_order(x, False)).view(dtype)
        m = bd.DspMat(x)
        for method in METHODS:
            code, got = bd.quantile(m, QS, method)
            assert code == 0 and got.dtype == np.float64 and got.shape == (rows, len(QS))
            want = np.array([[model_quantile(v[r], q, method) for q in QS] for r in range(rows)], dtype=np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (n, method)
            assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), (n, method)
        code, one = bd.quantile(m, 0.25)
        assert code == 0 and one.shape == (rows,)
        code, vec = bd.quantile(bd.DspVec(x[0].copy()), QS)
        assert code == 0 and vec.shape == (len(QS),)
        code, scalar = bd.quantile(bd.DspVec(x[0].copy()), 0.5, "lower")
        assert code == 0 and scalar.shape == () and (np.isnan(scalar) or scalar == model_quantile(v[0], 0.5, "lower"))
        code, med = bd.median(m)
        code2, half = bd.quantile(m, 0.5)
        assert code == 0 and code2 == 0 and np.array_equal(bits(med), bits(half))
        assert np.array_equal(bits(m.data()), bits(x))  # x is untouched


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_quantile_agrees_with_numpy_on_finite_data(bd, prec):
    """Both sides are one interpolation of the same two doubles: within 4 eps(f64) max(|v[lo]|, |v[hi]|)."""
    dtype = PRECS[prec]
    eps = np.finfo(np.float64).eps
    for rows, n in ((7, 1), (7, 2), (7, 100), (3, 2049), (7, 4097)):
        x = draw(900 + n, rows, n, dtype, "uniform")
        code, got = bd.quantile(bd.DspMat(x), QS)
        assert code == 0
        d = np.sort(x.astype(np.float64), axis=1)
        want = np.quantile(d, QS, axis=1).T
        worst = 0.0
        for j, q in enumerate(QS):
            lo = int(np.floor(q * (n - 1)))
            hi = min(lo + 1, n - 1)
            bound = 4 * eps * np.maximum(np.abs(d[:, lo]), np.abs(d[:, hi]))
            err = np.abs(got[:, j] - want[:, j])
            worst = max(worst, float((err / np.maximum(np.abs(d[:, lo]), np.abs(d[:, hi])) / eps).max()))
            assert np.all(err <= bound), (n, q, err.max(), bound.min())
        print("n = %d: largest difference from np.quantile %.2f eps" % (n, worst))


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_quantile_special_cases(bd, prec):
    dtype = PRECS[prec]
    x = draw(31, 5, 301, dtype, "uniform")
    code, med = bd.median(bd.DspMat(x))
    assert code == 0 and np.array_equal(med, np.sort(x, axis=1)[:, 150].astype(np.float64))  # odd n: the middle element's value
    code, med = bd.median(bd.DspVec(x[2].copy()))
    assert code == 0 and med.shape == () and med == np.float64(np.sort(x[2])[150])
    # a row whose top third is +NaN: a finite median, a NaN quantile(1.0); numpy would answer NaN for both
    y = x.copy()
    y[:, 201:] = np.nan
    y = (bits(y) & ~(uint_of(dtype)(1) << uint_of(dtype)(8 * y.itemsize - 1))).view(dtype)  # +NaN
    m = bd.DspMat(y)
    code, med = bd.median(m)
    assert code == 0 and np.all(np.isfinite(med)) and np.array_equal(med, np.sort(y[:, :201], axis=1)[:, 150].astype(np.float64))
    code, top = bd.quantile(m, 1.0)
    assert code == 0 and np.all(np.isnan(top))
    code, q = bd.quantile(m, [0.0, 0.66, 0.67, 1.0], "higher")
    assert code == 0 and np.array_equal(np.isnan(q), np.array([[False, False, True, True]] * 5))
    assert np.all(np.isnan(np.quantile(y.astype(np.float64), 0.5, axis=1)))


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
    x = draw(11, 3, 40, dtype, "edge")
    m, v = bd.DspMat(x), bd.DspVec(x[0].copy())

    def untouched(a=m, b=v):
        assert np.array_equal(bits(a.data()), bits(x)) and np.array_equal(bits(b.data()), bits(x[0]))

    # 7, the data untouched
    for obj in (m, v):
        assert bd.top_k(obj, 41) == (7, None) and bd.top_k(obj, -1) == (7, None) and bd.top_k(obj, 2.0) == (7, None)
        assert bd.top_k(obj, 3, largest="yes") == (7, None) and bd.sort(obj, descending=2) == 7 and bd.argsort(obj, None) == (7, None)
        for q in (-0.1, 1.5, float("nan"), [0.5, 2.0], "0.5", None, [[0.5]]):
            assert bd.quantile(obj, q) == (7, None), q
        assert bd.quantile(obj, 0.5, "nearest") == (7, None) and bd.quantile(obj, 0.5, None) == (7, None)
    untouched()
    # 7 at the C entry: a flag that is not 0 or 1, a rank at n, count above n without ranks
    ranks = np.array([0, 40], dtype=np.uint64)
    out = np.zeros(3 * 41, dtype=np.int64)
    select, sort = getattr(bd.lib, "bdsp_hip_mat_order_select" + m._sfx), getattr(bd.lib, "bdsp_hip_mat_sort" + m._sfx)
    assert sort(m._h, 2) == 7 and select(m._h, 2, 1, None, out.ctypes.data, None) == 7
    assert select(m._h, 0, 2, ranks.ctypes.data, out.ctypes.data, None) == 7 and select(m._h, 0, 41, None, out.ctypes.data, None) == 7
    assert not out.any()
    untouched()
    # ranks in any order, with repeats; index or value alone
    ranks = np.array([39, 0, 39, 5], dtype=np.uint64)
    index, value = np.zeros((3, 4), dtype=np.int64), np.zeros((3, 4), dtype=dtype)
    assert select(m._h, 1, 4, ranks.ctypes.data, index.ctypes.data, None) == 0 and select(m._h, 1, 4, ranks.ctypes.data, None, value.ctypes.data) == 0
    order = model_order(x, True)
    assert np.array_equal(index, order[:, [39, 0, 39, 5]]) and np.array_equal(bits(value), take(x, order)[:, [39, 0, 39, 5]])
    # k = 0: empty arrays
    code, top = bd.top_k(m, 0)
    assert code == 0 and top["index"].shape == (3, 0) and top["value"].shape == (3, 0) and top["value"].dtype == dtype
    code, top = bd.top_k(v, 0)
    assert code == 0 and top["index"].shape == (0,)
    # 4: complex data, untouched; an argument error comes first
    cm, cv = bd.DspMat(x, is_complex=True), bd.DspVec(x[0].copy(), is_complex=True)
    for obj in (cm, cv):
        assert bd.sort(obj) == 4 and bd.argsort(obj) == (4, None) and bd.top_k(obj, 3) == (4, None)
        assert bd.quantile(obj, 0.5) == (4, None) and bd.median(obj) == (4, None)
        assert bd.top_k(obj, 41) == (7, None) and bd.quantile(obj, 2.0) == (7, None)
    untouched(cm, cv)
    # -1: a poisoned x stays poisoned; an argument error comes first
    for make in (_poisoned_mat, _poisoned_vec):
        p = make(bd, dtype)
        assert bd.sort(p) == -1 and bd.sort(p, True) == -1 and bd.argsort(p) == (-1, None) and bd.top_k(p, 0) == (-1, None)
        assert bd.sort(p, 3) == 7 and bd.top_k(p, 1) == (7, None)
        assert bd.sort(p) == -1
    # empty vector, 0 x n and rows x 0 matrices: 0, nothing changes, empty arrays; a quantile of no points is 7
    ev = bd.DspVec(np.zeros(0, dtype))
    assert bd.sort(ev) == 0 and len(ev) == 0
    code, index = bd.argsort(ev)
    assert code == 0 and index.shape == (0,)
    assert bd.quantile(ev, 0.5) == (7, None) and bd.median(ev) == (7, None) and bd.top_k(ev, 1) == (7, None)
    for empty in (bd.DspMat(np.zeros((0, 8), dtype)), bd.DspMat(np.zeros((3, 0), dtype))):
        rows = empty.rows()
        assert bd.sort(empty, True) == 0 and empty.rows() == rows
        code, index = bd.argsort(empty)
        assert code == 0 and index.size == 0 and index.shape[0] == rows
        code, top = bd.top_k(empty, 0)
        assert code == 0 and top["index"].size == 0
        assert bd.quantile(empty, 0.5) == (7, None)
    # TypeError for anything that is not a DspVec or DspMat
    for bad in (x, [1.0, 2.0], None):
        for call in (lambda: bd.sort(bad), lambda: bd.argsort(bad), lambda: bd.top_k(bad, 1), lambda: bd.quantile(bad, 0.5),
                     lambda: bd.median(bad), lambda: bd.quantile(bad, 7.0, "no such method")):
            with pytest.raises(TypeError):
                call()


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_IDS)
def test_domain_and_delta_stay_and_sort_twice_is_idempotent(bd, prec):
    dtype = PRECS[prec]
    for n in (300, 4097, 8209):  # no merge pass, one (the result in the trade buffer), two
        x = np.abs(draw(21 + n, 4, n, dtype, "edge"))
        m, v = bd.DspMat(x, domain=1, delta=0.25), bd.DspVec(x[1].copy(), domain=1, delta=0.25)
        assert bd.sort(m) == 0 and bd.sort(v) == 0
        assert (m.rows(), m.row_len(), m.is_complex(), m.domain(), m.delta()) == (4, n, False, 1, 0.25)
        assert (len(v), v.is_complex(), v.domain(), v.delta()) == (n, False, 1, 0.25)
        once = bits(m.data())
        assert np.array_equal(once, take(x, model_order(x, False))) and np.array_equal(bits(v.data()), once[1])
        assert bd.sort(m) == 0 and np.array_equal(bits(m.data()), once)  # idempotent, and the call works on the traded buffer
        assert bd.sort(m, True) == 0 and np.array_equal(bits(m.data()), once[:, ::-1])  # descending: the bit-reverse of ascending
        d = bd.DspMat(x)
        assert bd.sort(d, True) == 0 and np.array_equal(bits(d.data()), once[:, ::-1])


def test_readme_robust_threshold_and_top_k_snippet(bd):
    """The README's snippet as written, on 64 pulses x 1000 -> 2048 points: the per-row median, a per-row threshold from it
    fed to detect as the README says, and the eight strongest cells per row.  The pulses are noise without a target, so the
    threshold factor is 1.25 here: some cells of every row pass."""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "median(" in b]
    assert len(blocks) == 1
    code = blocks[0]
    for line in ("from basic_dsp_amd import median, top_k", "code, med = median(pulses)", "threshold = alpha * med", "code, top = top_k(pulses, 8)"):
        assert line in code, line
    assert '`detect(pulses, threshold, order=1, boundary="wrap")`' in " ".join(text.split())
    rng = np.random.default_rng(5)
    x = rng.random((64, 2 * 1000)).astype(np.float32)
    t = rng.random(2 * 1000).astype(np.float32)
    pulses, template = bd.DspMat(x, is_complex=True), bd.DspVec(t, is_complex=True)
    assert template.zero_pad(2048, 1) == 0 and template.prepare_argument() == 0
    assert pulses.correlate(template) == 0 and pulses.magnitude() == 0
    mags = pulses.data()
    assert mags.shape == (64, 2048)
    env = {"np": np, "pulses": pulses, "alpha": 1.25}
    exec(code, env)
    assert env["code"] == 0
    s = np.sort(mags, axis=1)
    want_med = s[:, 1023].astype(np.float64) + (s[:, 1024].astype(np.float64) - s[:, 1023].astype(np.float64)) * 0.5
    assert np.array_equal(env["med"], want_med) and np.array_equal(env["threshold"], 1.25 * want_med)
    code, det = bd.detect(pulses, env["threshold"], order=1, boundary="wrap")
    assert code == 0
    mask = (mags.astype(np.float64) > env["threshold"][:, None]) & (mags > np.roll(mags, 1, 1)) & (mags > np.roll(mags, -1, 1))
    rows, cells = np.nonzero(mask)
    assert len(rows) > 64 and np.array_equal(det["row"], rows) and np.array_equal(det["index"], cells)
    order = model_order(mags, True)
    assert np.array_equal(env["top"]["index"], order[:, :8]) and np.array_equal(bits(env["top"]["value"]), take(mags, order)[:, :8])
    unique_max = (mags == mags.max(axis=1, keepdims=True)).sum(axis=1) == 1
    assert unique_max.sum() > 32
    assert np.array_equal(env["top"]["index"][unique_max, 0], pulses.statistics()["max_index"][unique_max])
    assert np.array_equal(bits(pulses.data()), bits(mags))  # x is untouched
