"""The module-level functions (zoom_fft, matmul, cholesky, cholesky_solve, eigh, sosfilt, rank_filter, medfilt, detect,
argrelmax, sort, argsort, top_k, quantile, median) on objects with a history.  Their own test files build a fresh upload,
call once and compare; here the DspMat or DspVec has been shrunk, transposed on the device, filled to its allocation's last
scalar, regrown, moved between the number spaces or traded between its two buffers first.

  * a. test_module_sequences_*: generated sequences of 16 steps (tests/module_model.py: movers of mat_model / vec_model and
    the in-place module operations with an exact model: sort, medfilt, rank_filter) from real start data, half of it edge
    values (plain noise where the sequence holds overlap_add, which adds).  After EVERY step code, metadata, delta and data bits equal the model's; then the read-only functions (argsort,
    top_k, quantile, detect, argrelmax) run on the state, equal the model's answers and leave metadata, bits and
    device_ptr() as they were: "x is not modified" includes not trading its buffers.
  * b. test_module_results_owe_nothing_to_history: every MODULE_CATALOGUE entry on every dirty state of mm.DIRTY /
    vm.DIRTY, on the long states of module_model (rows of more than one tile), on the Hermitian states (linalg) and on a
    fresh upload of the same values: equal codes, metadata, deltas and bits of the object and of everything returned -- no
    tolerance: none of sort.hip, rank_filter.hip, detect.hip, iir.hip, zoom_fft.hip, mat_mul.hip, mat_chol.hip, mat_eigh.hip
    uses an atomic.  The fresh result is held to the function's own reference once per entry, with the bound of the
    function's own test, taken by calling that test's helper or quoted with file and line.
  * c. argument errors leave a dirty object as it was (device_ptr() included); a poisoned object or operand gives the
    documented answer and stays poisoned.
  * d. sequences that leave every live / trade pair as they found it capture into a Graph and replay to the direct bits.

tests/test_module_model.py checks on the CPU that every module function is catalogued here for every class it accepts, that
every documented code has a row, and what the generated sequences cover."""
import numpy as np
import pytest

import mat_model as mm
import module_model as M
import test_gpu_mat_sequences as ms
import test_gpu_vec_sequences as vs
import vec_model as vm
from mat_model import FREQ, TIME
from module_model import tchol, tiir, tmul, trank, tsort, tzoom

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
DTYPE_IDS = ("f32", "f64")
DELTA = ms.DELTA


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    assert np.finfo(np.longdouble).nmant >= 63
    return b


# ---------------------------------------------------------------------------------------------- helpers
def _bits(a):
    return ms._bits(np.asarray(a))


def _same_state(kind, got, want, what):
    if kind == "mat" or not hasattr(want, "allocated_len"):   # (a matrix step's side objects are matrices and plain vectors)
        ms._same_state(got, want, what)
    else:
        vs._same_state(got, want, what)


def _api(kind, bd):
    return ms._Api(bd) if kind == "mat" else vs._Api(bd)


def _model_api(kind):
    return mm.ModelApi if kind == "mat" else vm.ModelApi


def _upload(kind, bd, a, cplx, domain=TIME, delta=1.0):
    return ms._mat(bd, a, cplx, domain, delta) if kind == "mat" else vs._vec(bd, a, cplx, domain, delta)


def _model_of(kind, a, cplx, domain=TIME, delta=1.0):
    """the model state of the same values and metadata"""
    return M.mat_state(a, cplx, domain, delta) if kind == "mat" else vm.VecModel(a, cplx, domain, delta)


def _snapshot(o):
    return dict(meta=ms._meta(o), delta=o.delta(), bits=_bits(o.data()).copy(), ptr=o.device_ptr())


def _unchanged(o, snap, what):
    """metadata, delta, bits and the live buffer's address are what the snapshot holds"""
    assert ms._meta(o) == snap["meta"], (what, "metadata", ms._meta(o), snap["meta"])
    ms._same_delta(o.delta(), snap["delta"], what)
    assert np.array_equal(_bits(o.data()), snap["bits"]), (what, "data bits")
    assert o.device_ptr() == snap["ptr"], (what, "device_ptr: the live and the trade buffer changed places")


def _same_value(p, q, what, exact_nan=True):
    """two results of a module function: None, numbers, arrays (bit for bit; integers by value), dicts, tuples, objects"""
    if p is None or q is None:
        assert p is None and q is None, (what, p, q)
    elif isinstance(p, dict):
        assert p.keys() == q.keys(), (what, sorted(p), sorted(q))
        for key in p:
            _same_value(p[key], q[key], (what, key), exact_nan)
    elif isinstance(p, (tuple, list)):
        assert len(p) == len(q), what
        for k, (a, b) in enumerate(zip(p, q)):
            _same_value(a, b, (what, k), exact_nan)
    elif isinstance(p, (int, np.integer)):
        assert isinstance(q, (int, np.integer)) and int(p) == int(q), (what, p, q)
    elif isinstance(p, (np.ndarray, np.floating)):
        p, q = np.asarray(p), np.asarray(q)
        assert p.dtype == q.dtype and p.shape == q.shape, (what, p.dtype, q.dtype, p.shape, q.shape)
        if p.dtype.kind == "f" and not exact_nan:   # test_gpu_sort.test_quantile_equals_the_exact_model: the NaN pattern, then ==
            assert np.array_equal(np.isnan(p), np.isnan(q)), (what, "NaN pattern")
            assert np.array_equal(p[~np.isnan(q)], q[~np.isnan(q)]), what
        elif p.dtype.kind == "f":
            assert np.array_equal(_bits(p), _bits(q)), (what, np.argwhere(_bits(p) != _bits(q))[:4].tolist())
        else:
            assert np.array_equal(p, q), (what, np.argwhere(p != q)[:4].tolist())
    else:
        kind = "mat" if hasattr(p, "rows") else "vec"
        _same_state(kind, p, q, what)


# ============================================================================================== a: sequences
_SEQ = {}


def _sequence(rows, pts, seed):
    key = (rows, pts, seed)
    if key not in _SEQ:
        _SEQ[key] = M.gen_module_sequence(*key)[0]
    return _SEQ[key]


def _start_data(rows, pts, dtype, seed, edge=True):
    """test_gpu_sort.draw's `edge` class: normal noise, every second scalar (drawn) replaced by one of +-0, +-inf, quiet and
    signalling NaNs of both signs with payloads, denormals and the largest finite values.  edge=False: the noise alone,
    for the sequences that hold overlap_add, which adds"""
    x = tsort.draw(4100 + 7 * seed + pts, rows or 1, pts, dtype, "edge" if edge else "uniform")
    return np.array(x if rows is not None else x[0])


def _read_only(kind, bd, g, w, what):
    """the read-only functions on the current state: the model's answers, and the object left exactly as it was"""
    snap = _snapshot(g)
    rows, n, _ = M.grid(w)
    calls = [("argsort", (True,), {}), ("top_k", (min(n, 8),), {}), ("detect", (), dict(threshold=None, order=1)),
             ("argrelmax", (), dict(order=2))]
    for name, args, kw in calls:
        got, want = getattr(bd, name)(g, *args, **kw), getattr(M, name)(w, *args, **kw)
        assert got[0] == want[0], (what, name, "codes", got[0], want[0])
        _same_value(got[1], want[1], (what, name))
    qs = [0, 0.25, 0.5, 1]
    code, got = bd.quantile(g, qs, "linear")
    wcode, want = M.quantile(w, qs, "linear")   # every row (the generator keeps a matrix at M.MAX_ROWS rows or fewer)
    assert code == wcode, (what, "quantile", "codes", code, wcode)
    _same_value(got, want, (what, "quantile"), exact_nan=False)
    _unchanged(g, snap, (what, "after the read-only functions"))


SEQ_CASES = [("mat", r, p, d) for (r, p) in M.START_SHAPES for d in DTYPES] + [("vec", None, p, d) for p in M.START_POINTS for d in DTYPES]


@pytest.mark.parametrize("kind,rows,pts,dtype", SEQ_CASES,
                         ids=["%s-%s%d-%s" % (k, "" if r is None else "%dx" % r, p, np.dtype(d).name) for (k, r, p, d) in SEQ_CASES])
def test_module_sequences_equal_the_model_at_every_step(bd, kind, rows, pts, dtype):
    """the sequences of module_model.MAT_SEEDS / VEC_SEEDS from this start state; nothing is skipped.  The assertion names
    the seed, the step index and the step: a sort that forgot (or doubled) its trade after an odd pass count, or a
    rank_filter that wrote past a row the transpose before it had shortened, fails here at that step."""
    api, fns = _api(kind, bd), bd
    for seed in (M.MAT_SEEDS if kind == "mat" else M.VEC_SEEDS):
        seq = _sequence(rows, pts, seed)
        x = _start_data(rows, pts, dtype, seed, edge=not any(step[0] in M.ARITHMETIC_MOVERS for step in seq))
        g, w = _upload(kind, bd, x, False, TIME, 0.25), _model_of(kind, x, False, TIME, 0.25)
        _same_state(kind, g, w, (seed, "start"))
        base = (g, g.device_ptr(), M.trades(w), w.reallocs)
        for i, step in enumerate(seq):
            what = ("seed", seed, "step", i, step)
            g_codes, g, g_side = M.apply_step(kind, fns, api, g, step)
            w_codes, w, w_side = M.apply_step(kind, M.ModelFns, _model_api(kind), w, step)
            assert g_codes == w_codes, (what, "codes", g_codes, w_codes)
            _same_state(kind, g, w, what)
            # the model's count of trades is the device's: since the object was made or last reallocated, the live buffer
            # is where it was iff the count's parity is what it was
            if g is not base[0] or w.reallocs != base[3]:
                base = (g, g.device_ptr(), M.trades(w), w.reallocs)
            else:
                assert (g.device_ptr() == base[1]) == ((M.trades(w) - base[2]) % 2 == 0), (what, "trades", M.trades(w) - base[2])
            assert len(g_side) == len(w_side)
            for k, (a, b) in enumerate(zip(g_side, w_side)):
                _same_state(kind, a, b, (what, "side object", k))
            if kind == "mat" or not w.unspec.any():   # (what set_len grew is not specified: no answer to compare)
                _read_only(kind, bd, g, w, what)


# ============================================================================================== b: the catalogue
class Ctx:
    """what an entry's call and check see: the state's description, its model, and operands that are built dirty for the
    dirty object and fresh for the fresh one (equal values either way)"""

    def __init__(self, kind, bd, dtype, w, seed, dirty):
        self.kind, self.bd, self.dtype, self.w, self.seed, self.dirty = kind, bd, dtype, w, seed, dirty
        self.cplx, self.domain = bool(w.is_complex()), w.domain()
        self.rows, self.n, _ = M.grid(w)
        self.points = self.n // (2 if self.cplx else 1)
        self.arrays, self.models = {}, {}

    def mat(self, k, rows, points, lo=-10, hi=10, cplx=None, dirty=None, values=None):
        """operand matrix k.  Dirty: uploaded transposed and transposed back on the device (ms.Ctx.mat's route: traded
        buffers, `rows` rewritten); fresh: uploaded as it is."""
        cplx = self.cplx if cplx is None else cplx
        dirty = self.dirty if dirty is None else dirty
        e = 2 if cplx else 1
        base = ms._fill(rows, points * e, self.seed + 101 * k, self.dtype, lo, hi) if values is None else np.array(values)
        self.arrays[k] = base
        self.models[k] = M.mat_state(base, cplx, self.domain, DELTA)
        if dirty and base.size:
            t = np.ascontiguousarray(base.reshape(rows, points, e).transpose(1, 0, 2)).reshape(points, rows * e)
            m = ms._mat(self.bd, t, cplx, self.domain, DELTA)
            assert m.transpose() == 0
            return m
        return ms._mat(self.bd, base, cplx, self.domain, DELTA)

    def vec(self, k, points, lo=-10, hi=10, cplx=None, dirty=None):
        """operand vector k.  Dirty: uploaded one scalar pair longer and cut back by set_len on the device; fresh: as it is."""
        cplx = self.cplx if cplx is None else cplx
        dirty = self.dirty if dirty is None else dirty
        e = 2 if cplx else 1
        base = vs._fill(points * e, self.seed + 211 * k, self.dtype, lo, hi)
        self.arrays[k] = base
        self.models[k] = vm.VecModel(base, cplx, self.domain, DELTA)
        if dirty and base.size:
            v = vs._vec(self.bd, np.concatenate([base, np.full(2, 77.0, self.dtype)]), cplx, self.domain, DELTA)
            vs._Api(self.bd).set_len(v, base.size)
            assert v.len() == base.size
            return v
        return vs._vec(self.bd, base, cplx, self.domain, DELTA)


class Entry:
    def __init__(self, fn, label, call, check=None, kinds=("mat", "vec"), space=None, rng=(-10, 10), hermitian=None,
                 need=("shrunk", "moved", "exact", "empty"), defined=None):
        """call(x, ctx) -> (code, extras): extras is whatever the call returned or wrote besides x -- arrays, dicts,
        numbers, matrices, vectors.  check(ctx, x0, got, code, extras): the reference assertions, x0 the model state before
        the call, got the object's data after it.  space: "real" / "complex" / None (both).  hermitian: the orders of the
        Hermitian states the entry also runs on.  need: the classes of state on which the entry must have answered 0.
        defined(w): whether the function is defined on model state w (default: on every state); there the fresh call must
        answer 0, elsewhere dirty and fresh must only agree."""
        self.fn, self.label, self.call, self.check, self.kinds, self.space = fn, label, call, check, kinds, space
        self.rng, self.hermitian, self.need, self.defined = rng, hermitian, need, defined or (lambda w: True)


# ---- zoom_fft ---------------------------------------------------------------------------------------------------------
def _zoom_bins(how, c):
    if how == "fits":        # the result's rows x bins x 2 scalars fit what the input already holds
        return max(1, c.points // 2 if not c.cplx else c.points)
    if how == "reallocates":   # one bin more than the allocation holds: the reserve inside the call reallocates
        return c.w.cap // (2 * max(c.rows, 1)) + 1
    return how


def e_zoom_fft(how, per_row=False):
    def start_of(c):
        return [0.01 * (r + 1) for r in range(c.rows)] if per_row else 0.05

    def call(x, c):
        bins = _zoom_bins(how, c)
        return c.bd.zoom_fft(x, start_of(c), 1.0 / (4 * max(c.points, 1)), bins), []

    def check(c, x0, got, code, extras):
        # test_gpu_zoom_fft.check_rows: rel-L2 per row <= TOL = 1e-6 / 1e-12 (tests/test_gpu_zoom_fft.py:34)
        bins = _zoom_bins(how, c)
        ref = M.zoom_fft_reference(x0, start_of(c), 1.0 / (4 * max(c.points, 1)), bins)
        tzoom.check_rows("zoom_fft(%s)" % how, tzoom.as_complex(got, c.rows), ref, c.dtype)
    label = "zoom_fft(%s%s)" % ("%d bins" % how if isinstance(how, int) else how, ", per-row starts" if per_row else "")
    return Entry("zoom_fft", label, call, check, kinds=("mat",) if per_row else ("mat", "vec"), rng=(-1, 1), need=("shrunk", "moved", "exact", "empty"))


# ---- sosfilt ----------------------------------------------------------------------------------------------------------
def e_sosfilt(S, state):
    sos = tiir.make_sos("lowpass", S)

    def make_state(c):
        if state == "none":
            return None
        dirty = c.dirty and state == "dirty"
        if c.kind == "mat":
            return c.mat(1, c.rows, 2 * S, -1, 1, dirty=dirty)
        return c.vec(1, 2 * S, -1, 1, dirty=dirty)

    def call(x, c):
        st = make_state(c)
        return c.bd.sosfilt(x, sos, st), ([] if st is None else [st])

    def check(c, x0, got, code, extras):
        # test_gpu_iir: e_dev <= R max(e_ser, eps max |truth|), R = 16 (tests/test_gpu_iir.py:23), outputs and final states
        out, fin = M.sosfilt_ratio(x0, sos, c.models.get(1), got, extras[0].data() if extras else None)
        print("sosfilt(%d, %s): ratio %.3f, states %s (bound %.0f)" % (S, state, out, fin, tiir.R))
        assert out <= tiir.R and (fin is None or fin <= tiir.R), (out, fin)
    return Entry("sosfilt", "sosfilt(%d sections, %s state)" % (S, state), call, check, rng=(-1, 1))


# ---- rank_filter, medfilt ---------------------------------------------------------------------------------------------
def e_rank(fn, label, args_of):
    def call(x, c):
        return getattr(c.bd, fn)(x, *args_of(c.dtype)), []

    def check(c, x0, got, code, extras):   # test_gpu_rank_filter: the bits of the model
        w = M.mat_state(M.grid(x0)[2], False)
        assert getattr(M, fn)(w, *args_of(c.dtype)) == 0
        assert np.array_equal(_bits(got).reshape(w.a.shape), _bits(w.a)), label
    return Entry(fn, label, call, check, space="real")


def _above_cross(dtype):
    half = trank.CROSS[dtype] // 2 + 1   # W = 2 half + 1 is the first odd window above the crossover: the bisecting selector
    return (half, half // 2, None, "nearest")


# ---- detect, argrelmax ------------------------------------------------------------------------------------------------
def e_detect(label, threshold_of, kinds=("mat", "vec"), **kw):
    """threshold_of(ctx, side) -> the threshold argument of the side: "gpu" or "model" """
    def call(x, c):
        code, det = c.bd.detect(x, threshold_of(c, "gpu"), **kw)
        return code, [det]

    def check(c, x0, got, code, extras):   # test_gpu_detect: counts, rows, indices equal, values to the bit
        wcode, want = M.detect(x0, threshold_of(c, "model"), **kw)
        assert wcode == code == 0
        _same_value(extras[0], want, label)
    return Entry("detect", label, call, check, kinds=kinds, space="real")


def _profile(c, side):
    if side == "gpu":
        return c.vec(1, c.n, dirty=c.dirty) if c.kind == "vec" else _row_vector(c)
    return c.models[1]


def _row_vector(c):
    """a profile for a matrix: ms.Ctx.vec's route (uploaded zero-interleaved, decimated on the device)"""
    base = vs._fill(c.n, c.seed + 211, c.dtype)
    c.arrays[1], c.models[1] = base, vm.VecModel(base, False, c.domain, DELTA)
    if c.dirty and base.size:
        wide = np.zeros((c.n, 2), c.dtype)
        wide[:, 0] = base
        v = vs._vec(c.bd, wide.reshape(-1), False, c.domain, DELTA)
        assert v.decimatei(2, 0) == 0 and v.points() == c.n
        return v
    return vs._vec(c.bd, base, False, c.domain, DELTA)


def _cell(c, side):
    return c.mat(1, c.rows, c.n, cplx=False) if side == "gpu" else c.models[1]


def _per_row(c, side):
    return [0.5 * (r % 5) - 1.0 for r in range(c.rows)]


# ---- sort, argsort, top_k, quantile, median ---------------------------------------------------------------------------
def e_order(fn, label, args=(), kw=None, in_place=False, exact_nan=True, on_empty=True):
    kw = kw or {}

    def resolve(c):
        return tuple(a(c) if callable(a) else a for a in args)

    def call(x, c):
        res = getattr(c.bd, fn)(x, *resolve(c), **kw)
        return (res, []) if in_place else (res[0], [res[1]])

    def check(c, x0, got, code, extras):   # test_gpu_sort: every comparison is equality
        w = _model_of(c.kind, x0.a, False)
        res = getattr(M, fn)(w, *resolve(c), **kw)
        if in_place:
            assert res == code == 0 and np.array_equal(_bits(got).reshape(-1), _bits(w.a).reshape(-1)), label
        else:
            assert res[0] == code == 0
            _same_value(extras[0], res[1], label, exact_nan)
    if on_empty:
        return Entry(fn, label, call, check, space="real")
    return Entry(fn, label, call, check, space="real", need=NOT_ON_EMPTY, defined=_has_points)


# ---- linalg -----------------------------------------------------------------------------------------------------------
def _square(w):
    """cholesky, cholesky_solve and eigh are defined on N x N points; 0 x 0 (D7-no-rows) is the documented N == 0"""
    return w.rows() == w.row_points()


def _has_points(w):
    """quantile, median and top_k(1) answer 7 on rows of no points (their docstrings): undefined on the empty states"""
    return M.grid(w)[1] > 0


NOT_ON_EMPTY = ("shrunk", "moved", "exact")


def e_matmul(form, which):
    """which: "first" -- x is the first operand, the second is fresh; "second" -- x is the second operand, the first is
    fresh; "both" -- x first, the second built dirty; "same" -- matmul(x, x)"""
    trans = form == "conj_transpose"

    def operands(x, c):
        R, P = c.rows, c.points
        if which == "same":
            return x, x
        if which == "second":   # b (3 x R) . x, or b (3 x P) . x^H
            return c.mat(1, 3, P if trans else R, dirty=False), x
        return x, c.mat(1, 3 if trans else P, P if trans else 3, dirty=c.dirty and which == "both")

    def call(x, c):
        a, b = operands(x, c)
        code, y = c.bd.matmul(a, b, conj_transpose=trans)
        return code, [y]

    def check(c, x0, got, code, extras):
        # test_gpu_mat_mul.worst_ratio: |out - ref| <= (2 K + 4) eps sum |a| |b| element by element
        a, b = (x0, x0) if which == "same" else (c.models[1], x0) if which == "second" else (x0, c.models[1])
        r = M.matmul_ratio(a, b, trans, extras[0].data())
        print("matmul(%s, %s): %.4f of the bound" % (form, which, r))
        assert r <= 1.0, r
    return Entry("matmul", "matmul(%s, %s dirty)" % (form, which), call, check, kinds=("mat",), need=("shrunk", "moved", "exact", "empty"))


def e_cholesky(loading):
    def call(x, c):
        code, l = c.bd.cholesky(x, loading=loading) if loading else c.bd.cholesky(x)
        return code, [l]

    def check(c, x0, got, code, extras):
        # test_gpu_mat_chol.chol_ratio: |A - L L^H| <= (2 N + 4) eps |L| |L|^H, and the factor's structure
        l = extras[0].data()
        tchol.check_structure(l, c.cplx)
        r = M.cholesky_ratio(x0, l, loading)
        print("cholesky(loading %g) N %d: %.4f of the bound" % (loading, c.rows, r))
        assert r <= 1.0, r
    return Entry("cholesky", "cholesky(loading %g)" % loading, call, check, kinds=("mat",), hermitian=M.CHOLESKY_N, defined=_square)


def e_cholesky_solve(part, dirty_factor=False):
    def call(x, c):
        code, l = c.bd.cholesky(x)
        if code != 0:
            return code, [l]
        if dirty_factor:   # the factor itself with a history: downloaded, uploaded transposed, transposed back on the device
            l = c.mat(2, c.rows, c.rows, values=l.data())
        b = c.mat(1, c.rows, 3, -1, 1)
        code, y = c.bd.cholesky_solve(l, b, part=part)
        return code, [l, y]

    def check(c, x0, got, code, extras):
        # test_gpu_mat_chol.solve_ratio: |B - L X| <= c(N) eps |L| |X| (one pass), 3 c(N) (both)
        l = M.mat_state(extras[0].data(), c.cplx)
        r = M.cholesky_solve_ratio(l, c.models[1], extras[1].data(), part)
        print("cholesky_solve(%s) N %d: %.4f of the bound" % (part, c.rows, r))
        assert r <= 1.0, r
    label = "cholesky_solve(%s%s)" % (part, ", dirty factor" if dirty_factor else "")
    return Entry("cholesky_solve", label, call, check, kinds=("mat",), hermitian=M.CHOLESKY_N, defined=_square)


def e_eigh():
    def call(x, c):
        code, w, v, sweeps = c.bd.eigh(x, return_sweeps=True)
        return code, [w, v, sweeps]

    def check(c, x0, got, code, extras):   # test_gpu_mat_eigh.check: residual, orthogonality, f32 eigenvalues, the order of w
        M.eigh_check(x0, extras[0].data(), extras[1].data(), extras[2], "eigh on a history")
    return Entry("eigh", "eigh", call, check, kinds=("mat",), hermitian=M.EIGH_N, defined=_square)


def e_chain():
    """matmul -> cholesky -> cholesky_solve -> matmul: A = x x^H (the rows' Gram matrix), A = L L^H, A X = B, Y = A X"""
    def call(x, c):
        code, a = c.bd.matmul(x, x, conj_transpose=True)
        if code != 0:
            return code, [a]
        code, l = c.bd.cholesky(a)
        if code != 0:
            return code, [a, l]
        b = c.mat(1, c.rows, 4, -1, 1)
        code, xs = c.bd.cholesky_solve(l, b)
        if code != 0:
            return code, [a, l, xs]
        code, y = c.bd.matmul(a, xs)
        return code, [a, l, xs, y]

    def check(c, x0, got, code, extras):
        # every link to the bound of its own test and no other: the solve's residual |B - L L^H X| <= 3 c(N) eps |L| |L|^H |X|
        # (test_gpu_mat_chol.solve_ratio, "both"), the factor |A - L L^H| <= c(N) eps |L| |L|^H (chol_ratio), and the two
        # products (2 K + 4) eps sum |a| |b| (test_gpu_mat_mul.worst_ratio)
        a, l, xs, y = [m.data() for m in extras]
        am, xm = M.mat_state(a, c.cplx), M.mat_state(xs, c.cplx)
        ratios = dict(gram=M.matmul_ratio(x0, x0, True, a), cholesky=M.cholesky_ratio(am, l),
                      solve=M.cholesky_solve_ratio(M.mat_state(l, c.cplx), c.models[1], xs, "both"), product=M.matmul_ratio(am, xm, False, y))
        print("chain: of the bounds", {k: round(v, 4) for k, v in ratios.items()})
        assert max(ratios.values()) <= 1.0, ratios
    # defined where the Gram matrix of the rows is positive definite: no more rows than points (0 x 0: the N == 0 path)
    return Entry("matmul", "chain matmul -> cholesky -> cholesky_solve -> matmul", call, check, kinds=("mat",), rng=(-1, 1),
                 defined=lambda w: w.rows() == 0 or 0 < w.rows() <= w.row_points())


def _catalogue():
    cat = [e_zoom_fft("fits"), e_zoom_fft("reallocates"), e_zoom_fft(2200), e_zoom_fft(64, per_row=True)]
    cat += [e_sosfilt(S, st) for S in (2, 16) for st in ("none", "fresh", "dirty")]
    cat += [e_rank("rank_filter", "rank_filter(half 1)", lambda d: (1, 1, None, "zero")),
            e_rank("rank_filter", "rank_filter(above the crossover)", _above_cross),
            e_rank("rank_filter", "rank_filter(guard, wrap)", lambda d: (8, 3, 2, "wrap")),
            e_rank("medfilt", "medfilt(5)", lambda d: (5,))]
    cat += [e_detect("detect(no threshold, order 1)", lambda c, s: None, order=1),
            e_detect("detect(scalar)", lambda c, s: 0.5),
            e_detect("detect(per row, order 2, wrap)", _per_row, order=2, boundary="wrap"),
            e_detect("detect(profile)", _profile),
            e_detect("detect(per cell)", _cell, kinds=("mat",)),
            e_detect("detect(capacity below the total)", lambda c, s: None, capacity=7)]
    cat.append(Entry("argrelmax", "argrelmax(order 2, wrap)",
                     lambda x, c: (lambda r: (r[0], [r[1]]))(c.bd.argrelmax(x, order=2, mode="wrap")),
                     lambda c, x0, got, code, extras: _same_value(extras[0], M.argrelmax(x0, 2, "wrap")[1], "argrelmax"), space="real"))
    cat += [e_order("sort", "sort(ascending)", (False,), in_place=True), e_order("sort", "sort(descending)", (True,), in_place=True),
            e_order("argsort", "argsort(ascending)", (False,)), e_order("argsort", "argsort(descending)", (True,))]
    for largest in (True, False):
        tag = "largest" if largest else "smallest"
        cat += [e_order("top_k", "top_k(1, %s)" % tag, (1, largest), on_empty=False),
                e_order("top_k", "top_k(8, %s)" % tag, (lambda c: min(8, c.n), largest)),
                e_order("top_k", "top_k(n, %s)" % tag, (lambda c: c.n, largest))]
    cat += [e_order("quantile", "quantile(%s)" % m, ([0.0, 0.1, 0.5, 0.999, 1.0], m), exact_nan=False, on_empty=False) for m in tsort.METHODS]
    cat.append(e_order("median", "median", exact_nan=False, on_empty=False))
    cat += [e_matmul(form, which) for form in ("plain", "conj_transpose") for which in ("first", "second", "both")]
    cat.append(e_matmul("conj_transpose", "same"))
    cat += [e_cholesky(0.0), e_cholesky(0.25)]
    cat += [e_cholesky_solve(p) for p in ("both", "forward", "backward")] + [e_cholesky_solve("both", dirty_factor=True)]
    cat += [e_eigh(), e_chain()]
    return cat


MODULE_CATALOGUE = _catalogue()
assert len({e.label for e in MODULE_CATALOGUE}) == len(MODULE_CATALOGUE)


# ---- the states -------------------------------------------------------------------------------------------------------
def _spaces(d):
    return (False, True) if d["is_complex"] is None else (d["is_complex"],)


def _class_of(kind, name):
    """the class of history a state stands for in an entry's `need`"""
    if kind == "mat":
        if name.startswith(("D1", "L1", "H2")):
            return "shrunk"
        if name.startswith(("D2", "D4", "L3", "H1")):   # transposed on the device; D4: regrown and traded by swap_halves
            return "moved"
        return "exact" if name.startswith(("D3", "L2", "H4")) else "empty" if name.startswith("D7") else None
    base = name.split(":")[-1]
    if base.startswith("shrunk"):
        return "shrunk"
    if base.startswith(("odd-trades", "regrown")):
        return "moved"
    return "exact" if base.startswith("exact-fit") else "empty" if base == "empty" else None


def states_of(entry, kind):
    """(name, is_complex, order or None) of every state the entry runs on: mm.DIRTY / vm.DIRTY, the long states, and for
    linalg the Hermitian states at the orders the entry names"""
    if kind == "mat":
        out = [(n, c, None) for n, d in mm.DIRTY.items() for c in _spaces(d)]
        out += [(n, c, None) for n, d in M.LONG_DIRTY.items() for c in _spaces(d)]
        if entry.hermitian:
            out += [(n, c, N) for n in M.HERMITIAN for N in entry.hermitian for c in (False, True)]
            assert M.H4_N in entry.hermitian
            out.append((M.EXACT_FIT_HERMITIAN, False, M.H4_N))
    else:
        out = [(n, c, None) for n, d in vm.DIRTY.items() for c in _spaces(d)]
        out += [("long:" + n, c, None) for n, d in M.LONG_DIRTY_VEC.items() for c in _spaces(d)]
    if entry.space is not None:
        out = [s for s in out if s[1] == (entry.space == "complex")]
    return out


def build_state(kind, api, name, cplx, order, dtype, domain, rng, seed, bd=None):
    """the state on side `api` (bd: the GPU side, whose H3 is a device product)"""
    if kind == "mat":
        fill = lambda rows, scalars: ms._fill(rows, scalars, seed, dtype, *rng)
        if order is not None:
            return M.build_hermitian(api, name, order, cplx, dtype, domain, DELTA, matmul=bd.matmul if bd is not None else None)
        if name in M.LONG_DIRTY:
            return M.build_long(api, name, fill, cplx, domain, DELTA)
        make_vec = (lambda a: bd.DspVec(a, is_complex=True, domain=domain, delta=DELTA)) if bd is not None else \
            (lambda a: mm.VecModel(a, True, domain, DELTA))
        return mm.build_dirty(api, name, fill, dtype, cplx, domain, DELTA, vec=make_vec)
    fill = lambda n, k: vs._fill(n, seed + 53 * k, dtype, *rng)
    if name.startswith("long:"):
        return M.build_long_vec(api, name[5:], fill, cplx, domain, DELTA)
    return vm.build_dirty(api, name, fill, cplx, domain, DELTA)


HISTORY_CASES = [(e, k, d) for e in MODULE_CATALOGUE for k in e.kinds for d in DTYPES]


@pytest.mark.parametrize("entry,kind,dtype", HISTORY_CASES,
                         ids=["%s-%s-%s" % (e.label, k, np.dtype(d).name) for e, k, d in HISTORY_CASES])
def test_module_results_owe_nothing_to_history(bd, entry, kind, dtype):
    """the function on every dirty state and on a fresh upload of the same values and metadata: equal code, metadata,
    delta and bits of the object and of everything returned.  The comparison names the state: a stale `rows` after the
    device transpose, a missed or doubled trade, a stride taken from the allocation instead of the valid length or a
    write past an exact-fit allocation makes the dirty object differ from its fresh copy here.  Then the fresh result
    against the function's own reference, once, on the first state with data; and on every class of state the entry
    names the function must have answered 0 at least once."""
    api = _api(kind, bd)
    ran, checked = set(), False
    for k, (name, cplx, order) in enumerate(states_of(entry, kind)):
        seed = 3000 + 17 * k
        d = build_state(kind, api, name, cplx, order, dtype, TIME, entry.rng, seed, bd)
        w = build_state(kind, _model_api(kind), name, cplx, order, dtype, TIME, entry.rng, seed)
        what = (entry.label, kind, name, order, "complex" if cplx else "real")
        if name != "H3-product":   # the recipe's result is known exactly, a vector's capacity included
            _same_state(kind, d, w, (what, "the recipe's result"))
        else:                      # a device product: Hermitian to the bit, as matmul documents; its values are d's own
            p = tchol.as_points(d.data(), cplx)
            assert np.array_equal(p, p.conj().T) and (d.rows(), d.row_points()) == (order, order), what
        x = d.data()
        f = _upload(kind, bd, x, d.is_complex(), d.domain(), d.delta())
        _same_state(kind, f, d, (what, "fresh copy"))
        x0 = _model_of(kind, x, d.is_complex(), d.domain(), d.delta())
        x0.cap = w.cap
        ctxs = [Ctx(kind, bd, dtype, x0, seed, dirty) for dirty in (True, False)]
        code_d, extra_d = entry.call(d, ctxs[0])
        code_f, extra_f = entry.call(f, ctxs[1])
        assert code_d == code_f, (what, "codes", code_d, code_f)
        _same_state(kind, d, f, what)
        _same_value(extra_d, extra_f, (what, "results"))
        if entry.defined(x0):
            assert code_f == 0, (what, "defined here, yet refused", code_f)
        if code_f == 0:   # a state on which the call was refused does not count as run
            ran.add(_class_of(kind, name))
        if not checked and x.size and code_f == 0 and entry.check is not None:
            with np.errstate(all="ignore"):
                entry.check(ctxs[1], x0, f.data(), code_f, extra_f)
            checked = True
    need = set(entry.need) - ({"exact"} if entry.space == "complex" else set())
    assert need <= ran and checked, (entry.label, kind, "classes of state without a call that answered 0:", sorted(need - ran), "checked:", checked)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_matmul_paths_with_dirty_operands(bd, dtype):
    """one shape per path and form of tests/mat_mul_shapes.txt, the one of the fewest multiplications: the first operand
    shrunk on the device (uploaded with junk in the odd columns, decimated), the second transposed on the device; the
    bits of the product of fresh uploads, and test_gpu_mat_mul's bound (worst_ratio <= 1)."""
    smallest = {}
    for path, trans, Mr, K, N in tmul.SHAPES:
        if (path, trans) not in smallest or Mr * K * N < np.prod(smallest[(path, trans)][2:]):
            smallest[(path, trans)] = (path, trans, Mr, K, N)
    assert len(smallest) == 5
    for (path, trans, Mr, K, N) in smallest.values():
        for cplx in (False, True):
            e = 2 if cplx else 1
            a, b = tmul.operands(77, Mr, K, N, cplx, trans, dtype)
            wide = np.full((Mr, 2 * K, e), 3.0, dtype)
            wide[:, 0::2, :] = a.reshape(Mr, K, e)
            da = ms._mat(bd, wide.reshape(Mr, 2 * K * e), cplx)
            assert da.decimatei(2, 0) == 0
            br, bp = b.shape[0], b.shape[1] // e
            db = ms._mat(bd, np.ascontiguousarray(b.reshape(br, bp, e).transpose(1, 0, 2)).reshape(bp, br * e), cplx)
            assert db.transpose() == 0
            snaps = _snapshot(da), _snapshot(db)
            fresh = tmul.product(bd, a, b, cplx, trans)
            for first, second, what in ((da, tmul.upload(bd, b, cplx), "first"), (tmul.upload(bd, a, cplx), db, "second"), (da, db, "both")):
                code, y = bd.matmul(first, second, conj_transpose=trans)
                assert code == 0 and np.array_equal(_bits(y.data()), _bits(fresh)), (path, trans, cplx, what)
            _unchanged(da, snaps[0], (path, "first operand"))
            _unchanged(db, snaps[1], (path, "second operand"))
            ref, mod = tmul.reference(a, b, cplx, trans)
            assert tmul.worst_ratio(fresh, ref, mod, K, dtype, cplx) <= 1.0, (path, trans, cplx)


# ============================================================================================== c: errors, poisoning
def _bad_sos():
    s = tiir.make_sos("lowpass", 2)
    s[1, 3] = 0.0   # a0 == 0
    return s


SOS2 = tiir.make_sos("lowpass", 2)


def _arg_errors():
    """(function, label, kinds, space, domain, bad call(x, ctx) -> code or (code, result), the documented code): every
    module function whose docstring names an argument-error code (tests/test_module_model.py checks that none is missing).
    A call that breaks two rules gives the code the docstring puts first."""
    first = lambda r: r[0] if isinstance(r, tuple) else r
    B = lambda c: c.bd
    t = [
        ("zoom_fft", "0 bins", ("mat", "vec"), None, TIME, lambda x, c: B(c).zoom_fft(x, 0.1, 0.01, 0), 7),
        ("zoom_fft", "a step that is not finite", ("mat", "vec"), None, TIME, lambda x, c: B(c).zoom_fft(x, 0.1, float("inf"), 8), 7),
        ("zoom_fft", "one start too few", ("mat",), None, TIME, lambda x, c: B(c).zoom_fft(x, [0.1] * (c.rows - 1), 0.01, 8), 7),
        ("zoom_fft", "0 bins on frequency-domain data: 7 comes first", ("mat", "vec"), None, FREQ, lambda x, c: B(c).zoom_fft(x, 0.1, 0.01, 0), 7),
        ("zoom_fft", "frequency-domain data", ("mat", "vec"), None, FREQ, lambda x, c: B(c).zoom_fft(x, 0.1, 0.01, 8), 5),
        ("sosfilt", "a sos that is not [S, 6]", ("mat", "vec"), None, TIME, lambda x, c: B(c).sosfilt(x, np.ones((2, 5))), 7),
        ("sosfilt", "a0 == 0", ("mat", "vec"), None, TIME, lambda x, c: B(c).sosfilt(x, _bad_sos()), 7),
        ("sosfilt", "17 sections", ("mat", "vec"), None, TIME, lambda x, c: B(c).sosfilt(x, tiir.make_sos("lowpass", 17)), 7),
        ("sosfilt", "a0 == 0 on frequency-domain data: 7 comes first", ("mat", "vec"), None, FREQ, lambda x, c: B(c).sosfilt(x, _bad_sos()), 7),
        ("sosfilt", "frequency-domain data", ("mat", "vec"), None, FREQ, lambda x, c: B(c).sosfilt(x, SOS2), 5),
        ("sosfilt", "a state of the other number kind", ("mat", "vec"), None, TIME,
         lambda x, c: B(c).sosfilt(x, SOS2, c.mat(1, c.rows, 4, cplx=not c.cplx) if c.kind == "mat" else c.vec(1, 4, cplx=not c.cplx)), 2),
        ("sosfilt", "a state of the wrong shape", ("mat", "vec"), None, TIME,
         lambda x, c: B(c).sosfilt(x, SOS2, c.mat(1, c.rows, 5) if c.kind == "mat" else c.vec(1, 5)), 7),
        ("rank_filter", "rank == W", ("mat", "vec"), "real", TIME, lambda x, c: B(c).rank_filter(x, 2, 5), 7),
        ("rank_filter", "guard == half", ("mat", "vec"), "real", TIME, lambda x, c: B(c).rank_filter(x, 2, 0, guard=2), 7),
        ("rank_filter", "an unknown boundary", ("mat", "vec"), "real", TIME, lambda x, c: B(c).rank_filter(x, 2, 0, boundary="mirror"), 7),
        ("rank_filter", "rank == W on complex data: 7 comes first", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).rank_filter(x, 2, 5), 7),
        ("rank_filter", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).rank_filter(x, 2, 2), 4),
        ("medfilt", "an even kernel", ("mat", "vec"), "real", TIME, lambda x, c: B(c).medfilt(x, 4), 7),
        ("medfilt", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).medfilt(x, 3), 4),
        ("detect", "a negative order", ("mat", "vec"), "real", TIME, lambda x, c: B(c).detect(x, None, -1), 7),
        ("detect", "an unknown boundary", ("mat", "vec"), "real", TIME, lambda x, c: B(c).detect(x, None, 1, "zero"), 7),
        ("detect", "a sequence of the wrong length", ("mat", "vec"), "real", TIME, lambda x, c: B(c).detect(x, [0.0] * (c.rows + 1)), 7),
        ("detect", "a matrix threshold for a vector", ("vec",), "real", TIME, lambda x, c: B(c).detect(x, c.mat(1, 1, c.n)), 7),
        ("detect", "a threshold of the other precision", ("mat", "vec"), "real", TIME,
         lambda x, c: B(c).detect(x, B(c).DspVec(np.zeros(c.n, np.float64 if c.dtype == np.float32 else np.float32))), 2),
        ("detect", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).detect(x, 0.5), 4),
        ("detect", "a negative order on complex data: 7 comes first", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).detect(x, 0.5, -1), 7),
        ("detect", "a cell matrix of another row count", ("mat",), "real", TIME, lambda x, c: B(c).detect(x, c.mat(1, c.rows - 1, c.n)), 7),
        ("detect", "a profile of another length", ("mat", "vec"), "real", TIME, lambda x, c: B(c).detect(x, c.vec(1, c.n - 1)), 1),
        ("detect", "a profile of the other domain", ("mat", "vec"), "real", TIME,
         lambda x, c: B(c).detect(x, vs._vec(B(c), vs._fill(c.n, 5, c.dtype), False, FREQ, DELTA)), 2),
        ("argrelmax", "order 0", ("mat", "vec"), "real", TIME, lambda x, c: B(c).argrelmax(x, 0), 7),
        ("argrelmax", "an unknown mode", ("mat", "vec"), "real", TIME, lambda x, c: B(c).argrelmax(x, 1, "open"), 7),
        ("argrelmax", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).argrelmax(x, 1), 4),
        ("sort", "a direction that is no bool", ("mat", "vec"), "real", TIME, lambda x, c: B(c).sort(x, 2), 7),
        ("sort", "a direction that is no bool on complex data: 7 comes first", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).sort(x, 2), 7),
        ("sort", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).sort(x), 4),
        ("argsort", "a direction that is no bool", ("mat", "vec"), "real", TIME, lambda x, c: B(c).argsort(x, None), 7),
        ("argsort", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).argsort(x), 4),
        ("top_k", "k above n", ("mat", "vec"), "real", TIME, lambda x, c: B(c).top_k(x, c.n + 1), 7),
        ("top_k", "k above n on complex data: 7 comes first", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).top_k(x, c.n + 1), 7),
        ("top_k", "a k that is no integer", ("mat", "vec"), "real", TIME, lambda x, c: B(c).top_k(x, 2.0), 7),
        ("top_k", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).top_k(x, 3), 4),
        ("quantile", "q above 1", ("mat", "vec"), "real", TIME, lambda x, c: B(c).quantile(x, 1.5), 7),
        ("quantile", "an unknown method", ("mat", "vec"), "real", TIME, lambda x, c: B(c).quantile(x, 0.5, "nearest"), 7),
        ("quantile", "q above 1 on complex data: 7 comes first", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).quantile(x, 1.5), 7),
        ("quantile", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).quantile(x, 0.5), 4),
        ("median", "complex data", ("mat", "vec"), "complex", TIME, lambda x, c: B(c).median(x), 4),
        ("matmul", "inner sizes that differ", ("mat",), None, TIME, lambda x, c: B(c).matmul(x, c.mat(1, c.points + 1, 3)), 7),
        ("matmul", "inner sizes that differ, conj_transpose", ("mat",), None, TIME,
         lambda x, c: B(c).matmul(x, c.mat(1, 3, c.points + 1), conj_transpose=True), 7),
        ("matmul", "a real and a complex operand", ("mat",), None, TIME, lambda x, c: B(c).matmul(x, c.mat(1, c.points, 3, cplx=not c.cplx)), 2),
        ("matmul", "as the second operand, inner sizes that differ", ("mat",), None, TIME, lambda x, c: B(c).matmul(c.mat(1, 3, c.rows + 1), x), 7),
        ("cholesky", "not square", ("mat",), None, TIME, lambda x, c: B(c).cholesky(x), 7),
        ("cholesky_solve", "a factor that is not square", ("mat",), None, TIME, lambda x, c: B(c).cholesky_solve(x, c.mat(1, c.rows, 3)), 7),
        ("cholesky_solve", "as the right-hand side, another row count", ("mat",), None, TIME,
         lambda x, c: B(c).cholesky_solve(c.mat(1, c.rows + 1, c.rows + 1), x), 7),
        ("cholesky_solve", "as the right-hand side, the other number kind", ("mat",), None, TIME,
         lambda x, c: B(c).cholesky_solve(c.mat(1, c.rows, c.rows, cplx=not c.cplx), x), 2),
        ("eigh", "not square", ("mat",), None, TIME, lambda x, c: B(c).eigh(x), 7),
    ]
    return t, first


MODULE_ARG_ERRORS, _first = _arg_errors()
# (function, code) that a docstring (or the one it refers to) names, and why MODULE_ARG_ERRORS has no row for it
MODULE_ARG_ERRORS_EXEMPT = {
    ("eigh", 1): "'1 for the identity' counts sweeps: it is no code",
    ("argrelmax", 2): "detect's 2 is about a device threshold, and argrelmax passes none",
    ("median", 7): "quantile's 7 is about q, the method and rows of no points: median takes neither argument, and no state of "
                   "D1 to D4, L1, L2 is empty (the catalogue runs median on the D7 states, where dirty and fresh both answer 7)",
}
MAT_ERR_STATES = [(n, c) for (n, c) in ms.DIRTY_STATES if n[:2] in ("D1", "D2", "D3", "D4")] + \
    [(n, c) for n in ("L1-shrunk-two-tiles", "L2-exact-fit-three-tiles") for c in _spaces(M.LONG_DIRTY[n])]
VEC_ERR_STATES = list(vs.ERR_STATES)


@pytest.mark.parametrize("kind", ("mat", "vec"))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_module_argument_errors_leave_a_dirty_object_as_it_was(bd, dtype, kind):
    """every row of MODULE_ARG_ERRORS on D1 to D4, L1 and L2 (vectors: the states of test_gpu_vec_sequences.ERR_STATES): the
    documented code, nothing returned, and metadata, delta, bits and device_ptr() of the object as the model left them"""
    api = _api(kind, bd)
    states = MAT_ERR_STATES if kind == "mat" else VEC_ERR_STATES
    built = {}
    for j, (fn, label, kinds, space, domain, bad, code) in enumerate(MODULE_ARG_ERRORS):
        if kind not in kinds:
            continue
        ran = 0
        for k, (name, cplx) in enumerate(states):
            if space is not None and (space == "complex") != cplx:
                continue
            key = (name, cplx, domain)
            if key not in built:   # a refused call leaves the object as it was: the rows share one object per state
                seed = 5000 + 31 * k
                d = build_state(kind, api, name, cplx, None, dtype, domain, (-10, 10), seed, bd)
                w = build_state(kind, _model_api(kind), name, cplx, None, dtype, domain, (-10, 10), seed)
                _same_state(kind, d, w, (name, "the recipe's result"))
                built[key] = (d, w, _snapshot(d))
            d, w, snap = built[key]
            what = (fn, label, kind, name, "complex" if cplx else "real")
            ctx = Ctx(kind, bd, dtype, w, 5000 + j, True)
            res = bad(d, ctx)
            assert _first(res) == code, (what, res)
            assert not isinstance(res, tuple) or all(r is None for r in res[1:]), (what, "a result came back with the code")
            _same_state(kind, d, w, (what, "after the refused call"))
            _unchanged(d, snap, what)
            ran += 1
        assert ran >= 2, (fn, label, kind, ran)


def _poisoned(kind, bd, dtype, cplx=False):
    """an object poisoned after a history: transposed on the device (a vector: traded by swap_halves), then a call its
    docstring says poisons it"""
    if kind == "mat":
        m = ms._mat(bd, ms._fill(7, 5 * (2 if cplx else 1), 11, dtype), cplx)
        assert m.transpose() == 0 and (m.mirror() if not cplx else m.to_complex()) == -1
        return m
    v = vs._vec(bd, vs._fill(35 * (2 if cplx else 1), 11, dtype), cplx)
    assert v.swap_halves() == 0 and (v.mirror() if not cplx else v.to_complex()) == -1 and v.is_erroneous()
    return v


def _is_poisoned(o):
    if hasattr(o, "rows"):
        return o.row_len() == 0 and np.isnan(o.delta())
    return bool(o.is_erroneous())


def _poisoned_rows():
    """(function, label, kinds, call(p, good, bd) -> result, the documented answer, the results that must be poisoned too):
    p the poisoned object, good a healthy one of the same kind"""
    sos = SOS2
    return [
        ("zoom_fft", "x", ("mat", "vec"), lambda p, good, bd: bd.zoom_fft(p, 0.1, 0.01, 8), -1),
        ("sosfilt", "x", ("mat", "vec"), lambda p, good, bd: bd.sosfilt(p, sos), -1),
        ("sosfilt", "state", ("mat", "vec"), lambda p, good, bd: bd.sosfilt(good, sos, p), -1),
        ("rank_filter", "x", ("mat", "vec"), lambda p, good, bd: bd.rank_filter(p, 1, 1), -1),
        ("rank_filter", "x, rank == W: 7 comes first", ("mat", "vec"), lambda p, good, bd: bd.rank_filter(p, 1, 3), 7),
        ("medfilt", "x", ("mat", "vec"), lambda p, good, bd: bd.medfilt(p, 3), -1),
        ("detect", "x", ("mat", "vec"), lambda p, good, bd: bd.detect(p, 0.5), (-1, None)),
        ("detect", "threshold", ("mat", "vec"), lambda p, good, bd: bd.detect(good, p), (-1, None)),
        ("argrelmax", "x", ("mat", "vec"), lambda p, good, bd: bd.argrelmax(p), (-1, None)),
        ("sort", "x", ("mat", "vec"), lambda p, good, bd: bd.sort(p), -1),
        ("sort", "x, a direction that is no bool: 7 comes first", ("mat", "vec"), lambda p, good, bd: bd.sort(p, 2), 7),
        ("argsort", "x", ("mat", "vec"), lambda p, good, bd: bd.argsort(p), (-1, None)),
        ("top_k", "x", ("mat", "vec"), lambda p, good, bd: bd.top_k(p, 0), (-1, None)),
        ("quantile", "x: rows of no points give 7 before the device is asked", ("mat", "vec"), lambda p, good, bd: bd.quantile(p, 0.5), (7, None)),
        ("median", "x: as quantile", ("mat", "vec"), lambda p, good, bd: bd.median(p), (7, None)),
        ("matmul", "first operand", ("mat",), lambda p, good, bd: bd.matmul(p, good), "poisoned result"),
        ("matmul", "second operand", ("mat",), lambda p, good, bd: bd.matmul(good, p, conj_transpose=True), "poisoned result"),
        ("cholesky", "a", ("mat",), lambda p, good, bd: bd.cholesky(p), "poisoned result"),
        ("cholesky_solve", "factor", ("mat",), lambda p, good, bd: bd.cholesky_solve(p, good), "poisoned result"),
        ("cholesky_solve", "right-hand side", ("mat",), lambda p, good, bd: bd.cholesky_solve(good, p), "poisoned result"),
        ("eigh", "a", ("mat",), lambda p, good, bd: bd.eigh(p), "poisoned result"),
    ]


MODULE_POISONED = _poisoned_rows()


@pytest.mark.parametrize("kind", ("mat", "vec"))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_module_calls_on_a_poisoned_object(bd, dtype, kind):
    """a poisoned x or operand gives -1 (or the function's documented answer), stays poisoned, and the other operand keeps
    metadata, bits and device_ptr(); results that come back are poisoned too"""
    for fn, label, kinds, call, want in MODULE_POISONED:
        if kind not in kinds:
            continue
        p = _poisoned(kind, bd, dtype)
        if kind == "mat":   # 7 x 7, transposed on the device: the rows of the poisoned operand, square for the linalg calls
            good = ms._mat(bd, ms._fill(7, 7, 12, dtype), False)
            assert good.transpose() == 0
        else:
            good = vs._vec(bd, vs._fill(35, 12, dtype), False)
            assert good.swap_halves() == 0
        snap = _snapshot(good)
        rows = p.rows() if kind == "mat" else None
        res = call(p, good, bd)
        what = (fn, label, kind)
        if want == "poisoned result":
            assert res[0] == -1 and all(r is not None and _is_poisoned(r) for r in res[1:]), (what, res)
        else:
            assert res == want, (what, res, want)
        assert _is_poisoned(p) and (kind == "vec" or p.rows() == rows), (what, "the poisoned object")
        _unchanged(good, snap, (what, "the other operand"))


# ============================================================================================== d: graph capture
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_graph_capture_replays_module_sequences_that_restore_their_buffers(bd, dtype):
    """as test_gpu_zoom_fft.test_graph_capture_replays_the_same_bits_once_the_plan_is_warm: a sequence a Graph may hold
    leaves every live / trade pair as it found it.  On L1 (3 x 4100 after decimatei: one merge pass, so every sort trades)
    sort + sort(descending) trade twice, and so does medfilt(3) twice.  (sosfilt, detect and the order_select family upload
    or read back inside the call and are documented as not capturable.)"""
    fill = lambda rows, scalars: tsort.draw(91, rows, scalars, dtype, "ties16")
    for seq_of in (lambda u: (lambda: (bd._lib.check(bd.sort(u)), bd._lib.check(bd.sort(u, descending=True)))),
                   lambda u: (lambda: (bd._lib.check(bd.medfilt(u, 3)), bd._lib.check(bd.medfilt(u, 3))))):
        v = M.build_long(ms._Api(bd), "L1-shrunk-two-tiles", fill, False, TIME, DELTA)
        w = M.build_long(ms._Api(bd), "L1-shrunk-two-tiles", fill, False, TIME, DELTA)
        ptr = v.device_ptr()
        g = bd.Graph.capture(seq_of(v))   # one warm-up run, then the capture, which runs nothing
        g.launch()
        g.launch()
        for _ in range(3):
            assert seq_of(w)() == (0, 0)
        assert v.device_ptr() == ptr and (v.rows(), v.row_len()) == (w.rows(), w.row_len()) == (3, 4100)
        assert np.array_equal(_bits(v.data()), _bits(w.data()))
        assert np.any(v.data() != 0)
        del g
