"""The module-level functions (zoom_fft, matmul, cholesky, cholesky_solve, eigh, sosfilt, rank_filter, medfilt, detect,
argrelmax, sort, argsort, top_k, quantile, median) on a model state.  numpy only: nothing here imports the library.

No operation is modelled a second time.  The order statistics, the rank filter and the detections have exact numpy models
in their own test files (test_gpu_sort.to_keys / model_order / model_quantile, test_gpu_rank_filter.model,
test_gpu_detect.model); the functions below wrap them so that they answer a mat_model.MatModel or a vec_model.VecModel
with the codes, in the order, of the Python functions of basic_dsp_amd, and so that the in-place ones (sort, medfilt,
rank_filter) are steps a sequence can hold next to the movers of mat_model / vec_model (apply_step).  The references of
the approximate functions (test_gpu_iir.models / yardstick, test_gpu_zoom_fft.model, test_gpu_mat_mul.reference,
test_gpu_mat_chol's and test_gpu_mat_eigh's bound functions) are wrapped on a state in the same way.

Next to the data the wrappers keep what a module operation does to the buffers: sort trades the live and the trade buffer
iff its merge pass count ceil(log2(ceil(n / SORT_TILE))) is odd, rank_filter always trades.  A VecModel counts every trade
(vec_model knows its movers'); for a MatModel apply_step counts them in `trades`, the movers' by MAT_MOVER_TRADES, which is
read from the host functions of capi.cpp (mat_model does not say which matrix movers trade).  The GPU test holds the parity
to device_ptr() at every step, for matrices and vectors.

The tables of this module: LONG_DIRTY / LONG_DIRTY_VEC (rows of more than one tile, in the style of mm.DIRTY / vm.DIRTY,
which are not edited: that would multiply the existing catalogue's run time), HERMITIAN (positive-definite matrices
reached by a history) and the generator of sequences that mix movers and in-place module operations."""
import copy
import math
import os
import re

import numpy as np

import mat_model as mm
import vec_model as vm
import test_gpu_detect as tdet
import test_gpu_iir as tiir
import test_gpu_mat_chol as tchol
import test_gpu_mat_eigh as teigh
import test_gpu_mat_mul as tmul
import test_gpu_rank_filter as trank
import test_gpu_sort as tsort
import test_gpu_zoom_fft as tzoom
from mat_model import PAD_END, TIME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SCALARS = 1 << 16   # of a generated sequence's state: the exact models sort a window per scalar
STEPS = 16


def read_constants(header, prefix):
    """the `constexpr int PREFIX_* = N;` of a core header, as test_gpu_rank_filter.read_constants reads its own"""
    with open(os.path.join(ROOT, "basic_dsp_amd", "csrc", header)) as f:
        return {k: int(v) for k, v in re.findall(r"^constexpr int (%s_\w+) = (\d+);" % prefix, f.read(), re.M)}


SORT_TILE = read_constants("sort_core.h", "SORT")["SORT_TILE"]
IIR_TILE = read_constants("iir_core.h", "IIR")["IIR_TILE"]
DETECT_TILE = tdet.TILE
MAX_HALF = trank.MAX_HALF


# ---------------------------------------------------------------------------------------------- a state, either kind
def is_mat(s):
    return isinstance(s, mm.MatModel)


def poisoned(s):
    return s.poisoned if is_mat(s) else bool(s.a.size == 0 and np.isnan(s.delta()))


def grid(s):
    """(rows, scalars per row, the data as [rows, n]) of a MatModel or of a VecModel (one row)"""
    if is_mat(s):
        return s.rows(), s.row_len(), s.a.reshape(s.rows(), s.row_len())
    return 1, s.a.size, s.a.reshape(1, -1)


def trades(s):
    return getattr(s, "trades", 0) if is_mat(s) else s.trades


def _store(s, rows_data, traded):
    if is_mat(s):
        s.a = np.ascontiguousarray(rows_data).reshape(s.a.shape)
        s.trades = getattr(s, "trades", 0) + int(traded)
    else:
        s.a = np.ascontiguousarray(rows_data).reshape(-1)
        s.trades = getattr(s, "trades", 0) + int(traded)


def mat_state(a, is_complex=False, domain=TIME, delta=1.0):
    m = mm.MatModel(a, is_complex, domain, delta)
    m.trades = 0
    return m


def _flag(value):
    if isinstance(value, (bool, np.bool_)):
        return int(value)
    if isinstance(value, (int, np.integer)) and value in (0, 1):
        return int(value)
    return None


def _index(value):
    """a non-negative integer, else None"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        return None
    return int(value) if value >= 0 else None


def _after_args(s):
    """the codes every real-data function gives after its argument errors: -1 poisoned, 4 complex, else None"""
    if poisoned(s):
        return -1
    if s.is_complex():
        return 4
    return None


# ---------------------------------------------------------------------------------------------- in place, exact
def sort_passes(n):
    tiles = -(-n // SORT_TILE)
    return 0 if tiles <= 1 else int(math.ceil(math.log2(tiles)))


def sort(s, descending=False):
    flag = _flag(descending)
    if flag is None:
        return 7
    code = _after_args(s)
    if code is not None:
        return code
    rows, n, x = grid(s)
    if rows and n:
        _store(s, np.take_along_axis(x, tsort.model_order(x, bool(flag)), axis=1), sort_passes(n) % 2)
    return 0


def rank_filter(s, half, rank, guard=None, boundary="zero"):
    half, rank = _index(half), _index(rank)
    if half is None or rank is None or (guard is not None and _index(guard) is None) or boundary not in ("zero", "wrap", "nearest"):
        return 7
    if (guard is not None and guard >= half) or rank >= trank.window_size(half, guard):
        return 7
    code = _after_args(s)
    if code is not None:
        return code
    assert half <= MAX_HALF, "the backend refuses it: not a model state"
    rows, n, x = grid(s)
    if rows and n:
        _store(s, trank.model(x, half, rank, guard, boundary).view(x.dtype), 1)
    return 0


def medfilt(s, kernel_size=3, boundary="zero"):
    k = _index(kernel_size)
    if k is None or k % 2 == 0:
        return 7
    return rank_filter(s, (k - 1) // 2, (k - 1) // 2, None, boundary)


# ---------------------------------------------------------------------------------------------- read only, exact
def _squeeze(s, a):
    return a if is_mat(s) else a[0]


def argsort(s, descending=False):
    flag = _flag(descending)
    if flag is None:
        return 7, None
    code = _after_args(s)
    if code is not None:
        return code, None
    rows, n, x = grid(s)
    order = tsort.model_order(x, bool(flag)).astype(np.int64) if rows and n else np.zeros((rows, n), np.int64)
    return 0, _squeeze(s, order)


def top_k(s, k, largest=True):
    flag, k = _flag(largest), _index(k)
    rows, n, x = grid(s)
    if flag is None or k is None or k > n:
        return 7, None
    code = _after_args(s)
    if code is not None:
        return code, None
    if rows and n and k:
        order = tsort.model_order(x, bool(flag))[:, :k].astype(np.int64)
        value = np.take_along_axis(x, order, axis=1)
    else:
        order, value = np.zeros((rows, k), np.int64), np.zeros((rows, k), x.dtype)
    return 0, {"index": _squeeze(s, order), "value": _squeeze(s, value)}


def quantile(s, q, method="linear"):
    if method not in tsort.METHODS or isinstance(q, (bool, str, bytes)) or q is None:
        return 7, None
    try:
        qs = np.asarray(q, dtype=np.float64)
    except (TypeError, ValueError):
        return 7, None
    if qs.ndim > 1 or not np.all((qs.reshape(-1) >= 0.0) & (qs.reshape(-1) <= 1.0)):
        return 7, None
    rows, n, x = grid(s)
    if n == 0:
        return 7, None
    code = _after_args(s)
    if code is not None:
        return code, None
    v = np.take_along_axis(x, tsort.model_order(x, False), axis=1)
    out = np.array([[tsort.model_quantile(v[r], qq, method) for qq in qs.reshape(-1)] for r in range(rows)], dtype=np.float64)
    out = out.reshape(rows, qs.size)
    out = _squeeze(s, out)
    return 0, (out[..., 0] if qs.ndim == 0 else out)


def median(s):
    return quantile(s, 0.5)


def _threshold(s, threshold):
    """(test_gpu_detect's kind, its threshold) of a detect argument on state s, or a code"""
    rows, n, x = grid(s)
    if threshold is None:
        return "none", None
    if isinstance(threshold, mm.MatModel):
        return ("cell", threshold) if is_mat(s) else 7
    if hasattr(threshold, "a") and hasattr(threshold, "is_complex"):
        return "profile", threshold
    if np.ndim(threshold) == 0:
        return "scalar", float(threshold)
    t = np.asarray(threshold, dtype=np.float64)
    if t.ndim != 1 or t.size != rows:
        return 7
    return ("row", t) if is_mat(s) else ("scalar", float(t[0]))


def detect(s, threshold=None, order=0, boundary="open", capacity=None):
    kt = _threshold(s, threshold)
    if _index(order) is None or boundary not in ("open", "wrap", "nearest") or (capacity is not None and _index(capacity) is None) \
            or kt == 7:
        return 7, None
    kind, t = kt
    rows, n, x = grid(s)
    if kind in ("profile", "cell") and t.a.dtype != x.dtype:
        return 2, None
    if poisoned(s) or (kind in ("profile", "cell") and poisoned(t)):
        return -1, None
    if s.is_complex() or (kind in ("profile", "cell") and t.is_complex()):
        return 4, None
    if kind == "cell":
        if t.rows() != rows:
            return 7, None
        if t.a.size != x.size:
            return 1, None
    if kind == "profile" and t.a.size != n:
        return 1, None
    if kind in ("profile", "cell"):
        if t.domain() != s.domain() or t.is_complex() != s.is_complex():
            return 2, None
        t = t.a.reshape(x.shape) if kind == "cell" else t.a.reshape(-1)
    if rows == 0 or n == 0:
        count, row, index = np.zeros(rows, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    else:
        count, row, index = tdet.model(x, kind, t, int(order), boundary)
    k = len(index) if capacity is None else min(len(index), capacity)
    value = x[row[:k], index[:k]] if k else np.zeros(0, x.dtype)
    det = {"count": count if is_mat(s) else int(count[0]), "index": index[:k], "value": value}
    if is_mat(s):
        det["row"] = row[:k]
    return 0, det


def argrelmax(s, order=1, mode="clip"):
    if _index(order) is None or order < 1 or mode not in ("clip", "wrap"):
        return 7, None
    code, det = detect(s, None, order, {"clip": "nearest", "wrap": "wrap"}[mode])
    if code != 0:
        return code, None
    return 0, ((det["row"], det["index"]) if is_mat(s) else (det["index"],))


# ---------------------------------------------------------------------------------------------- references with a bound
def sosfilt_models(s, sos, state=None):
    """test_gpu_iir.models on the rows of s: (truth y, T-precision y, truth state, T-precision state) per signal"""
    rows, n, x = grid(s)
    st = None if state is None else grid(state)[2]
    return tiir.models(np.asarray(sos, dtype=np.float64), x, st, s.dtype, s.is_complex())


def sosfilt_ratio(s, sos, state, got, got_state=None):
    """(test_gpu_iir.yardstick of the outputs, of the final states or None): both are held to test_gpu_iir.R"""
    ty, sy, ts, ss = sosfilt_models(s, sos, state)
    eps = np.finfo(s.dtype).eps
    cplx = s.is_complex()
    out = tiir.yardstick(tiir.signals(np.asarray(got).reshape(grid(s)[2].shape), cplx), ty, sy, eps)
    if got_state is None:
        return out, None
    gs = tiir.signals(np.asarray(got_state).reshape(grid(s)[0], -1), cplx)
    return out, tiir.yardstick(gs, ts, ss, eps)


def zoom_fft_reference(s, start, step, bins):
    """test_gpu_zoom_fft.model on the rows of s: complex128 [rows, bins]; start: a number or one per row"""
    rows, n, x = grid(s)
    starts = [float(start)] * rows if np.ndim(start) == 0 else list(start)
    assert len(starts) == rows
    return tzoom.model(x, s.is_complex(), starts, step, bins)


def matmul_reference(a, b, conj_transpose=False):
    """test_gpu_mat_mul.reference on two states: (reference one precision up, sum |a| |b|, K)"""
    assert a.is_complex() == b.is_complex()
    ref, mod = tmul.reference(grid(a)[2], grid(b)[2], a.is_complex(), bool(conj_transpose))
    return ref, mod, a.row_points()


def matmul_ratio(a, b, conj_transpose, out):
    ref, mod, K = matmul_reference(a, b, conj_transpose)
    return tmul.worst_ratio(np.asarray(out), ref, mod, K, a.dtype, a.is_complex())


def cholesky_ratio(a, l, loading=0.0):
    """test_gpu_mat_chol.chol_ratio of the factor l (an array) of state a, loaded as the device loads it"""
    cplx = a.is_complex()
    x = grid(a)[2]
    x = tchol.loaded(x, loading, cplx) if loading else x
    return tchol.chol_ratio(tchol.as_points(x, cplx), np.asarray(l), cplx, a.dtype)


def cholesky_solve_ratio(l, b, x, part="both"):
    """test_gpu_mat_chol.solve_ratio: l, b states, x the result as an array"""
    return tchol.solve_ratio(grid(l)[2], grid(b)[2], np.asarray(x), part, b.is_complex(), b.dtype)


def eigh_check(a, w, v, sweeps, what="eigh"):
    """test_gpu_mat_eigh.check: both bounds, the f32 eigenvalue bound and the order of w, asserted there"""
    return teigh.check(grid(a)[2], a.is_complex(), np.asarray(w).reshape(-1), np.asarray(v), sweeps, what)


# ---------------------------------------------------------------------------------------------- one step, on either side
class ModelFns:
    """the model side's namespace of module functions (the GPU side passes basic_dsp_amd itself)"""
    sort, rank_filter, medfilt = staticmethod(sort), staticmethod(rank_filter), staticmethod(medfilt)
    argsort, top_k, quantile, median = staticmethod(argsort), staticmethod(top_k), staticmethod(quantile), staticmethod(median)
    detect, argrelmax = staticmethod(detect), staticmethod(argrelmax)


MODULE_STEPS = ("sort", "medfilt", "rank_filter")
BOUNDARIES = ("zero", "wrap", "nearest")
# the in-place module operations coverage() tells apart
IN_PLACE = ("sort(ascending)", "sort(descending)", "medfilt(3)", "medfilt(5)") + \
    tuple("rank_filter(%s%s)" % (b, g) for b in BOUNDARIES for g in ("", ", guard"))


def variant(step):
    if step[0] == "sort":
        return "sort(%s)" % ("descending" if step[1] else "ascending")
    if step[0] == "medfilt":
        return "medfilt(%d)" % step[1]
    return "rank_filter(%s%s)" % (step[4], "" if step[3] is None else ", guard")


# How often a matrix mover trades the live and the trade buffer of the matrix it runs on, for a matrix with data (the
# generator's states always have some), read from capi.cpp: mat_transpose, mat_zero_pad, op_swap (swap_halves, fft_shift,
# ifft_shift), op_reverse, mat_zero_interleave (factor > 1), op_decimatei (a result with points), mat_mirror, op_to_complex
# and op_complex_to_real (to_real, to_imag) write the trade buffer and trade once; conj and set_row write in place.  The
# steps between matrices leave the source alone and go on with another matrix, which starts at 0.
MAT_MOVER_TRADES = dict(transpose=1, zero_pad=1, swap_halves=1, fft_shift=1, ifft_shift=1, reverse=1, zero_interleave=1,
                        decimatei=1, mirror=1, to_complex=1, to_real=1, to_imag=1, conj=0, row_move=0)


def apply_step(kind, fns, api, obj, step):
    """Runs `step` on obj of either side.  A module step (MODULE_STEPS) calls fns.<name>(obj, *args) in place; every
    other step is a mover and goes to mat_model.apply_step / vec_model.apply_step with the side's `api`.  Returns what
    they return: (codes, the object the sequence goes on with, the other objects the step read or wrote).  On a MatModel
    the mover's trades are counted too."""
    if step[0] in MODULE_STEPS:
        return [getattr(fns, step[0])(obj, *step[1:])], obj, []
    if kind == "vec":
        return vm.apply_step(api, obj, step)
    before = trades(obj) if is_mat(obj) else 0
    codes, nxt, side = mm.apply_step(api, obj, step)
    if is_mat(nxt):
        traded = (step[0] != "zero_interleave" or step[1] > 1) and nxt.a.size > 0
        nxt.trades = before + MAT_MOVER_TRADES[step[0]] * int(traded) if nxt is obj else 0
    return codes, nxt, side


# ---------------------------------------------------------------------------------------------- the sequence generator
START_SHAPES = ((5, 1001), (3, 4097), (2, 8209), (257, 100), (1, 1), (7, 16))   # matrices: (rows, points)
START_POINTS = (1, 16, 1001, 4097, 8209, 20483)                                  # vectors
MAT_SEEDS = (0, 1, 2, 3, 4, 9)   # chosen on the CPU: tests/test_module_model.py asserts what they cover
VEC_SEEDS = tuple(range(6))
EXACT_FIT_AT = (4, 10)   # as vm.EXACT_FIT_AT: the step that fills the allocation where the state allows it; a module
#                          operation follows at the next step
MAX_ROWS = 1024          # of a generated matrix state: the quantile model is a Python loop per row
# overlap_add ("frames") adds +0 to every scalar: a sequence that holds it starts from data without edge values (what an
# adder makes of a signalling NaN or of -0 is the business of overlap_add's own tests)
ARITHMETIC_MOVERS = ("frames",)


def _module_candidate(rng):
    """one in-place module step, the variant drawn uniformly"""
    k = int(rng.randint(len(IN_PLACE)))
    if k < 2:
        return ("sort", bool(k))
    if k < 4:
        return ("medfilt", 3 if k == 2 else 5)
    boundary, guarded = BOUNDARIES[(k - 4) // 2], (k - 4) % 2 == 1
    half = int((2, 3, 7)[rng.randint(3)]) if guarded else int((1, 2, 3, 7)[rng.randint(4)])
    guard = int(rng.randint(half)) if guarded else None
    return ("rank_filter", half, int(rng.randint(trank.window_size(half, guard))), guard, boundary)


def _modelable(s):
    """real data, every scalar specified: the states an exact module operation can run on"""
    return not s.is_complex() and not (hasattr(s, "unspec") and s.unspec.any())


def _mat_exact_fit_step(s, rng):
    e, rows, n = s._e(), s.rows(), s.a.size
    if n >= s.cap or s.cap % (rows * e) or s.cap > MAX_SCALARS:
        return None
    return ("zero_pad", s.cap // (rows * e), int(rng.randint(3)))


def _dry(kind, s, step):
    """(the state after `step` on a copy, whether it is still the same object) -- the generator's data are zeros: only the
    shape, the capacity and the trades matter -- or None where the step does not leave 1 <= scalars <= MAX_SCALARS"""
    c = copy.deepcopy(s)
    codes, nxt, _ = apply_step(kind, _Dry, mm.ModelApi if kind == "mat" else vm.ModelApi, c, step)
    ok = all(code in (0, 9) for code in codes) and not poisoned(nxt) and 1 <= nxt.a.size <= MAX_SCALARS
    ok = ok and (kind == "vec" or nxt.rows() <= MAX_ROWS)
    return (nxt, nxt is c) if ok else None


class _Dry:
    """the module steps without their data: the generator needs the trades only"""

    @staticmethod
    def sort(s, descending):
        _store(s, grid(s)[2], sort_passes(grid(s)[1]) % 2)
        return 0

    @staticmethod
    def rank_filter(s, *args):
        _store(s, grid(s)[2], 1)
        return 0

    @staticmethod
    def medfilt(s, k):
        _store(s, grid(s)[2], 1)
        return 0


def gen_module_sequence(rows, points, seed, steps=STEPS):
    """The steps of one sequence from a REAL matrix of rows x points (rows=None: a vector of `points` points) and, per
    step, the history it ran in.  Deterministic in its arguments; dtype and domain play no part.  Each step is a mover
    of the existing tables (mm._candidates / vm._candidates) or, on a real state with every
    scalar specified and every second time at most, an in-place module operation."""
    kind = "vec" if rows is None else "mat"
    rng = np.random.RandomState(seed * 1013 + (rows or 0) * 37 + points * 11 + 5)
    if kind == "mat":
        s = mat_state(np.zeros((rows, points), np.float32), False)
    else:
        s = vm.VecModel(np.zeros(points, np.float32), False)
    seq, log = [], []
    for i in range(steps):
        movers = (mm if kind == "mat" else vm)._candidates(s, rng)
        module = _module_candidate(rng)
        pick_module = bool(rng.randint(2))
        order = list(rng.permutation(len(movers)))
        step = None
        if i in EXACT_FIT_AT:
            step = (_mat_exact_fit_step if kind == "mat" else vm._exact_fit_step)(s, rng)
            if step is not None and _dry(kind, s, step) is None:
                step = None
        if step is None and _modelable(s) and (pick_module or (i - 1 in EXACT_FIT_AT and s.a.size == s.cap)):
            step = module
        res = None if step is None else _dry(kind, s, step)
        while res is None:   # the first mover of the drawn order that keeps the state within bounds
            step = movers[order.pop(0)]
            res = _dry(kind, s, step)
        nxt, same = res   # (another object than s starts without reallocations and without trades)
        log.append(dict(step=step, op=variant(step) if step[0] in MODULE_STEPS else None,
                        odd_trades=trades(s) % 2 == 1, exact_fit=s.a.size == s.cap,
                        realloc=nxt.reallocs > (s.reallocs if same else 0), shrink=nxt.a.size < s.a.size,
                        space_change=nxt.is_complex() != s.is_complex()))
        seq.append(step)
        s = nxt
    return seq, log


def all_module_sequences():
    """(rows or None, points, seed) of every generated sequence: the dtype multiplies them in the GPU test"""
    return [(r, p, s) for (r, p) in START_SHAPES for s in MAT_SEEDS] + [(None, p, s) for p in START_POINTS for s in VEC_SEEDS]


HISTORIES = vm.HISTORIES


def coverage(logs):
    """{in-place module operation: count and, per history of vm.HISTORIES, how often it ran with it}: after_* -- the event
    happened at an earlier step of the sequence; odd_trades / exact_fit -- the state the step started from"""
    cov = {op: dict(count=0, **{h: 0 for h in HISTORIES}) for op in IN_PLACE}
    for log in logs:
        seen = dict(realloc=False, shrink=False, space_change=False)
        for ev in log:
            if ev["op"] is not None:
                c = cov[ev["op"]]
                c["count"] += 1
                for k in seen:
                    c["after_" + k] += int(seen[k])
                c["odd_trades"] += int(ev["odd_trades"])
                c["exact_fit"] += int(ev["exact_fit"])
            for k in seen:
                seen[k] = seen[k] or ev[k]
    return cov


# ---------------------------------------------------------------------------------------------- dirty states, long rows
# The smallest shapes at which the multi-launch routes run, as mover recipes in the style of mm.DIRTY.
#
# L1: 3 x 8200 decimated to 3 x 4100: two sort tiles (one merge pass: an odd pass count, so sort trades), two sosfilt tiles
#     (the three-launch carry route), five detect tiles.
# L2: 2 x 8000 real scalars start with cap = 16000 + 16000 / 8 + 64 = 18064 = 2 * 9032, so zero_pad(9032) needs exactly
#     the allocation: no reallocation, no scalar of slack behind the last row; three sort tiles (two merge passes), and the
#     padded zeros are a long run of ties.
# L3: 4100 x 3 transposed on the device to 3 x 4100.
LONG_DIRTY = {
    "L1-shrunk-two-tiles": dict(shape=(3, 8200), is_complex=None, steps=[("decimatei", 2, 0)]),
    "L2-exact-fit-three-tiles": dict(shape=(2, 8000), is_complex=False, steps=[("zero_pad", 9032, PAD_END)]),
    "L3-transposed-long": dict(shape=(4100, 3), is_complex=None, steps=[("transpose",)]),
}
# The vector counterparts, in vm.DIRTY's vocabulary.  set_len counts scalars: 8201 points end as 8200 real or 4100
# complex ones.  exact fit: 4000 real scalars start with cap = 4000 + 500 + 64 = 4564 > 4096, and zero_pad(4564) needs
# exactly the allocation: two sort tiles.
LONG_DIRTY_VEC = {
    "shrunk-by-set_len": dict(points=8201, is_complex=None, steps=[("set_len", 8200)]),
    "odd-trades": dict(points=4100, is_complex=None, steps=[("swap_halves",)]),
    "exact-fit-real": dict(points=4000, is_complex=False, steps=[("zero_pad", 4564, PAD_END)]),
}


def build_long(api, name, fill, is_complex, domain, delta):
    """The long dirty matrix `name` on side `api` (mm.build_dirty's contract): fill(rows, scalars per row)"""
    d = LONG_DIRTY[name]
    rows, pts = d["shape"]
    m = api.mat(fill(rows, pts * (2 if is_complex else 1)), is_complex, domain, delta)
    for step in d["steps"]:
        codes, m, _ = mm.apply_step(api, m, step)
        assert all(c == 0 for c in codes), (name, step, codes)
    return m


def build_long_vec(api, name, fill, is_complex, domain, delta):
    """The long dirty vector `name` on side `api` (vm.build_dirty's contract): fill(scalars, k)"""
    d = LONG_DIRTY_VEC[name]
    v = api.vec(fill(d["points"] * (2 if is_complex else 1), 0), is_complex, domain, delta)
    for step in d["steps"]:
        codes, v, _ = vm.apply_step(api, v, step)
        assert all(c == 0 for c in codes), (name, step, codes)
    return v


# ---------------------------------------------------------------------------------------------- Hermitian states
# A Hermitian positive-definite A of order N (test_gpu_mat_chol.spd: G G^H / 2N + 0.1 I) reached on the device by a history.
# H3's A exists on the device only: A = B B^H by matmul, B = G / sqrt(2N) of N x 2N, so the result of one module call is
# the operand of the next; the side that has no matmul (the model) gets the product one precision up, rounded.
# H4: a square matrix that ends on the last scalar of its allocation.  64 x 56 real scalars start with cap = 3584 + 448 + 64
# = 4096 = 64 x 64, so zero_pad(64) needs exactly the allocation; the zero matrix then takes A by the library's `add`
# (+0 + a is a, to the bit, for the finite non-zero-signed values of A).  Real, N = 64 only: the arithmetic gives no other.
HERMITIAN = ("H1-transposed", "H2-decimated", "H3-product")
EXACT_FIT_HERMITIAN = "H4-exact-fit"
H4_N, H4_START_POINTS = 64, 56
# one N on each side of each route boundary the shapes files name: one launch up to 64, blocks above; 130 is the largest
# blocked order the linalg tests share (three blocks for cholesky, five block columns for eigh)
CHOLESKY_N = (64, 65, 130)
EIGH_N = (64, 65, 130)


def hermitian_source(name, N, cplx, dtype):
    """(the array to upload [rows, scalars], the movers or module call that make A of it)"""
    e = 2 if cplx else 1
    if name == "H3-product":
        rng = np.random.default_rng(8100 + 7 * N + int(cplx))
        g = rng.standard_normal((N, 2 * N * e)) / np.sqrt(2.0 * N)
        return g.astype(dtype), "gram"
    a = np.array(tchol.spd(N, cplx, dtype))
    if name == "H1-transposed":   # conj(A) transposed is A^H to the bit: A, up to the last bit of A's construction on the host
        c = a.copy()
        if cplx:
            c[:, 1::2] = mm._flip_sign(c[:, 1::2])
        return c, [("transpose",)]
    assert name == "H2-decimated"   # A's points in the even columns, junk in the odd ones
    rng = np.random.default_rng(8200 + N)
    wide = rng.standard_normal((N, 2 * N, e)).astype(dtype)
    wide[:, 0::2, :] = a.reshape(N, N, e)
    return wide.reshape(N, 2 * N * e), [("decimatei", 2, 0)]


def build_hermitian(api, name, N, cplx, dtype, domain, delta, matmul=None):
    """The Hermitian state `name` of order N on side `api`.  matmul(b, b, conj_transpose=True) -> (code, matrix): the
    side's product, for H3 (None: the model's, one precision up and rounded to dtype)."""
    if name == EXACT_FIT_HERMITIAN:
        assert N == H4_N and not cplx
        a = np.array(tchol.spd(N, False, dtype))
        m = api.mat(np.zeros((N, H4_START_POINTS), dtype), False, domain, delta)
        codes, m, _ = mm.apply_step(api, m, ("zero_pad", N, PAD_END))
        assert codes == [0]
        if is_mat(m):
            m.a = m.a + a
        else:
            assert m.add(api.mat(a, False, domain, delta)) == 0
        return m
    src, how = hermitian_source(name, N, cplx, dtype)
    m = api.mat(src, cplx, domain, delta)
    if how == "gram":
        if matmul is not None:
            code, a = matmul(m, m, conj_transpose=True)
            assert code == 0
            return a
        p = tmul.as_points(src, cplx).astype(np.complex128 if cplx else np.float64)
        g = np.tril(p @ p.conj().T)   # Hermitian to the bit, as matmul's Gram matrix is: the lower triangle mirrored
        g = g + np.tril(g, -1).conj().T
        if cplx:
            np.fill_diagonal(g, g.diagonal().real)
        return api.mat(tchol.as_scalars(g, dtype), cplx, domain, delta)
    for step in how:
        codes, m, _ = mm.apply_step(api, m, step)
        assert all(c == 0 for c in codes), (name, step, codes)
    return m
