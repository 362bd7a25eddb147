"""tests/module_model.py and the tables of tests/test_gpu_module_sequences.py, on the CPU: the wrapped models agree with
what they wrap, the recipes reach the states they name, the generator is deterministic and its seed lists cover every
in-place module operation in every history, every module function of basic_dsp_amd is catalogued for every class it
accepts, and every code a docstring names has a row."""
import inspect
import re

import numpy as np
import pytest

import mat_model as mm
import module_model as M
import vec_model as vm
from mat_model import FREQ, TIME
from module_model import tchol, tdet, tiir, tmul, trank, tsort, tzoom


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _states(x):
    """the same rows as a matrix state and the first row as a vector state"""
    return M.mat_state(x), vm.VecModel(x[0])


# ---------------------------------------------------------------------------------------------- the wrapped models
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
def test_wrapped_exact_models_agree_with_what_they_wrap(dtype):
    """one small case each, every argument given a value that is not its default: a wrapper cannot drop one"""
    x = tsort.draw(5, 3, 37, dtype, "edge")
    asc, desc = tsort.model_order(x, False), tsort.model_order(x, True)
    for s, rows in zip(_states(x), (slice(None), 0)):
        pick = lambda a: a[rows]
        t = (M.mat_state if M.is_mat(s) else vm.VecModel)(pick(x))
        assert M.sort(t, True) == 0 and np.array_equal(_bits(t.a), tsort.take(x, desc)[rows]) and M.trades(t) == 0
        t = (M.mat_state if M.is_mat(s) else vm.VecModel)(pick(x))
        assert M.sort(t) == 0 and np.array_equal(_bits(t.a), tsort.take(x, asc)[rows])
        assert np.array_equal(M.argsort(s, True)[1], desc[rows]) and np.array_equal(M.argsort(s)[1], asc[rows])
        code, top = M.top_k(s, 5, largest=False)
        assert code == 0 and np.array_equal(top["index"], asc[rows][..., :5]) and np.array_equal(_bits(top["value"]), tsort.take(x, asc)[rows][..., :5])
        v = tsort.take(x, asc).view(dtype)
        for method in tsort.METHODS:
            code, q = M.quantile(s, [0.1, 0.999], method)
            want = np.array([[tsort.model_quantile(v[r], qq, method) for qq in (0.1, 0.999)] for r in range(3)])[rows]
            assert code == 0 and q.shape == want.shape and np.array_equal(np.isnan(q), np.isnan(want)) and np.array_equal(q[~np.isnan(q)], want[~np.isnan(want)])
        code, med = M.median(s)
        assert code == 0 and np.array_equal(_bits(med), _bits(M.quantile(s, 0.5)[1])) and med.shape == ((3,) if M.is_mat(s) else ())
        # rank_filter / medfilt: test_gpu_rank_filter.model, every argument
        t = (M.mat_state if M.is_mat(s) else vm.VecModel)(pick(x))
        assert M.rank_filter(t, 4, 2, 1, "wrap") == 0 and M.trades(t) == 1
        assert np.array_equal(_bits(t.a), trank.model(x, 4, 2, 1, "wrap")[rows])
        t = (M.mat_state if M.is_mat(s) else vm.VecModel)(pick(x))
        assert M.medfilt(t, 5, "nearest") == 0 and np.array_equal(_bits(t.a), trank.model(x, 2, 2, None, "nearest")[rows])
        # detect / argrelmax: test_gpu_detect.model
        count, row, index = tdet.model(x if M.is_mat(s) else x[:1], "scalar", -0.25, 2, "wrap")
        code, det = M.detect(s, -0.25, 2, "wrap", capacity=4)
        assert code == 0 and np.array_equal(det["index"], index[:4]) and np.array_equal(np.asarray(det["count"]).reshape(-1), count)
        assert np.array_equal(_bits(det["value"]), _bits((x if M.is_mat(s) else x[:1])[row[:4], index[:4]]))
        assert ("row" in det) == M.is_mat(s) and (not M.is_mat(s) or np.array_equal(det["row"], row[:4]))
        count, row, index = tdet.model(x if M.is_mat(s) else x[:1], "none", None, 3, "nearest")
        code, rel = M.argrelmax(s, 3, "clip")
        assert code == 0 and np.array_equal(rel[-1], index) and (not M.is_mat(s) or np.array_equal(rel[0], row))
    # the device thresholds: a profile for all rows, one value per cell
    m = M.mat_state(x)
    prof, cell = vm.VecModel(x[1]), M.mat_state(x[::-1].copy())
    assert np.array_equal(M.detect(m, prof)[1]["index"], tdet.model(x, "profile", x[1], 0, "open")[2])
    assert np.array_equal(M.detect(m, cell, 1)[1]["index"], tdet.model(x, "cell", x[::-1], 1, "open")[2])
    assert np.array_equal(M.detect(m, [0.0, 0.5, -0.5])[1]["count"], tdet.model(x, "row", [0.0, 0.5, -0.5], 0, "open")[0])


def test_wrapped_models_answer_the_documented_codes_in_the_documented_order():
    x = tsort.draw(6, 2, 8, np.float32, "uniform")
    real, cplx = M.mat_state(x), M.mat_state(x, True)
    dead = M.mat_state(x)
    assert dead.conj() == -1 and M.poisoned(dead)
    vdead = vm.VecModel(x[0])
    assert vdead.conj() == -1 and M.poisoned(vdead)
    for s, code in ((cplx, 4), (dead, -1), (vdead, -1)):
        assert M.sort(s) == code and M.rank_filter(s, 1, 1) == code and M.medfilt(s, 3) == code
        assert M.argsort(s) == (code, None) and M.top_k(s, 0) == (code, None) and M.detect(s, 0.5) == (code, None)
        assert M.argrelmax(s) == (code, None)
        assert M.sort(s, 2) == 7 and M.rank_filter(s, 1, 3) == 7 and M.medfilt(s, 4) == 7 and M.top_k(s, 99) == (7, None)   # 7 comes first
        assert M.detect(s, None, -1) == (7, None) and M.argrelmax(s, 0) == (7, None) and M.quantile(s, 1.5) == (7, None)
    assert M.quantile(cplx, 0.5) == (4, None) and M.quantile(dead, 0.5) == (7, None)   # rows of no points: 7 before the device is asked
    assert M.rank_filter(real, 2, 0, 2) == 7 and M.rank_filter(real, 2, 0, boundary="mirror") == 7 and M.quantile(real, 0.5, "nearest") == (7, None)
    assert M.detect(real, [0.0] * 3) == (7, None) and M.detect(vm.VecModel(x[0]), M.mat_state(x[:1])) == (7, None)
    assert M.detect(real, vm.VecModel(x[0].astype(np.float64))) == (2, None)            # precision before everything on the device
    assert M.detect(real, vm.VecModel(x[0, :7])) == (1, None) and M.detect(real, M.mat_state(x[:1])) == (7, None)
    assert M.detect(real, vm.VecModel(x[0], False, FREQ)) == (2, None)
    assert np.array_equal(_bits(real.a), _bits(x)) and M.trades(real) == 0   # nothing of it touched the data


def test_wrapped_references_agree_with_what_they_wrap():
    dtype = np.float32
    # sosfilt: test_gpu_iir.models / yardstick, with a state
    x = tiir.draw(3, 2, 50, dtype, True)
    st = tiir.draw(4, 2, 4, dtype, True)
    sos = tiir.make_sos("resonator", 2)
    s, state = M.mat_state(x, True), M.mat_state(st, True)
    ty, sy, ts, ss = tiir.models(sos, x, st, dtype, True)
    for got, want in zip(M.sosfilt_models(s, sos, state), (ty, sy, ts, ss)):
        assert np.array_equal(got, want)
    assert not np.array_equal(M.sosfilt_models(s, sos)[0], ty)   # (the state is an argument that matters)
    unrolled = np.stack([sy[0::2], sy[1::2]], axis=-1).reshape(2, -1)   # [rows * 2, n] signals back to interleaved rows
    fin = np.stack([ss[0::2], ss[1::2]], axis=-1).reshape(2, -1)
    assert M.sosfilt_ratio(s, sos, state, unrolled, fin) == (tiir.yardstick(sy, ty, sy, np.finfo(dtype).eps), tiir.yardstick(ss, ts, ss, np.finfo(dtype).eps))
    # zoom_fft: test_gpu_zoom_fft.model, one start and one per row
    r = M.mat_state(tzoom.make_rows(2, 20, False, dtype, 1, None))
    assert np.array_equal(M.zoom_fft_reference(r, 0.1, 0.01, 7), tzoom.model(r.a, False, [0.1, 0.1], 0.01, 7))
    assert np.array_equal(M.zoom_fft_reference(r, [0.1, 0.3], 0.01, 7), tzoom.model(r.a, False, [0.1, 0.3], 0.01, 7))
    v = vm.VecModel(tzoom.make_rows(1, 20, True, dtype, 2, None)[0], True)
    assert np.array_equal(M.zoom_fft_reference(v, 0.2, 0.02, 5), tzoom.model(v.a.reshape(1, -1), True, [0.2], 0.02, 5))
    # matmul: test_gpu_mat_mul.reference / worst_ratio, both forms
    a, b = tmul.operands(1, 3, 5, 4, True, False, dtype)
    _, bt = tmul.operands(1, 3, 5, 4, True, True, dtype)
    for trans, second in ((False, b), (True, bt)):
        ref, mod = tmul.reference(a, second, True, trans)
        got = M.matmul_reference(M.mat_state(a, True), M.mat_state(second, True), trans)
        assert np.array_equal(got[0], ref) and np.array_equal(got[1], mod) and got[2] == 5
        out = tchol.as_scalars(ref, dtype)
        assert M.matmul_ratio(M.mat_state(a, True), M.mat_state(second, True), trans, out) == tmul.worst_ratio(out, ref, mod, 5, dtype, True)
    # cholesky / cholesky_solve: test_gpu_mat_chol's ratios on numpy's own factor, with and without loading
    for cplx in (False, True):
        spd = np.array(tchol.spd(6, cplx, dtype))
        A = M.mat_state(spd, cplx)
        for loading in (0.0, 0.25):
            lo = tchol.loaded(spd, loading, cplx) if loading else spd
            l = tchol.as_scalars(np.linalg.cholesky(tchol.as_points(lo, cplx).astype(np.complex128 if cplx else np.float64)), dtype)
            assert M.cholesky_ratio(A, l, loading) == tchol.chol_ratio(tchol.as_points(lo, cplx), l, cplx, dtype) <= 1.0
        assert M.cholesky_ratio(A, l, 0.0) > 1.0   # (the loading is an argument that matters)
        rhs = tchol.rhs(6, 2, cplx, dtype)
        sol = tchol.as_scalars(np.linalg.solve(tchol.lower_of(l, cplx).astype(np.complex128), tchol.as_points(rhs, cplx)) if cplx else
                               np.linalg.solve(tchol.lower_of(l, cplx).astype(np.float64), rhs), dtype)
        for part in ("forward", "backward"):
            assert M.cholesky_solve_ratio(M.mat_state(l, cplx), M.mat_state(rhs, cplx), sol, part) == tchol.solve_ratio(l, rhs, sol, part, cplx, dtype)
        assert M.cholesky_solve_ratio(M.mat_state(l, cplx), M.mat_state(rhs, cplx), sol, "forward") <= 1.0
        # eigh: test_gpu_mat_eigh.check on numpy's decomposition (v's rows are the eigenvectors conjugate-transposed)
        lam, vec = np.linalg.eigh(tchol.as_points(spd, cplx).astype(np.complex128 if cplx else np.float64))
        rr, ro = M.eigh_check(A, lam.astype(dtype), tchol.as_scalars(vec.conj().T, dtype), 3)
        assert rr <= 1.0 and ro <= 1.0
        with pytest.raises(AssertionError):
            M.eigh_check(A, lam[::-1].astype(dtype), tchol.as_scalars(vec.conj().T, dtype), 3)


# ---------------------------------------------------------------------------------------------- the recipes
def test_long_recipes_reach_the_states_they_name():
    fill = lambda rows, scalars: np.arange(rows * scalars, dtype=np.float32).reshape(rows, scalars)
    build = lambda name, cplx: M.build_long(mm.ModelApi, name, fill, cplx, TIME, 1.0)
    for cplx in (False, True):
        l1 = build("L1-shrunk-two-tiles", cplx)
        assert (l1.rows(), l1.row_points()) == (3, 4100) and l1.cap > 2 * l1.a.size and l1.reallocs == 0
        l3 = build("L3-transposed-long", cplx)
        assert (l3.rows(), l3.row_points()) == (3, 4100)
    # L1 real: two tiles of sort (one merge pass: a trade), two of sosfilt (the carry route), five of detect
    assert M.sort_passes(4100) == 1 and -(-4100 // M.IIR_TILE) == 2 and -(-4100 // M.DETECT_TILE) == 5
    l2 = build("L2-exact-fit-three-tiles", False)
    assert (l2.rows(), l2.row_len()) == (2, 9032) and l2.cap == l2.a.size == 18064 == mm.grown_cap(16000) and l2.reallocs == 0
    assert M.sort_passes(9032) == 2 and not l2.a[:, 8000:].any()
    assert M.SORT_TILE == 4096 == M.IIR_TILE and M.DETECT_TILE == 1024

    vfill = lambda n, k: np.arange(n, dtype=np.float32) + 1000 * k
    vbuild = lambda name, cplx: M.build_long_vec(vm.ModelApi, name, vfill, cplx, TIME, 1.0)
    s = vbuild("shrunk-by-set_len", False)
    assert s.len() == 8200 and s.cap == vm.grown_cap(8201) and s.trades == 0 and not s.unspec.any()
    assert vbuild("shrunk-by-set_len", True).points() == 4100
    for cplx in (False, True):
        o = vbuild("odd-trades", cplx)
        assert o.points() == 4100 and o.trades % 2 == 1 and o.reallocs == 0
    e = vbuild("exact-fit-real", False)
    assert e.len() == e.cap == 4564 == vm.grown_cap(4000) and e.reallocs == 0 and e.len() > M.SORT_TILE and M.sort_passes(e.len()) == 1
    # the module operations' own trades: an odd pass count trades, an even one does not, rank_filter always
    for n, traded in ((4096, 0), (4097, 1), (8193, 0), (16385, 1)):
        v = vm.VecModel(np.zeros(n, np.float32))
        assert M.sort(v) == 0 and v.trades == traded, n
    v = vm.VecModel(np.zeros(9, np.float32))
    assert M.medfilt(v, 3) == 0 and M.rank_filter(v, 2, 0, 1, "wrap") == 0 and v.trades == 2


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
def test_hermitian_recipes_reach_a_positive_definite_matrix(dtype):
    assert M.HERMITIAN == ("H1-transposed", "H2-decimated", "H3-product") and M.EXACT_FIT_HERMITIAN == "H4-exact-fit"
    # H4: 64 x 56 real scalars fill cap = 4096 = 64 x 64 after zero_pad(64): no reallocation, no slack, and A to the bit
    h4 = M.build_hermitian(mm.ModelApi, "H4-exact-fit", 64, False, dtype, TIME, 0.5)
    assert mm.grown_cap(64 * 56) == 4096 == h4.cap == h4.a.size and h4.reallocs == 0 and (h4.rows(), h4.row_points()) == (64, 64)
    assert np.array_equal(_bits(h4.a), _bits(np.array(tchol.spd(64, False, dtype)))) and M.H4_N in M.CHOLESKY_N and M.H4_N in M.EIGH_N
    for fn_orders, shapes in ((M.CHOLESKY_N, tchol.SHAPES), (M.EIGH_N, M.teigh.SHAPES)):
        small = max(s[1] for s in shapes if s[0] == "small")
        blocked = min(s[1] for s in shapes if s[0] == "blocked")
        assert len(fn_orders) <= 3 and small in fn_orders and blocked in fn_orders and blocked == small + 1 and max(fn_orders) <= 130
    for cplx in (False, True):
        for N in (5, 64):
            a = np.array(tchol.spd(N, cplx, dtype))
            # H1 is conj(A) transposed, A^H to the bit: A itself up to the last bit of A's own construction on the host
            ah = tchol.as_scalars(tchol.as_points(a, cplx).conj().T, dtype)
            assert np.allclose(ah, a, rtol=0, atol=4 * np.finfo(dtype).eps * np.abs(a).max())
            for name, want in (("H1-transposed", ah), ("H2-decimated", a)):
                m = M.build_hermitian(mm.ModelApi, name, N, cplx, dtype, TIME, 0.5)
                assert (m.rows(), m.row_points(), m.is_complex()) == (N, N, cplx) and np.array_equal(_bits(m.a), _bits(want)), (name, N)
            src, how = M.hermitian_source("H2-decimated", N, cplx, dtype)
            assert src.shape == (N, 2 * N * (2 if cplx else 1)) and how == [("decimatei", 2, 0)]
            h3 = M.build_hermitian(mm.ModelApi, "H3-product", N, cplx, dtype, TIME, 0.5)
            p = tchol.as_points(h3.a, cplx).astype(np.complex128 if cplx else np.float64)
            assert (h3.rows(), h3.row_points()) == (N, N) and np.array_equal(p, p.conj().T) and np.linalg.eigvalsh(p).min() > 0.01


# ---------------------------------------------------------------------------------------------- the generator
@pytest.fixture(scope="module")
def logs():
    return {key: M.gen_module_sequence(*key) for key in M.all_module_sequences()}


def test_the_generator_is_deterministic_and_stays_in_bounds(logs):
    assert M.START_SHAPES == ((5, 1001), (3, 4097), (2, 8209), (257, 100), (1, 1), (7, 16))
    assert M.START_POINTS == (1, 16, 1001, 4097, 8209, 20483)
    assert len(logs) == 6 * len(M.MAT_SEEDS) + 6 * len(M.VEC_SEEDS)
    for key in list(logs)[::5]:
        assert M.gen_module_sequence(*key)[0] == logs[key][0]
    known = set(mm.STEP_MOVERS) | set(vm.STEP_MOVERS) | set(M.MODULE_STEPS)
    for (rows, pts, seed), (seq, log) in logs.items():
        assert len(seq) == M.STEPS == 16 and all(step[0] in known for step in seq)
        # replayed with data: every state is within bounds, and a module step only ever meets real, specified data
        kind = "vec" if rows is None else "mat"
        s = vm.VecModel(np.zeros(pts, np.float32)) if rows is None else M.mat_state(np.zeros((rows, pts), np.float32))
        for step in seq:
            if step[0] in M.MODULE_STEPS:
                assert not s.is_complex() and not (kind == "vec" and s.unspec.any()), (rows, pts, seed, step)
            codes, s, _ = M.apply_step(kind, M._Dry, mm.ModelApi if kind == "mat" else vm.ModelApi, s, step)
            assert all(c in (0, 9) for c in codes) and 1 <= s.a.size <= M.MAX_SCALARS, (rows, pts, seed, step)
    assert M.MAX_SCALARS <= mm.MAX_SCALARS and M.MAX_SCALARS <= vm.MAX_SCALARS


def test_the_seed_lists_cover_every_in_place_module_operation_in_every_history(logs):
    """the condition the GPU test's worth rests on, from the generator alone: more seeds if it fails, never a weaker
    condition"""
    assert M.HISTORIES == vm.HISTORIES == ("after_realloc", "after_shrink", "after_space_change", "odd_trades", "exact_fit")
    for kind in ("mat", "vec"):
        cov = M.coverage([log for (rows, _, _), (_, log) in logs.items() if (rows is None) == (kind == "vec")])
        assert set(cov) == set(M.IN_PLACE) and len(M.IN_PLACE) == 10
        for op, c in cov.items():
            assert c["count"] >= 3, (kind, op, c)
            for h in M.HISTORIES:
                assert c[h] >= 1, (kind, op, "never ran in the history", h)


# ---------------------------------------------------------------------------------------------- the catalogue
# (these import basic_dsp_amd for the docstrings, which loads the built library as the *_abi tests do: they need build()
# to have run, not a GPU)
NOT_FUNCTIONS = ("require_gpu", "last_error", "lib")


def _module_functions():
    import basic_dsp_amd as bd
    out = {}
    for name in bd.__all__:
        obj = getattr(bd, name)
        if name in NOT_FUNCTIONS or inspect.isclass(obj) or not callable(obj):
            continue
        out[name] = obj
    return out


def _accepts_a_vector(fn):
    return "DspVec" in (inspect.getdoc(fn) or "") and "DspVec" in inspect.getsource(fn)


def test_every_module_function_is_catalogued_for_every_class_it_accepts():
    """a module function added later without an entry in MODULE_CATALOGUE fails here, without a GPU"""
    import test_gpu_module_sequences as seqs
    fns = _module_functions()
    assert set(fns) == {"zoom_fft", "matmul", "cholesky", "cholesky_solve", "eigh", "sosfilt", "rank_filter", "medfilt", "detect",
                        "argrelmax", "sort", "argsort", "top_k", "quantile", "median"}, "a new module function: extend the catalogue and this list"
    takes_vec = {n for n, f in fns.items() if _accepts_a_vector(f)}
    assert takes_vec == set(fns) - {"matmul", "cholesky", "cholesky_solve", "eigh"}
    for kind, wanted in (("mat", set(fns)), ("vec", takes_vec)):
        have = {e.fn for e in seqs.MODULE_CATALOGUE if kind in e.kinds}
        assert wanted <= have, "no entry for %s: %s" % (kind, sorted(wanted - have))
        assert have <= set(fns)
    labels = {e.label for e in seqs.MODULE_CATALOGUE}
    # the entries the issue names
    for must in ("zoom_fft(fits)", "zoom_fft(reallocates)", "zoom_fft(2200 bins)", "zoom_fft(64 bins, per-row starts)",
                 "sosfilt(2 sections, none state)", "sosfilt(16 sections, dirty state)", "sosfilt(2 sections, fresh state)",
                 "rank_filter(half 1)", "rank_filter(above the crossover)", "medfilt(5)", "detect(profile)", "detect(per cell)",
                 "detect(capacity below the total)", "sort(ascending)", "sort(descending)", "argsort(descending)", "top_k(1, largest)",
                 "top_k(8, smallest)", "top_k(n, largest)", "quantile(linear)", "quantile(lower)", "quantile(higher)", "median",
                 "matmul(plain, first dirty)", "matmul(conj_transpose, second dirty)", "matmul(plain, both dirty)", "cholesky(loading 0)",
                 "cholesky(loading 0.25)", "cholesky_solve(forward)", "cholesky_solve(backward)", "cholesky_solve(both)", "eigh",
                 "chain matmul -> cholesky -> cholesky_solve -> matmul"):
        assert must in labels, must


def test_every_entry_meets_the_classes_of_state_it_needs():
    """from the tables and the model states alone: among the states on which an entry's function is defined (where the
    GPU test demands the answer 0, and only an answer of 0 counts there) are a shrunk, a moved (transposed or odd trades),
    an exact-fit (real functions) and an empty one -- but for quantile, median and top_k(1), which their docstrings leave
    undefined on rows of no points -- so the GPU test's own assertion cannot be met by refusals or by skipping"""
    import test_gpu_module_sequences as seqs
    built = {}

    def model_state(kind, name, cplx, order):
        key = (kind, name, cplx, order)
        if key not in built:
            built[key] = seqs.build_state(kind, seqs._model_api(kind), name, cplx, order, np.float32, TIME, (-1, 1), 1)
        return built[key]

    for e in seqs.MODULE_CATALOGUE:
        for kind in e.kinds:
            classes = {seqs._class_of(kind, name) for name, cplx, order in seqs.states_of(e, kind)
                       if e.defined(model_state(kind, name, cplx, order))}
            need = set(e.need) - ({"exact"} if e.space == "complex" else set())
            assert need <= classes, (e.label, kind, sorted(need - classes))
            assert {"shrunk", "moved", "exact"} <= set(e.need), e.label
            if "empty" not in e.need:
                assert e.fn in ("quantile", "median") or e.label.startswith("top_k(1,"), e.label
                empties = [model_state(kind, n, c, o) for n, c, o in seqs.states_of(e, kind) if seqs._class_of(kind, n) == "empty"]
                assert empties and not any(e.defined(w) for w in empties)
    # the linalg entries are defined on the square states only, the 0 x 0 of D7 among them (the documented N == 0)
    lin = [e for e in seqs.MODULE_CATALOGUE if e.fn in ("cholesky", "cholesky_solve", "eigh")]
    assert len(lin) == 7
    for e in lin:
        on = {(n, o) for n, c, o in seqs.states_of(e, "mat") if e.defined(model_state("mat", n, c, o))}
        assert {n for n, o in on if o is None} == {"D7-no-rows", "D7-empty-rows-transposed", "D7-no-rows-transposed"}, e.label
        assert {n for n, o in on if o is not None} == set(M.HERMITIAN) | {M.EXACT_FIT_HERMITIAN}, e.label
    # zoom_fft(2200 bins) on D4-regrown: a convolution length of 8192 (the five-step route) and a reallocation inside the call
    fill = lambda rows, scalars: np.zeros((rows, scalars), np.float32)
    d4 = mm.build_dirty(mm.ModelApi, "D4-regrown", fill, np.float32, False, TIME, 1.0)
    assert (d4.rows(), d4.row_points()) == (3, 2000) and tzoom.conv_len(2000, 2200) == 8192 and 3 * 2200 * 2 > d4.cap
    d1 = mm.build_dirty(mm.ModelApi, "D1-shrunk", fill, np.float32, False, TIME, 1.0)
    assert d1.row_points() == 1024 and tzoom.conv_len(d1.row_points(), 2200) == 4096   # and the fused route on D1
    # the selector crossover: the entry's window is the first odd one above it
    for dtype in (np.float32, np.float64):
        half = seqs._above_cross(dtype)[0]
        assert 2 * half + 1 > trank.CROSS[dtype] >= 2 * half - 1 and half <= trank.MAX_HALF


POISON_CODE = re.compile(r"-1 for a poisoned")


def _doc(fns, name, depth=0):
    """the function's docstring plus those it refers to ("codes are quantile's", "every other code is detect's", "then
    sort's")"""
    doc = inspect.getdoc(fns[name]) or ""
    if depth < 3:
        for other in re.findall(r"\b(\w+)'s\b", doc):
            if other in fns and other != name:
                doc += " " + _doc(fns, other, depth + 1)
    return doc


def test_every_documented_code_has_a_row():
    """the tables of test_gpu_module_sequences.py against the docstrings: a function whose docstring (or the one it refers
    to) names an argument-error code (7, 4, 5, 2, 1) has a row with that code in MODULE_ARG_ERRORS; one that names -1 for
    a poisoned operand has a row in MODULE_POISONED"""
    import test_gpu_module_sequences as seqs
    fns = _module_functions()
    docs = {n: " ".join(_doc(fns, n).split()) for n in fns}
    documented = {}
    for n, d in docs.items():
        codes = set()
        for code in (7, 4, 5, 2, 1):
            if re.search(r"(?<![\w.\-/])%d(?= for |, with the data| unless | when )" % code, d):
                codes.add(code)
        documented[n] = codes
    # the pattern finds what it is meant to find
    assert documented["sort"] == {7, 4} and documented["sosfilt"] == {5, 2, 7} and documented["zoom_fft"] == {7, 5}
    assert documented["matmul"] == {2, 7} and documented["cholesky"] >= {7} and documented["eigh"] >= {7}
    assert documented["detect"] >= {7, 2, 4} and documented["median"] >= {7, 4} and documented["argrelmax"] >= {7, 4}
    assert all(documented[n] for n in fns), "every module function documents a code"
    rows = {}
    for fn, label, kinds, space, domain, bad, code in seqs.MODULE_ARG_ERRORS:
        assert fn in fns, fn
        rows.setdefault(fn, set()).add(code)
    for n in fns:
        want = {c for c in documented[n] if (n, c) not in seqs.MODULE_ARG_ERRORS_EXEMPT}
        assert want <= rows.get(n, set()), "%s documents %s, MODULE_ARG_ERRORS has %s" % (n, sorted(want), sorted(rows.get(n, ())))
    assert all(fn in fns and code in documented[fn] for fn, code in seqs.MODULE_ARG_ERRORS_EXEMPT), "an exemption nothing needs"
    # detect's operand codes are add's: 7 for another row count, 1, 2
    assert {7, 2, 4, 1} <= rows["detect"]
    # calls that break two rules: the code the docstring puts first
    assert sum("comes first" in label for _, label, *_ in seqs.MODULE_ARG_ERRORS) >= 7
    poisonable = {n for n, d in docs.items() if POISON_CODE.search(d)}
    assert poisonable == set(fns), sorted(set(fns) - poisonable)
    have = {row[0] for row in seqs.MODULE_POISONED}
    assert poisonable <= have, "documents -1 for a poisoned operand, has no row in MODULE_POISONED: %s" % sorted(poisonable - have)
    # every operand that can be poisoned: sosfilt's state, detect's threshold, both operands of matmul and cholesky_solve
    for fn, count in (("sosfilt", 2), ("detect", 2), ("matmul", 2), ("cholesky_solve", 2)):
        assert sum(row[0] == fn and "comes first" not in row[1] for row in seqs.MODULE_POISONED) >= count, fn
    # the states the rows run on
    assert {n[:2] for n, _ in seqs.MAT_ERR_STATES} == {"D1", "D2", "D3", "D4", "L1", "L2"}
    assert seqs.VEC_ERR_STATES == __import__("test_gpu_vec_sequences").ERR_STATES
