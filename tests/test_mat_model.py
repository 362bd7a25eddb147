"""tests/mat_model.py on the CPU: every mover of the model against the CPU oracle row by row (two independent statements
of each operation: numpy index arithmetic there, the oracle's loops here), the model's own invariants, what the
generated sequences of tests/test_gpu_mat_sequences.py cover, and that every public DspMat method is either a mover or
has an entry in that file's catalogue."""
import inspect
import re

import numpy as np
import pytest

import mat_model as mm
import oracle_lib as orc
from mat_model import FREQ, PAD_CENTER, PAD_END, PAD_SURROUND, TIME, MatModel, VecModel

DTYPES = (np.float32, np.float64)
# (rows, points): odd and even lengths, one point, rows without points
SHAPES = ((3, 1), (2, 2), (3, 5), (4, 8), (5, 17), (2, 64), (3, 101), (4, 0))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(_bits(got), _bits(ref))


def _fill(rows, pts, cplx, dtype, seed=1):
    e = 2 if cplx else 1
    x = orc.fill_uniform(rows * pts * e, seed + 31 * rows + pts, -10, 10, dtype).reshape(rows, pts * e)
    if x.size >= 4:   # the values a copy must carry unchanged and a sign flip must flip
        f = x.reshape(-1)
        f[0], f[1], f[-1] = -0.0, 0.0, np.inf
        f[x.size // 2] = np.nan
    return x


def _rows(fn, x):
    out = [fn(r) for r in x]
    return np.stack(out) if out else np.zeros((0, 0), x.dtype)


CASES = [(r, p, c, d) for (r, p) in SHAPES for c in (False, True) for d in DTYPES]
IDS = ["%dx%d-%s-%s" % (r, p, "complex" if c else "real", np.dtype(d).name) for (r, p, c, d) in CASES]


@pytest.mark.parametrize("rows,pts,cplx,dtype", CASES, ids=IDS)
def test_in_place_movers_equal_the_oracle_row_by_row(rows, pts, cplx, dtype):
    x = _fill(rows, pts, cplx, dtype)
    e = 2 if cplx else 1
    new = lambda: MatModel(x, cplx, FREQ, 0.25)

    def meta(m, row_len, c=cplx):
        assert (m.rows(), m.row_len(), m.row_points(), m.is_complex()) == (rows, row_len, row_len // (2 if c else 1), c)
        assert m.domain() == FREQ and m.delta() == 0.25 and not m.poisoned

    for name, fwd in (("swap_halves", True), ("fft_shift", True), ("ifft_shift", False)):
        m = new()
        assert getattr(m, name)() == 0
        meta(m, pts * e)
        _same(m.data(), _rows(lambda r: orc.swap_halves(r, cplx, fwd), x))
    m = new()
    assert m.reverse() == 0
    meta(m, pts * e)
    _same(m.data(), _rows(lambda r: orc.reverse(r, cplx), x))
    for new_pts in (pts + 1, pts + 2, 2 * pts + 3):
        for opt in (PAD_END, PAD_SURROUND, PAD_CENTER):
            m = new()
            assert m.zero_pad(new_pts, opt) == 0
            meta(m, new_pts * e)
            _same(m.data(), _rows(lambda r: orc.zero_pad(r, cplx, new_pts, opt, buffered=(opt == PAD_SURROUND))[1], x))
    for opt in (PAD_END, PAD_SURROUND, PAD_CENTER):
        m = new()
        assert m.zero_pad(pts, opt) == 7 and (pts == 0 or m.zero_pad(pts - 1, opt) == 7)
        _same(m.data(), x)
    for factor in (0, 1, 2, 3, 5):
        m = new()
        assert m.zero_interleave(factor) == 0
        f = max(factor, 1)
        meta(m, pts * f * e)
        _same(m.data(), _rows(lambda r: orc.zero_interleave(r, cplx, f), x).reshape(rows, pts * f * e))
    for factor, delay in ((1, 0), (2, 0), (2, 1), (3, 2), (4, 1), (5, 7), (3, pts), (2, max(pts - 1, 0))):
        m = new()
        assert m.decimatei(factor, delay) == 0
        ref = _rows(lambda r: orc.decimatei(r, cplx, factor, delay), x)
        meta(m, ref.shape[1])
        _same(m.data(), ref.reshape(rows, -1))
    m = new()
    assert m.decimatei(0, 0) == 7
    _same(m.data(), x)
    if cplx:
        m = new()
        assert m.conj() == 0
        meta(m, pts * e)
        _same(m.data(), _rows(orc.conj, x).reshape(rows, pts * e))
        for name, kind in (("to_real", 2), ("to_imag", 3)):
            m = new()
            assert getattr(m, name)() == 0
            meta(m, pts, False)
            _same(m.data(), _rows(lambda r: orc.complex_to_real(r, kind), x).reshape(rows, pts))
        m = new()
        assert m.mirror() == 0
        n = max(2 * pts - 1, 0)
        meta(m, 2 * n)
        if pts:
            _same(m.data(), _rows(orc.mirror, x))
        assert new().to_complex() == -1
    else:
        m = new()
        assert m.to_complex() == 0
        meta(m, 2 * pts, True)
        _same(m.data(), _rows(lambda r: orc.zero_interleave(r, False, 2), x).reshape(rows, 2 * pts))
        for name in ("conj", "to_real", "to_imag"):
            m = new()
            assert getattr(m, name)() == -1 and m.poisoned and m.rows() == rows and m.row_len() == 0 and np.isnan(m.delta())
        m = MatModel(x, False, TIME)
        assert m.mirror() == -1 and m.poisoned


@pytest.mark.parametrize("rows,pts,cplx,dtype", CASES, ids=IDS)
def test_transpose_and_the_interleaved_pair_equal_split_into_and_merge(rows, pts, cplx, dtype):
    x = _fill(rows, pts, cplx, dtype)
    e = 2 if cplx else 1
    m = MatModel(x, cplx, FREQ, 0.25)
    code, v = m.to_interleaved()
    assert code == 0 and (v.points(), v.is_complex(), v.domain(), v.delta()) == (rows * pts, cplx, FREQ, 0.25)
    if pts:
        _same(v.data(), orc.merge(list(x), cplx))                       # to_interleaved is merge of the rows
        code, targets = orc.split_into(v.data(), cplx, rows)            # from_interleaved is split_into
        assert code == 0
        code, back = MatModel.from_interleaved(v, rows)
        assert code == 0 and back.rows() == rows and back.row_points() == pts
        _same(back.data(), np.stack(targets))
        _same(back.data(), x)
    assert m.transpose() == 0
    if pts == 0:
        assert (m.rows(), m.row_len()) == (0, 0) and m.transpose() == 0 and m.rows() == 0   # the rows do not come back
        return
    assert (m.rows(), m.row_points(), m.row_len(), m.is_complex(), m.delta()) == (pts, rows, rows * e, cplx, 0.25)
    _same(m.data().reshape(-1), v.data())                               # the transposed matrix, flat, IS the interleaved vector
    for j in range(pts):                                                # row j of the transpose = point j of every row
        _same(m.data()[j], x[:, j * e:(j + 1) * e].reshape(-1))
    assert m.transpose() == 0
    _same(m.data(), x)
    assert MatModel.from_interleaved(VecModel(np.zeros(7 * e, dtype), cplx), 2) == (7, None)
    assert MatModel.from_interleaved(VecModel(np.zeros(6 * e, dtype), cplx), 0) == (7, None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_part_getters_and_setter_between_matrices(dtype):
    x = _fill(3, 5, True, dtype)
    m = MatModel(x, True, FREQ, 0.25)
    re, im = MatModel(np.ones((1, 1), dtype), False, TIME, 0.5), MatModel(np.ones((2, 3), dtype), False, TIME, 0.125)
    assert m.get_real_imag(re, im) == 0
    _same(re.data(), np.stack([orc.complex_to_real(r, 2) for r in x]))
    _same(im.data(), np.stack([orc.complex_to_real(r, 3) for r in x]))
    assert (re.delta(), re.domain(), im.delta(), re.rows(), im.row_len()) == (0.5, TIME, 0.125, 3, 5)   # destinations keep theirs
    for name, kind in (("get_real", 2), ("get_imag", 3)):
        d = MatModel(np.ones((1, 1), dtype), False, TIME, 0.5)
        assert getattr(m, name)(d) == 0
        _same(d.data(), np.stack([orc.complex_to_real(r, kind) for r in x]))
        c = MatModel(np.ones((1, 2), dtype), True)
        assert getattr(m, name)(c) == 0 and (c.rows(), c.row_len()) == (3, 0)   # a complex destination: empty rows
        assert getattr(re, name)(d) == 0 and (d.rows(), d.row_len()) == (3, 0)  # a real source: empty rows
    t = MatModel(np.ones((1, 2), dtype), True, TIME, 2.0)
    assert t.set_real_imag(re, im) == 0
    assert (t.rows(), t.row_points(), t.is_complex(), t.domain(), t.delta()) == (3, 5, True, TIME, 2.0)
    _same(t.data(), x)
    assert t.set_real_imag(re, MatModel(np.ones((3, 4), dtype))) == 7
    _same(t.data(), x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cplx", (False, True))
def test_rows_frames_and_vectors(dtype, cplx):
    e = 2 if cplx else 1
    x = _fill(4, 6, cplx, dtype)
    m = MatModel(x, cplx, FREQ, 0.25)
    v = m.get_row(2)
    _same(v.data(), x[2])
    assert (v.is_complex(), v.domain(), v.delta(), v.points()) == (cplx, FREQ, 0.25, 6)
    with pytest.raises(IndexError):
        m.get_row(4)
    assert m.set_row(0, v) == 0 and m.set_row(4, v) == 7 and m.set_row(0, VecModel(x[0][:-e], cplx)) == 7
    want = x.copy()
    want[0] = x[2]
    _same(m.data(), want)
    code, back = MatModel.from_vectors([MatModel(x, cplx, FREQ, 0.25).get_row(r) for r in range(4)])
    assert code == 0 and (back.is_complex(), back.domain(), back.delta()) == (cplx, FREQ, 0.25)
    _same(back.data(), x)
    assert MatModel.from_vectors([VecModel(x[0], cplx), VecModel(x[0][:-e], cplx)]) == (7, None)
    assert MatModel.from_vectors([VecModel(x[0], cplx), VecModel(x[0], cplx, FREQ)]) == (2, None)
    # overlap_add against the row loop of its docstring; hop = frame flattens, up to -0.0 + 0 = +0.0
    m = MatModel(x, cplx, TIME, 0.5)
    for hop in (1, 4, 6, 9):
        code, y = m.overlap_add(hop)
        ref = np.zeros((3 * hop + 6) * e, dtype)
        for r in range(4):
            ref[r * hop * e:(r * hop + 6) * e] += x[r]
        assert code == 0
        _same(y.data(), ref)
    code, y = m.overlap_add(6)
    _same(y.data(), np.zeros(24 * e, dtype) + x.reshape(-1))
    assert np.signbit(x.reshape(-1)[0]) and not np.signbit(y.data()[0])
    assert m.overlap_add(0) == (7, None)
    # from_frames: x[r * hop + j], zero past the end, the row counts of the docstring
    sig = VecModel(orc.fill_uniform(23 * e, 5, -1, 1, dtype), cplx, TIME, 0.5)
    for frame, hop, tail, rows in ((6, 6, False, 3), (6, 6, True, 4), (8, 3, False, 6), (8, 3, True, 6), (8, 4, True, 5),
                                   (30, 2, False, 0), (30, 2, True, 1), (23, 5, True, 1), (23, 5, False, 1)):
        code, f = MatModel.from_frames(sig, frame, hop, tail)
        assert code == 0 and f.rows() == rows and f.row_points() == (frame if rows else 0), (frame, hop, tail)
        s = np.concatenate([sig.data(), np.zeros(40 * e, dtype)])
        for r in range(rows):
            _same(f.data()[r], s[r * hop * e:(r * hop + frame) * e])
    assert MatModel.from_frames(sig, 0, 1) == (7, None) and MatModel.from_frames(sig, 1, 0) == (7, None)
    code, f = MatModel.from_frames(VecModel(x.reshape(-1), cplx), 6, 6)
    _same(f.data(), x)


def test_poisoned_model_answers_minus_one_and_keeps_its_rows():
    m = MatModel(np.ones((3, 4), np.float32), False)
    assert m.conj() == -1
    for call in (m.transpose, m.swap_halves, m.reverse, lambda: m.zero_interleave(2), lambda: m.decimatei(2, 0),
                 lambda: m.zero_pad(8), m.to_complex):
        assert call() == -1 and m.poisoned and m.rows() == 3 and m.row_len() == 0 and np.isnan(m.delta())
    assert m.zero_pad(0) == 7   # an argument error comes first


def test_dirty_recipes_reach_the_states_they_name():
    fill = lambda rows, scalars: np.arange(rows * scalars, dtype=np.float32).reshape(rows, scalars)
    build = lambda name, cplx: mm.build_dirty(mm.ModelApi, name, fill, np.float32, cplx, TIME, 1.0, vec=lambda a: VecModel(a, True))
    d1 = build("D1-shrunk", False)
    assert (d1.rows(), d1.row_len()) == (5, 1024) and d1.cap > 4 * d1.a.size and d1.reallocs == 0
    d2 = build("D2-transposed", True)
    assert (d2.rows(), d2.row_points()) == (5, 1001)
    d3 = build("D3-exact-fit", False)
    assert (d3.rows(), d3.row_len()) == (3, 1315) and d3.cap == d3.a.size == 3945 and d3.reallocs == 1
    assert mm.grown_cap(3000) == 3439 and 3439 % 3 and mm.grown_cap(3450) == 3945
    d4 = build("D4-regrown", False)
    assert d4.reallocs == 1 and d4.row_len() == 2000
    d5 = build("D5-space-twice", False)
    assert not d5.is_complex() and d5.reallocs == 1
    _same(d5.data(), fill(5, 1001))
    d6 = build("D6-from-frames", True)
    assert d6.is_complex() and d6.row_points() == mm.D6_FRAME and d6.rows() == -(-(mm.D6_POINTS - mm.D6_FRAME) // mm.D6_HOP) + 1
    for name, shape in (("D7-empty-rows", (5, 0)), ("D7-no-rows", (0, 0)), ("D7-empty-rows-transposed", (0, 0)),
                        ("D7-no-rows-transposed", (0, 0))):
        d = build(name, False)
        assert (d.rows(), d.row_len()) == shape and not d.poisoned


# ---------------------------------------------------------------------------------------------- the generator
@pytest.fixture(scope="module")
def logs():
    return {key: mm.gen_sequence(*key) for key in mm.all_sequences()}


def test_the_generator_is_deterministic_and_stays_in_bounds(logs):
    assert len(mm.SEEDS) == 24 and len(logs) == 6 * 2 * 24
    for key in list(logs)[::17]:
        assert mm.gen_sequence(*key)[0] == logs[key][0]
    for seq, log in logs.values():
        assert len(seq) == mm.STEPS == 16 and all(step[0] in mm.STEP_MOVERS for step in seq)
    assert {mv for movers in mm.STEP_MOVERS.values() for mv in movers} == set(mm.MOVERS)


def test_the_seed_list_covers_every_mover_in_every_history(logs):
    """the conditions the GPU test's worth rests on, from the generator alone; more seeds if one fails, never a weaker
    condition"""
    cov = mm.coverage([log for _, log in logs.values()])
    assert set(cov) == set(mm.MOVERS)
    for mover, c in cov.items():
        assert c["count"] >= 3, (mover, c)
        assert c["after_transpose"] >= 1, (mover, "never after a transpose")
        assert c["after_realloc"] >= 1, (mover, "never after a grow that reallocates")
        assert c["after_shrink"] >= 1, (mover, "never after a shrink")
        assert c["after_space_change"] >= 1, (mover, "never after a change of number space")
    for key, (seq, log) in logs.items():
        assert any(ev["transpose"] for ev in log), (key, "no transpose")
        assert any(ev["row_len_change"] for ev in log), (key, "row_len never changes")


# ---------------------------------------------------------------------------------------------- the catalogue
# (these three import basic_dsp_amd for DspMat's docstrings, which loads the built library as the *_abi tests do: they
# need build() to have run, not a GPU)
def _public():
    from basic_dsp_amd.matrix import DspMat
    return DspMat, {n for n, f in inspect.getmembers(DspMat, callable) if not n.startswith("_")}


def test_every_public_method_is_a_mover_or_catalogued():
    """a DspMat method added later without an entry in test_gpu_mat_sequences.CATALOGUE fails here, on the CPU"""
    import test_gpu_mat_sequences as seqs
    _, public = _public()
    catalogued = {entry.method for entry in seqs.CATALOGUE}
    assert set(mm.MOVERS) <= public and catalogued <= public and set(seqs.ACCESSORS) <= public
    assert not set(mm.MOVERS) & catalogued
    missing = public - set(mm.MOVERS) - catalogued - set(seqs.ACCESSORS)
    assert not missing, "neither a mover nor catalogued: %s" % sorted(missing)


def _doc(cls, public, name, depth=0):
    """the method's docstring plus those it refers to ("As plain_sfft ...", "Codes: as add_smaller ...")"""
    doc = inspect.getdoc(getattr(cls, name)) or ""
    if depth < 4:
        for other in re.findall(r"\b[Aa]s (\w+)", doc):
            if other in public and other != name:
                doc += " " + _doc(cls, public, other, depth + 1)
    return doc


ARG_CODE = re.compile(r"(?<![\w.])7(?![\w.])|4 / 3 / 2")                      # InvalidArgumentLength, or dot_product's codes
POISONS = re.compile(r"\(poisoned\)|is poisoned \(-1\)|; poisoned\)|self is poisoned\)|matrix is\s+poisoned\)")


def test_every_documented_argument_error_and_poisoning_has_an_entry():
    """the tables of test_gpu_mat_sequences.py against DspMat's docstrings: a method whose docstring (or the one it
    refers to) names an argument-error code must be in ARG_ERRORS or, with a reason, in ARG_ERRORS_EXEMPT; one whose
    docstring says it poisons the matrix must be in POISONERS"""
    import test_gpu_mat_sequences as seqs
    cls, public = _public()
    docs = {n: _doc(cls, public, n) for n in public}
    with_codes = {n for n, d in docs.items() if ARG_CODE.search(d)}
    poisoning = {n for n, d in docs.items() if POISONS.search(d)}
    # the patterns find what they are meant to find
    assert {"add_smaller", "div_smaller", "set_real_imag", "set_mag_phase", "correlate", "interpolate", "decimatei",
            "dot_product", "overlap_add", "from_frames"} <= with_codes
    assert {"wrap", "unwrap", "abs", "cos_approx", "log_approx", "powf_approx", "multiply_complex_exponential", "plain_sfft",
            "sfft", "windowed_sfft", "plain_sifft", "sifft", "windowed_sifft", "mirror", "to_complex", "correlate", "convolve",
            "convolve_complex", "interpolate_lin", "interpolate_hermite"} <= poisoning
    assert not {"sqrt", "reverse", "transpose", "get_real", "zero_interleave"} & poisoning
    tried = {row[0] for row in seqs.ARG_ERRORS}
    assert tried <= public and set(seqs.ARG_ERRORS_EXEMPT) <= public
    missing = with_codes - tried - set(seqs.ARG_ERRORS_EXEMPT)
    assert not missing, "documents an argument-error code, has no entry in ARG_ERRORS: %s" % sorted(missing)
    assert "dot_product" in tried and {4, 3, 2, 7} <= {c for row in seqs.ARG_ERRORS if row[0] == "dot_product"
                                                    for c in ([row[4](True), row[4](False)] if callable(row[4]) else [row[4]])}
    poisoners = {row[0] for row in seqs.POISONERS}
    assert poisoners <= public
    missing = poisoning - poisoners
    assert not missing, "documents poisoning, has no entry in POISONERS: %s" % sorted(missing)
    for name in ("plain_sfft", "sfft", "windowed_sfft"):   # both documented codes, 5 and 9
        assert {5, 9} <= {row[5] for row in seqs.POISONERS if row[0] == name}, name
    for name in ("plain_sifft", "sifft", "windowed_sifft"):   # 6 and 8
        assert {6, 8} <= {row[5] for row in seqs.POISONERS if row[0] == name}, name
