"""tests/vec_model.py on the CPU: every mover of the model against the CPU oracle bit for bit (two independent statements
of each operation: one gather of numpy indices there, the oracle's loops here), the model's bookkeeping (capacity, trades,
unspecified scalars, poisoning), what the generated sequences of tests/test_gpu_vec_sequences.py cover, that the dirty
recipes reach the states they name, and that every public DspVec method is a mover, an accessor or has an entry in that
file's catalogue."""
import inspect
import re

import numpy as np
import pytest

import oracle_lib as orc
import vec_model as vm
from vec_model import FREQ, PAD_CENTER, PAD_END, PAD_SURROUND, TIME, VecModel

DTYPES = (np.float32, np.float64)
POINTS = (1, 2, 5, 8, 17, 64, 101)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(_bits(got), _bits(ref))


def _fill(pts, cplx, dtype, seed=1):
    """noise with -0.0, +0.0, inf and a NaN planted: the values a copy must carry unchanged and a sign flip must flip"""
    e = 2 if cplx else 1
    x = orc.fill_uniform(pts * e, seed + pts, -10, 10, dtype)
    for k, v in enumerate((-0.0, 0.0, np.inf, np.nan)):
        if k < x.size:
            x[(k * 7) % x.size if x.size >= 8 else k] = v
    return x


CASES = [(p, c, d) for p in POINTS for c in (False, True) for d in DTYPES]
IDS = ["%d-%s-%s" % (p, "complex" if c else "real", np.dtype(d).name) for (p, c, d) in CASES]


@pytest.mark.parametrize("pts,cplx,dtype", CASES, ids=IDS)
def test_in_place_movers_equal_the_oracle(pts, cplx, dtype):
    x = _fill(pts, cplx, dtype)
    e = 2 if cplx else 1
    new = lambda: VecModel(x, cplx, FREQ, 0.25)

    def meta(v, n, c=cplx, trades=1):
        assert (v.len(), len(v), v.points(), v.is_complex()) == (n, n, n // (2 if c else 1), c)
        assert v.domain() == FREQ and v.delta() == 0.25 and not v.is_erroneous() and v.trades == trades and not v.unspec.any()

    for name, fwd in (("swap_halves", True), ("fft_shift", True), ("ifft_shift", False)):
        v = new()
        assert getattr(v, name)() == 0
        meta(v, pts * e)
        _same(v.data(), orc.swap_halves(x, cplx, fwd))
    v = new()
    assert v.reverse() == 0
    meta(v, pts * e)
    _same(v.data(), orc.reverse(x, cplx))
    for new_pts in (pts + 1, pts + 2, 2 * pts + 3):
        for opt in (PAD_END, PAD_SURROUND, PAD_CENTER):
            v = new()
            assert v.zero_pad(new_pts, opt) == 0
            meta(v, new_pts * e)
            _same(v.data(), orc.zero_pad(x, cplx, new_pts, opt, buffered=(opt == PAD_SURROUND))[1])
    for opt in (PAD_END, PAD_SURROUND, PAD_CENTER):
        v = new()
        assert v.zero_pad(pts, opt) == 7 and v.zero_pad(pts - 1, opt) == 7 and v.trades == 0
        _same(v.data(), x)
    for factor in (0, 1, 2, 3, 5):
        v = new()
        assert v.zero_interleave(factor) == 0
        f = max(factor, 1)
        meta(v, pts * f * e, trades=int(factor > 1))
        _same(v.data(), orc.zero_interleave(x, cplx, f))
    for factor, delay in ((1, 0), (2, 0), (2, 1), (3, 2), (4, 1), (5, 7), (3, pts), (2, pts - 1)):
        v = new()
        assert v.decimatei(factor, delay) == 0
        ref = orc.decimatei(x, cplx, factor, delay)
        meta(v, ref.size, trades=int(ref.size > 0))
        _same(v.data(), ref)
    v = new()
    assert v.decimatei(0, 0) == 7 and v.trades == 0
    _same(v.data(), x)
    if cplx:
        v = new()
        assert v.conj() == 0
        meta(v, pts * e, trades=0)   # in place
        _same(v.data(), orc.conj(x))
        for name, kind in (("to_real", 2), ("to_imag", 3)):
            v = new()
            assert getattr(v, name)() == 0
            meta(v, pts, False)
            _same(v.data(), orc.complex_to_real(x, kind))
        v = new()
        assert v.mirror() == 0
        meta(v, 2 * (2 * pts - 1))
        _same(v.data(), orc.mirror(x))
        v = new()
        assert v.to_complex() == -1 and v.is_erroneous() and v.is_complex()
    else:
        v = new()
        assert v.to_complex() == 0
        meta(v, 2 * pts, True)
        _same(v.data(), orc.zero_interleave(x, False, 2))
        for name in ("conj", "to_real", "to_imag"):
            v = new()
            assert getattr(v, name)() == -1 and v.is_erroneous() and v.len() == 0 and np.isnan(v.delta()) and not v.is_complex()
        v = VecModel(x, False, TIME)
        assert v.mirror() == -1 and v.is_erroneous()


@pytest.mark.parametrize("pts,cplx,dtype", CASES, ids=IDS)
def test_movers_between_vectors_equal_the_oracle(pts, cplx, dtype):
    x = _fill(pts, cplx, dtype)
    e = 2 if cplx else 1
    v = VecModel(x, cplx, FREQ, 0.25)
    small = lambda n, c=False: VecModel(np.ones(n, dtype), c, TIME, 0.5)
    # clone: equal values and metadata, capacity from the valid length, no history
    v.trades, v.cap = 3, 4 * v.cap
    c = v.clone()
    _same(c.data(), x)
    assert (c.is_complex(), c.domain(), c.delta(), c.cap, c.trades, c.reallocs) == (cplx, FREQ, 0.25, vm.grown_cap(x.size), 0, 0)
    # split_into / merge: point i <-> target i % n, position i / n
    for n in (1, 2, 3, 5):
        targets = [small(4 if cplx else 5, cplx) for _ in range(n)]
        code = v.split_into(targets)
        ocode, ref = orc.split_into(x, cplx, n)
        if pts % n:
            assert code == (13 if cplx and (x.size % n == 0) else 7) and all(t.len() == (4 if cplx else 5) for t in targets)
            continue
        assert code == 9 and ocode == 0
        for t, r in zip(targets, ref):
            _same(t.data(), r)
            assert (t.domain(), t.delta(), t.is_complex(), t.trades) == (TIME, 0.5, cplx, 0)   # a target keeps its own
        back = small(2, cplx)
        assert back.merge(targets) == 0
        _same(back.data(), x)
        _same(back.data(), orc.merge([t.data() for t in targets], cplx))
        assert back.cap == max(vm.grown_cap(2), vm.grown_cap(x.size) if x.size > vm.grown_cap(2) else 0) and back.trades == 0
    assert v.split_into([]) == 7 and small(2, cplx).merge([]) == 7
    assert small(2, cplx).merge([small(4, cplx), small(6, cplx)]) == 7
    if not cplx:
        im = VecModel(x[::-1], False, TIME, 2.0)
        t = small(2, True)
        assert t.set_real_imag(v, im) == 0 and (t.points(), t.is_complex(), t.domain(), t.delta()) == (pts, True, TIME, 0.5)
        _same(t.data()[0::2], x)
        _same(t.data()[1::2], x[::-1])
        assert t.set_real_imag(v, small(pts + 1)) == 7
        _same(t.data()[0::2], x)
        for name in ("get_real", "get_imag"):   # a real source empties the destination; the code is 9 whatever happened
            d = small(5)
            assert getattr(v, name)(d) == 9 and d.len() == 0 and not d.is_erroneous()
        return
    re, im = small(5), small(3)
    assert v.get_real_imag(re, im) == 9
    _same(re.data(), orc.complex_to_real(x, 2))
    _same(im.data(), orc.complex_to_real(x, 3))
    assert (re.delta(), re.domain(), re.is_complex(), im.len()) == (0.5, TIME, False, pts)   # destinations keep theirs
    assert re.cap == max(vm.grown_cap(5), vm.grown_cap(pts) if pts > vm.grown_cap(5) else 0)
    for name, kind in (("get_real", 2), ("get_imag", 3)):
        d = small(5)
        assert getattr(v, name)(d) == 9
        _same(d.data(), orc.complex_to_real(x, kind))
        c = small(2, True)
        assert getattr(v, name)(c) == 9 and c.len() == 0   # a complex destination is emptied
    c = small(2, True)
    assert v.get_real_imag(re, c) == 9 and re.len() == 0 and c.len() == 0


def test_capacity_follows_the_library_rule():
    v = VecModel(np.zeros(3000, np.float32))
    assert v.cap == 3439 == 3000 + 3000 // 8 + 64 and vm.grown_cap(1) == 65
    assert v.zero_pad(3439) == 0 and v.cap == 3439 and v.reallocs == 0 and v.len() == v.cap   # fills it exactly
    assert v.zero_pad(3440) == 0 and v.cap == vm.grown_cap(3440) and v.reallocs == 1
    assert v.decimatei(10, 0) == 0 and v.cap == vm.grown_cap(3440)                            # never shrinks
    assert v.clone().cap == vm.grown_cap(344)                                                 # a clone starts over
    assert VecModel(np.zeros(0, np.float64)).cap == 65
    c = VecModel(np.zeros(3008, np.float64), True)
    assert c.cap == 3448 and c.zero_pad(1724) == 0 and c.len() == c.cap and c.reallocs == 0


def test_set_len_marks_exactly_the_grown_tail_and_the_mark_moves_with_the_scalar():
    x = np.arange(1, 11, dtype=np.float32)
    v = VecModel(x)
    v.set_len(6)
    assert v.len() == 6 and not v.unspec.any()
    v.set_len(9)   # within the allocation: the tail is whatever the buffer held
    assert v.len() == 9 and v.unspec.tolist() == [False] * 6 + [True] * 3 and v.reallocs == 0
    _same(v.data()[:6], x[:6])
    assert v.reverse() == 0 and v.unspec.tolist() == [True] * 3 + [False] * 6
    assert v.zero_pad(12, PAD_SURROUND) == 0 and v.unspec.tolist() == [False, False] + [True] * 3 + [False] * 7   # left = 3 - 1
    assert v.to_complex() == 0 and v.unspec.tolist() == [False] * 4 + [True, False] * 3 + [False] * 14
    assert v.conj() == 0 and v.unspec.sum() == 3
    v.set_len(23)   # odd length of a complex vector: ignored
    assert v.len() == 24
    d = VecModel(np.ones(5, np.float32))
    assert v.get_real(d) == 9 and d.unspec.tolist() == [False, False] + [True] * 3 + [False] * 7
    v.set_len(0)
    assert v.len() == 0 and not v.is_erroneous()
    big = VecModel(x)
    big.set_len(100)   # past the allocation: one reallocation, the old scalars are copied
    assert big.cap == vm.grown_cap(100) and big.reallocs == 1 and big.unspec.sum() == 90
    _same(big.data()[:10], x)


def test_poisoned_model_answers_as_the_facade_does():
    v = VecModel(np.ones(6, np.float32), False, TIME, 0.5)
    assert v.conj() == -1 and v.is_erroneous()
    for call in (v.swap_halves, v.reverse, lambda: v.zero_interleave(3), lambda: v.decimatei(2, 0), v.conj, v.to_real):
        assert call() == -1 and v.is_erroneous() and v.len() == 0 and np.isnan(v.delta())
    assert v.zero_pad(0) == 7 and v.decimatei(0, 0) == 7   # an argument error comes first
    assert v.to_complex() == -1 and v.is_complex() and v.to_complex() == -1


def test_dirty_recipes_reach_the_states_they_name():
    fill = lambda n, k: np.arange(n, dtype=np.float32) + 1000 * k
    build = lambda name, cplx: vm.build_dirty(vm.ModelApi, name, fill, cplx, TIME, 0.5)
    for cplx in (False, True):
        e = 2 if cplx else 1
        d = build("shrunk-even", cplx)
        assert d.points() == 1024 and d.cap > 4 * d.len() and d.reallocs == 0 and d.trades == 1
        d = build("shrunk-odd", cplx)
        assert d.points() == 1023 and d.trades == 2
        d = build("shrunk-by-set_len", cplx)
        assert d.len() == 2000 and d.len() % 2 == 0 and d.trades == 0 and d.cap == vm.grown_cap(2001 * e) and not d.unspec.any()
        d = build("odd-trades", cplx)
        assert d.trades == 1 and d.reallocs == 0 and d.points() == 1000
        assert build("odd-trades-odd", cplx).points() == 1001
        d = build("regrown", cplx)
        assert d.reallocs == 1 and d.points() == 2000 and d.trades == 2
        d = build("regrown-odd", cplx)
        assert d.reallocs == 1 and d.points() == 2001
        d = build("split_into-target", cplx)
        assert d.points() == 1001 and d.reallocs == 1 and d.cap == vm.grown_cap(1001 * e) and d.trades == 0
        d = build("clone-of-dirty", cplx)
        assert d.points() == 2001 and d.cap == vm.grown_cap(2001 * e) and d.reallocs == 0 and d.trades == 0
        d = build("emptied-and-refilled", cplx)
        assert d.points() == 1000 and d.reallocs == 0 and d.trades == 0
        _same(d.data().reshape(-1, 2, e)[:, 1].reshape(-1), fill(500 * e, 2))
        d = build("empty", cplx)
        assert d.len() == 0 and not d.is_erroneous() and d.is_complex() == cplx
    assert build("shrunk-by-set_len-odd", False).len() == 1001
    d = build("exact-fit-real", False)
    assert d.len() == d.cap == 3439 and d.reallocs == 0 and vm.grown_cap(3000) == 3439
    d = build("exact-fit-complex", True)
    assert d.len() == d.cap == 3448 and d.reallocs == 0 and d.points() == 1724 and vm.grown_cap(3008) == 3448
    d = build("space-twice", False)
    assert not d.is_complex() and d.reallocs == 1 and d.trades == 2
    _same(d.data(), fill(1001, 0))
    d = build("get_real-destination", True)
    assert not d.is_complex() and d.len() == 1001 and d.reallocs == 1 and d.cap == vm.grown_cap(1001)
    _same(d.data(), fill(2002, 0)[0::2])


# ---------------------------------------------------------------------------------------------- the generator
@pytest.fixture(scope="module")
def logs():
    return {key: vm.gen_sequence(*key) for key in vm.all_sequences()}


def test_the_generator_is_deterministic_and_stays_in_bounds(logs):
    assert len(logs) == len(vm.START_POINTS) * 2 * len(vm.SEEDS) and vm.START_POINTS == (1, 16, 1001, 4096, 4097, 25700)
    for key in list(logs)[::7]:
        assert vm.gen_sequence(*key)[0] == logs[key][0]
    for (pts, cplx, seed), (seq, log) in logs.items():
        assert len(seq) == vm.STEPS == 16 and all(step[0] in vm.STEP_MOVERS for step in seq)
        v = VecModel(np.zeros(pts * (2 if cplx else 1), np.float32), cplx)   # replayed: every state within the bounds
        for step in seq:
            codes, v, side = vm.apply_step(vm.ModelApi, v, step)
            assert 1 <= v.len() <= vm.MAX_SCALARS == 1 << 20 and all(s.len() <= vm.MAX_SCALARS for s in side), (pts, cplx, seed, step)
    assert {mv for movers in vm.STEP_MOVERS.values() for mv in movers} == set(vm.MOVERS)


def test_the_seed_list_covers_every_mover_in_every_history(logs):
    """the conditions the GPU test's worth rests on, from the generator alone; more seeds if one fails, never a weaker
    condition.  get_real .. set_real_imag, split_into, merge and clone run on (or make) a vector that was never traded
    only in their destination; their SOURCE is the sequence's vector, and that is what the histories are about."""
    cov = vm.coverage([log for _, log in logs.values()])
    assert set(cov) == set(vm.MOVERS)
    for mover, c in cov.items():
        assert c["count"] >= 3, (mover, c)
        for h in vm.HISTORIES:
            assert c[h] >= 1, (mover, "never with history", h, c)
    assert any(ev["step"][0] == "set_len" and ev["exact_fit"] is False and ev["step"][1] > 0 for _, log in logs.values() for ev in log)


# ---------------------------------------------------------------------------------------------- the catalogue
# (these import basic_dsp_amd for DspVec's methods and docstrings, which loads the built library as the *_abi tests do:
# they need build() to have run, not a GPU)
def _public():
    from basic_dsp_amd.vector import DspVec
    return DspVec, {n for n, f in inspect.getmembers(DspVec, callable) if not n.startswith("_")}


def test_every_public_method_is_a_mover_an_accessor_or_catalogued():
    """a DspVec method added later without an entry in test_gpu_vec_sequences.CATALOGUE fails here, on the CPU"""
    import test_gpu_vec_sequences as seqs
    _, public = _public()
    catalogued = {entry.method for entry in seqs.CATALOGUE}
    movers = set(vm.MOVERS) - {"set_len"}   # set_len is the C ABI's: DspVec has no wrapper
    assert movers <= public and catalogued <= public and set(vm.ACCESSORS) <= public and set(vm.PLUMBING) <= public
    assert not movers & catalogued
    missing = public - movers - catalogued - set(vm.ACCESSORS) - set(vm.PLUMBING)
    assert not missing, "neither a mover nor catalogued: %s" % sorted(missing)


def test_no_entry_is_skipped_everywhere_and_few_pairs_are_skipped():
    """(entry, dirty state) pairs from the model alone: an entry runs on a state unless the state cannot satisfy the
    entry's precondition (number space, length).  Every entry runs on two states at least, and fewer than a quarter of all
    pairs are skipped."""
    import test_gpu_vec_sequences as seqs
    pairs = skipped = 0
    for entry in seqs.CATALOGUE:
        ran = 0
        for name, cplx in seqs.DIRTY_STATES:
            w = seqs.model_state(name, cplx, np.float32, entry)
            pairs += 1
            if seqs.applies(entry, w):
                ran += 1
            else:
                skipped += 1
        assert ran >= 2, (entry.label, "runs on", ran, "states")
    assert skipped * 4 < pairs, (skipped, pairs)


ARG_CODE = re.compile(r"(?<![\w.])7(?![\w.])|4 / 3 / 2")
POISONS = re.compile(r"\(poisoned\)|is poisoned|; poisoned\)|poisons")


def test_every_documented_argument_error_and_poisoning_has_an_entry():
    """the tables of test_gpu_vec_sequences.py against vector.py's docstrings: a method whose docstring names an
    argument-error code must be in ARG_ERRORS, one whose docstring says it poisons the vector in POISONERS.  vector.py
    documents few of them (dot_product's codes); the tables go further and hold every rejection that capi.cpp makes on
    the host before any launch, and this test keeps a docstring added later from outrunning them."""
    import test_gpu_vec_sequences as seqs
    cls, public = _public()
    docs = {n: inspect.getdoc(getattr(cls, n)) or "" for n in public}
    with_codes = {n for n, d in docs.items() if ARG_CODE.search(d)}
    poisoning = {n for n, d in docs.items() if POISONS.search(d)}
    assert "dot_product" in with_codes   # the pattern finds what it is meant to find
    tried = {row[0] for row in seqs.ARG_ERRORS}
    assert tried <= public | {"set_len"}
    assert not with_codes - tried, "documents an argument-error code, has no entry in ARG_ERRORS: %s" % sorted(with_codes - tried)
    codes = {c for row in seqs.ARG_ERRORS if row[0] == "dot_product" for c in ([row[4](True), row[4](False)] if callable(row[4]) else [row[4]])}
    assert {4, 3, 2} <= codes, codes
    poisoners = {row[0] for row in seqs.POISONERS}
    assert poisoners <= public
    assert not poisoning - poisoners, "documents poisoning, has no entry in POISONERS: %s" % sorted(poisoning - poisoners)
