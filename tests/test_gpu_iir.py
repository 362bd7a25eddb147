"""sosfilt: IIR filtering of a DspVec or of every row of a DspMat on the device, through the Python function.

There is no forward bound for a recursive filter that holds independently of the filter, so the yardstick is the
recurrence itself.  Per row (a complex row is two real signals), on the coefficients as rounded to the data's precision T:

    truth  the serial recurrence in numpy float64 (f32 data) or longdouble (f64 data)
    e_ser  max over the row of |the serial recurrence in T, every operation rounded on its own, - truth|
    e_dev  the same maximum for the device result

and the assertion is e_dev <= R max(e_ser, eps max|truth|), eps = np.finfo(T).eps.  Final states are held to the same
construction on the state vector.  R = 16: twice the larger of the worst ratios measured in the host simulation
(tests/host_sim/sim_iir.cpp on the same shapes: 2.84 for outputs, 4.84 for states) and on an MI355X (2.99 and 5.47;
DESIGN.md 4.19, profiles/iir.txt), rounded up to a power of two.  Both models are written here and use no scipy.  The shapes are
tests/iir_shapes.txt, which the host simulation reads too.  Every accuracy test prints its worst ratio."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 16.0
TILE = 4096
MAX_SECTIONS = 16
KINDS = [("real", "f32"), ("complex", "f32"), ("real", "f64"), ("complex", "f64")]
KIND_IDS = ["%s-%s" % k for k in KINDS]


def read_shapes():
    out = []
    with open(os.path.join(ROOT, "tests", "iir_shapes.txt")) as f:
        for line in f:
            w = line.split("#")[0].split()
            if w:
                out.append((w[0], w[1], int(w[2]), int(w[3]), int(w[4]), w[5]))
    return out


SHAPES = read_shapes()


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    assert np.finfo(np.longdouble).nmant >= 63
    return b


def make_sos(family, S):
    """the families of tests/iir_shapes.txt: pole pairs r e^(+-i theta), zeros at -1, unit gain at DC"""
    sos = np.zeros((S, 6))
    for k in range(S):
        if family == "fir":
            sos[k] = [0.25, 0.5, 0.25, 1, 0, 0]
            continue
        if family == "integrator" and k == 0:
            sos[k] = [1, 0, 0, 1, -1, 0]
            continue
        r, th = 0.70 + 0.25 * (k + 1) / (S + 1), np.pi * (0.10 + 0.15 * k / S)
        if family == "resonator" and k == 0:
            r, th = 0.9995, 0.05 * np.pi
        a1, a2 = -2 * r * np.cos(th), r * r
        g = (1 + a1 + a2) / 4
        sos[k] = [g, 2 * g, g, 1, a1, a2]
    return sos


def rounded(sos, dtype):
    """b0 b1 b2 a1 a2 per section: divided by a0 in double, rounded once to the data's precision"""
    sos = np.asarray(sos, dtype=np.float64).reshape(-1, 6)
    return (sos[:, [0, 1, 2, 4, 5]] / sos[:, 3:4]).astype(dtype)


def serial(coef, x, state, prec):
    """The recurrence in precision `prec`, every operation rounded on its own.  x: [signals, n]; state: [signals, 2S] or
    None; returns (y, final state).  Vectorised over the signals only."""
    y = x.astype(prec).T.copy()  # [n, signals]
    sig = y.shape[1]
    out = np.zeros((sig, 2 * len(coef)), dtype=prec)
    for k, c in enumerate(coef.astype(prec)):
        b0, b1, b2, a1, a2 = c
        s1 = (state[:, 2 * k] if state is not None else np.zeros(sig)).astype(prec)
        s2 = (state[:, 2 * k + 1] if state is not None else np.zeros(sig)).astype(prec)
        bx0, bx1, bx2 = b0 * y, b1 * y, b2 * y
        for i in range(y.shape[0]):
            yi = bx0[i] + s1
            s1 = (bx1[i] - a1 * yi) + s2
            s2 = bx2[i] - a2 * yi
            y[i] = yi
        out[:, 2 * k], out[:, 2 * k + 1] = s1, s2
    return y.T, out


def signals(a, cplx):
    """[rows, n * C] scalars -> [rows * C, n] real signals (row-major: row 0 re, row 0 im, row 1 re, ...)"""
    a = np.asarray(a)
    if not cplx:
        return a
    return a.reshape(a.shape[0], -1, 2).transpose(0, 2, 1).reshape(a.shape[0] * 2, -1)


def yardstick(got, truth, ser, eps):
    """worst over the signals of e_dev / max(e_ser, eps max|truth|)"""
    if truth.shape[1] == 0:
        return 0.0
    e_dev = np.max(np.abs(got.astype(truth.dtype) - truth), axis=1)
    e_ser = np.max(np.abs(ser.astype(truth.dtype) - truth), axis=1)
    floor = eps * np.max(np.abs(truth), axis=1)
    return float(np.max(e_dev / np.maximum(np.maximum(e_ser, floor), np.finfo(np.float64).tiny)))


def models(sos, x, state, dtype, cplx):
    """(truth y, T-precision y, truth state, T-precision state) on the signals of x"""
    wide = np.float64 if dtype == np.float32 else np.longdouble
    coef = rounded(sos, dtype)
    xs = signals(x, cplx)
    st = signals(state, cplx) if state is not None else None
    ty, ts = serial(coef, xs, st, wide)
    sy, ss = serial(coef, xs, st, dtype)
    return ty, sy, ts, ss


def draw(seed, rows, n, dtype, cplx):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (rows, n * (2 if cplx else 1))).astype(dtype)


def kind_of(kind, prec):
    return (np.float32 if prec == "f32" else np.float64), kind == "complex"


_worst = {"out": 0.0, "state": 0.0}


@pytest.mark.parametrize("line", range(len(SHAPES)), ids=["-".join(str(w) for w in s) for s in SHAPES])
def test_accuracy_on_every_shape_line_for_matrix_and_vector(bd, line):
    kind, prec, rows, n, S, family = SHAPES[line]
    dtype, cplx = kind_of(kind, prec)
    eps = np.finfo(dtype).eps
    sos = make_sos(family, S)
    x = draw(1000 + line, rows, n, dtype, cplx)
    ty, sy, _, _ = models(sos, x, None, dtype, cplx)
    m = bd.DspMat(x, is_complex=cplx, delta=0.5)
    assert bd.sosfilt(m, sos) == 0
    assert (m.rows(), m.row_len(), m.is_complex(), m.domain(), m.delta()) == (rows, x.shape[1], cplx, 0, 0.5)
    got = m.data()
    ratio = yardstick(signals(got, cplx), ty, sy, eps)
    v = bd.DspVec(x[rows - 1], is_complex=cplx, delta=0.5)
    assert bd.sosfilt(v, sos) == 0
    assert (len(v), v.is_complex(), v.domain(), v.delta()) == (x.shape[1], cplx, 0, 0.5)
    gv = v.data()
    C = 2 if cplx else 1
    ratio_v = yardstick(signals(gv.reshape(1, -1), cplx), ty[(rows - 1) * C:], sy[(rows - 1) * C:], eps)
    _worst["out"] = max(_worst["out"], ratio, ratio_v)
    print("ratio matrix %.3f vector %.3f (worst so far %.3f)" % (ratio, ratio_v, _worst["out"]))
    assert ratio <= R and ratio_v <= R
    assert np.array_equal(gv.view(np.uint8), got[rows - 1].view(np.uint8))  # the matrix row is the vector call, bit for bit


@pytest.mark.parametrize("n", [17, TILE, TILE + 1, 2 * TILE + 17])
@pytest.mark.parametrize("kind,prec", KINDS, ids=KIND_IDS)
def test_rows_are_bit_equal_to_vector_calls_independent_and_deterministic(bd, kind, prec, n):
    dtype, cplx = kind_of(kind, prec)
    sos = make_sos("resonator", 2)
    x = draw(7 + n, 3, n, dtype, cplx)
    m = bd.DspMat(x, is_complex=cplx)
    assert bd.sosfilt(m, sos) == 0
    got = m.data()
    for r in range(3):
        v = bd.DspVec(x[r], is_complex=cplx)
        assert bd.sosfilt(v, sos) == 0
        assert np.array_equal(v.data().view(np.uint8), got[r].view(np.uint8)), r
    again = bd.DspMat(x, is_complex=cplx)
    assert bd.sosfilt(again, sos) == 0
    assert np.array_equal(again.data().view(np.uint8), got.view(np.uint8))
    other = x.copy()
    other[1] = draw(99, 1, n, dtype, cplx)[0] * 1000
    mo = bd.DspMat(other, is_complex=cplx)
    assert bd.sosfilt(mo, sos) == 0
    go = mo.data()
    assert np.array_equal(go[0].view(np.uint8), got[0].view(np.uint8)) and np.array_equal(go[2].view(np.uint8), got[2].view(np.uint8))
    # one row more or fewer: the bits of a row do not depend on the row count
    one = bd.DspMat(x[2:3], is_complex=cplx)
    assert bd.sosfilt(one, sos) == 0
    assert np.array_equal(one.data()[0].view(np.uint8), got[2].view(np.uint8))


@pytest.mark.parametrize("family,S", [("resonator", 2), ("lowpass", 8)])
@pytest.mark.parametrize("kind,prec", KINDS, ids=KIND_IDS)
def test_streaming_in_two_pieces_carries_the_state(bd, kind, prec, family, S):
    dtype, cplx = kind_of(kind, prec)
    eps = np.finfo(dtype).eps
    C = 2 if cplx else 1
    n, cut, rows = 2 * TILE + 17, 5000, 3
    sos = make_sos(family, S)
    x = draw(31 + S, rows, n, dtype, cplx)
    ty, sy, ts, ss = models(sos, x, None, dtype, cplx)
    state = bd.DspMat(np.zeros((rows, 2 * S * C), dtype), is_complex=cplx)
    a, b = bd.DspMat(x[:, :cut * C], is_complex=cplx), bd.DspMat(x[:, cut * C:], is_complex=cplx)
    assert bd.sosfilt(a, sos, state) == 0
    assert bd.sosfilt(b, sos, state) == 0
    got = np.concatenate([a.data(), b.data()], axis=1)
    ratio = yardstick(signals(got, cplx), ty, sy, eps)
    final = signals(state.data(), cplx)
    ratio_s = yardstick(final, ts, ss, eps)
    print("streaming ratio %.3f, final state ratio %.3f" % (ratio, ratio_s))
    assert ratio <= R and ratio_s <= R
    # the vector form on row 1, in the same two pieces: the same bits, state included
    sv = bd.DspVec(np.zeros(2 * S * C, dtype), is_complex=cplx)
    va, vb = bd.DspVec(x[1, :cut * C], is_complex=cplx), bd.DspVec(x[1, cut * C:], is_complex=cplx)
    assert bd.sosfilt(va, sos, sv) == 0 and bd.sosfilt(vb, sos, sv) == 0
    assert np.array_equal(np.concatenate([va.data(), vb.data()]).view(np.uint8), got[1].view(np.uint8))
    assert np.array_equal(sv.data().view(np.uint8), state.data()[1].view(np.uint8))


@pytest.mark.parametrize("n", [1, 1000, TILE, 2 * TILE + 17])
@pytest.mark.parametrize("kind,prec", KINDS, ids=KIND_IDS)
def test_a_non_zero_incoming_state(bd, kind, prec, n):
    dtype, cplx = kind_of(kind, prec)
    eps = np.finfo(dtype).eps
    S, rows = 3, 2
    sos = make_sos("resonator", S)
    x = draw(57 + n, rows, n, dtype, cplx)
    s0 = draw(58 + n, rows, 2 * S, dtype, cplx)
    ty, sy, ts, ss = models(sos, x, s0, dtype, cplx)
    m, state = bd.DspMat(x, is_complex=cplx), bd.DspMat(s0, is_complex=cplx)
    assert bd.sosfilt(m, sos, state) == 0
    ratio = yardstick(signals(m.data(), cplx), ty, sy, eps)
    ratio_s = yardstick(signals(state.data(), cplx), ts, ss, eps)
    print("ratio %.3f, final state ratio %.3f" % (ratio, ratio_s))
    assert ratio <= R and ratio_s <= R
    assert (state.rows(), state.row_points(), state.is_complex()) == (rows, 2 * S, cplx)


@pytest.mark.parametrize("n", [100, 2 * TILE + 17])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_complex_data_are_two_real_signals_bit_for_bit(bd, dtype, n):
    S = 2
    sos = make_sos("lowpass", S)
    x, s0 = draw(5, 1, n, dtype, True)[0], draw(6, 1, 2 * S, dtype, True)[0]
    v, st = bd.DspVec(x, is_complex=True), bd.DspVec(s0, is_complex=True)
    assert bd.sosfilt(v, sos, st) == 0
    y, sf = v.data(), st.data()
    for part in range(2):
        r, sr = bd.DspVec(x[part::2].copy()), bd.DspVec(s0[part::2].copy())
        assert bd.sosfilt(r, sos, sr) == 0
        assert np.array_equal(r.data().view(np.uint8), y[part::2].copy().view(np.uint8)), part
        assert np.array_equal(sr.data().view(np.uint8), sf[part::2].copy().view(np.uint8)), part


@pytest.mark.parametrize("kind,prec", KINDS, ids=KIND_IDS)
def test_the_integrator_counts_and_a0_divides(bd, kind, prec):
    dtype, cplx = kind_of(kind, prec)
    C = 2 if cplx else 1
    n = 2 * TILE + 17
    m = bd.DspMat(np.ones((2, n * C), dtype), is_complex=cplx)
    assert bd.sosfilt(m, [[1, 0, 0, 1, -1, 0]]) == 0
    want = np.repeat(np.arange(1, n + 1), C).astype(dtype)
    assert np.array_equal(m.data(), np.stack([want, want]))  # cum_sum's meaning, exactly
    c = bd.DspMat(np.ones((2, n * C), dtype), is_complex=cplx)
    assert c.cum_sum() == 0
    assert np.array_equal(c.data(), m.data())
    # a0 = 4 with every coefficient four times as large: the same rounded section, the same bits
    sos = make_sos("resonator", 2)
    x = draw(3, 2, n, dtype, cplx)
    p, q = bd.DspMat(x, is_complex=cplx), bd.DspMat(x, is_complex=cplx)
    assert bd.sosfilt(p, sos) == 0 and bd.sosfilt(q, sos * 4.0) == 0
    assert np.array_equal(p.data().view(np.uint8), q.data().view(np.uint8))


def _poisoned_vec(bd, dtype):
    v = bd.DspVec(np.ones(4, dtype))
    assert v.magnitude() == -1 and v.is_erroneous()
    return v


def _poisoned_mat(bd, dtype):
    m = bd.DspMat(np.ones((2, 4), dtype))
    assert m.conj() == -1
    return m


@pytest.mark.parametrize("kind,prec", KINDS, ids=KIND_IDS)
def test_codes_and_edge_cases(bd, kind, prec):
    dtype, cplx = kind_of(kind, prec)
    C = 2 if cplx else 1
    S = 2
    sos = make_sos("lowpass", S)
    x = draw(11, 3, 40, dtype, cplx)

    def fresh():
        return (bd.DspMat(x, is_complex=cplx), bd.DspVec(x[0], is_complex=cplx),
                bd.DspMat(np.ones((3, 2 * S * C), dtype), is_complex=cplx), bd.DspVec(np.ones(2 * S * C, dtype), is_complex=cplx))

    def untouched(m, v, sm=None, sv=None):
        assert np.array_equal(m.data().view(np.uint8), x.view(np.uint8)) and np.array_equal(v.data().view(np.uint8), x[0].view(np.uint8))
        if sm is not None:
            assert np.all(sm.data() == 1) and np.all(sv.data() == 1)

    # 7: sos not [S, 6], a coefficient that is not finite, a0 == 0, too many sections
    bad_a0, nan, inf = sos.copy(), sos.copy(), sos.copy()
    bad_a0[1, 3], nan[0, 1], inf[1, 5] = 0.0, np.nan, np.inf
    for bad in (sos[:, :5], sos.ravel(), sos.reshape(1, 2, 6), [1, 2, 3], bad_a0, nan, inf, make_sos("lowpass", MAX_SECTIONS + 1)):
        m, v, sm, sv = fresh()
        assert bd.sosfilt(m, bad) == 7 and bd.sosfilt(v, bad) == 7
        assert bd.sosfilt(m, bad, sm) == 7 and bd.sosfilt(v, bad, sv) == 7
        untouched(m, v, sm, sv)
    # the maximum itself is accepted
    m, v, _, _ = fresh()
    assert bd.sosfilt(m, make_sos("lowpass", MAX_SECTIONS)) == 0 and bd.sosfilt(v, make_sos("lowpass", MAX_SECTIONS)) == 0
    # 7: a state of the wrong shape
    m, v, sm, sv = fresh()
    for wrong in (bd.DspMat(np.ones((3, 2 * S * C + C), dtype), is_complex=cplx), bd.DspMat(np.ones((2, 2 * S * C), dtype), is_complex=cplx)):
        assert bd.sosfilt(m, sos, wrong) == 7
    assert bd.sosfilt(v, sos, bd.DspVec(np.ones(2 * S * C - C, dtype), is_complex=cplx)) == 7
    untouched(m, v)
    # 2: a state of the other number kind (with as many points as the right one)
    other_m = bd.DspMat(np.ones((3, 2 * S * (3 - C)), dtype), is_complex=not cplx)
    other_v = bd.DspVec(np.ones(2 * S * (3 - C), dtype), is_complex=not cplx)
    assert bd.sosfilt(m, sos, other_m) == 2 and bd.sosfilt(v, sos, other_v) == 2
    untouched(m, v)
    # 5: frequency-domain data
    fm, fv = bd.DspMat(x, is_complex=cplx, domain=1), bd.DspVec(x[0], is_complex=cplx, domain=1)
    assert bd.sosfilt(fm, sos) == 5 and bd.sosfilt(fv, sos) == 5
    assert np.array_equal(fm.data().view(np.uint8), x.view(np.uint8))
    # -1: a poisoned x or state
    assert bd.sosfilt(_poisoned_mat(bd, dtype), sos) == -1 and bd.sosfilt(_poisoned_vec(bd, dtype), sos) == -1
    assert bd.sosfilt(m, sos, _poisoned_mat(bd, dtype)) == -1 and bd.sosfilt(v, sos, _poisoned_vec(bd, dtype)) == -1
    untouched(m, v)
    # TypeError: another class or precision
    other = np.float64 if dtype == np.float32 else np.float32
    for bad_state in (np.ones(2 * S * C, dtype), sv, bd.DspMat(np.ones((3, 2 * S * C), other), is_complex=cplx)):
        with pytest.raises(TypeError):
            bd.sosfilt(m, sos, bad_state)
    for bad_state in (sm, bd.DspVec(np.ones(2 * S * C, other), is_complex=cplx), [0.0] * 4):
        with pytest.raises(TypeError):
            bd.sosfilt(v, sos, bad_state)
    untouched(m, v, sm, sv)
    # S == 0, no rows, rows of no points: 0 and nothing changes
    assert bd.sosfilt(m, np.zeros((0, 6))) == 0 and bd.sosfilt(v, np.zeros((0, 6))) == 0
    assert bd.sosfilt(m, np.zeros((0, 6)), bd.DspMat(np.zeros((3, 0), dtype), is_complex=cplx)) == 0
    untouched(m, v)
    for empty in (bd.DspMat(np.zeros((0, 8 * C), dtype), is_complex=cplx), bd.DspMat(np.zeros((3, 0), dtype), is_complex=cplx)):
        rows = empty.rows()
        assert bd.sosfilt(empty, sos) == 0 and (empty.rows(), empty.row_len()) == (rows, 0 if rows else empty.row_len())
    e3 = bd.DspMat(np.zeros((3, 0), dtype), is_complex=cplx)
    assert bd.sosfilt(e3, sos, sm) == 0 and np.all(sm.data() == 1)  # rows of no points: the state stays
    ev = bd.DspVec(np.zeros(0, dtype), is_complex=cplx)
    assert bd.sosfilt(ev, sos, sv) == 0 and len(ev) == 0 and np.all(sv.data() == 1)
    # an unstable filter: inf or NaN as the recurrence gives them, code 0
    u = bd.DspVec(np.ones(2000 * C, dtype), is_complex=cplx)
    assert bd.sosfilt(u, [[1, 0, 0, 1, -4, 0]]) == 0
    assert not np.all(np.isfinite(u.data()))


def test_chain_interpolatef_sosfilt_matmul(bd):
    from basic_dsp_amd import vector as V
    rng = np.random.default_rng(77)
    x = rng.uniform(-1, 1, (8, 441)).astype(np.float32)
    sos = make_sos("lowpass", 2)
    ch = bd.DspMat(x)
    assert ch.interpolatef(V.CONV_RAISED_COSINE, 48 / 44.1, np.linspace(-0.5, 0.5, 8), 12, rolloff=0.35) == 0
    resampled = ch.data()
    assert resampled.shape == (8, 480)
    assert bd.sosfilt(ch, sos) == 0
    ty, sy, _, _ = models(sos, resampled, None, np.float32, False)
    assert yardstick(ch.data(), ty, sy, np.finfo(np.float32).eps) <= R
    w = rng.uniform(-1, 1, (2, 8)).astype(np.float32)
    code, beams = bd.matmul(bd.DspMat(w), ch)
    assert code == 0 and (beams.rows(), beams.row_points()) == (2, 480)
    got = ch.data().astype(np.float64)  # matmul's own bound on the filtered rows: (2 K + 4) eps sum |a| |b|, K = 8
    assert np.all(np.abs(beams.data() - w.astype(np.float64) @ got) <= 20 * np.finfo(np.float32).eps * (np.abs(w).astype(np.float64) @ np.abs(got)))


@pytest.mark.parametrize("kind,prec", KINDS, ids=KIND_IDS)
def test_zero_phase_composition(bd, kind, prec):
    dtype, cplx = kind_of(kind, prec)
    eps = np.finfo(dtype).eps
    C = 2 if cplx else 1
    n = TILE + 100
    sos = make_sos("lowpass", 2)
    x = draw(21, 2, n, dtype, cplx)
    m = bd.DspMat(x, is_complex=cplx)
    assert bd.sosfilt(m, sos) == 0 and m.reverse() == 0 and bd.sosfilt(m, sos) == 0 and m.reverse() == 0
    # the model on the device's own intermediate: forward pass, then the backward pass on its reversed output
    f = bd.DspMat(x, is_complex=cplx)
    assert bd.sosfilt(f, sos) == 0
    mid = f.data().reshape(2, n, C)[:, ::-1, :].reshape(2, n * C).copy()
    ty, sy, _, _ = models(sos, mid, None, dtype, cplx)
    got = m.data().reshape(2, n, C)[:, ::-1, :].reshape(2, n * C)
    assert yardstick(signals(got, cplx), ty, sy, eps) <= R
    # zero phase: a slow cosine in the middle of the row comes back in phase (its delay is cancelled), scaled by |H|^2
    t = np.arange(n)
    tone = np.cos(2 * np.pi * t / 512.0)
    z = bd.DspVec(tone.astype(dtype))
    assert bd.sosfilt(z, sos) == 0 and z.reverse() == 0 and bd.sosfilt(z, sos) == 0 and z.reverse() == 0
    y = z.data().astype(np.float64)[1024:-1024]
    ref = tone[1024:-1024]
    gain = np.dot(y, ref) / np.dot(ref, ref)
    zi = np.exp(-2j * np.pi / 512.0)
    h2 = np.prod(np.abs((sos[:, 0] + sos[:, 1] * zi + sos[:, 2] * zi * zi) / (sos[:, 3] + sos[:, 4] * zi + sos[:, 5] * zi * zi)) ** 2)
    assert np.max(np.abs(y - gain * ref)) <= 1e-3 * abs(gain) and abs(gain - h2) <= 1e-4 * h2
