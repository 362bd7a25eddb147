"""DspMat.prepare_argument / prepare_argument_padded / correlate: every row against the vector path, against the
float64 CPU oracle, against the reference's known answers, end to end as a pulse compressor, and the codes."""
import json
import os

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
KINDS = ("matrix", "vector")
FUSED = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
SURROUND = 1


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def tol_for(dtype):
    # what the project holds the vector path to (test_gpu_parity.py, test_correlate_and_prepare_argument)
    return 2e-6 if dtype == np.float32 else 1e-12


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def rows_per_workgroup(n):
    return 256 // (n // 16)  # k_mc_correlate: N/16 threads per row, 256 threads per workgroup


def sample_rows(rows, rpw=0):
    """at most 64 rows: first, last, both sides of the workgroup boundaries near the ends, the rest spread evenly"""
    if rows <= 64:
        return list(range(rows))
    s = {0, rows - 1}
    if rpw:
        last = (rows - 1) // rpw * rpw
        s |= {r for r in (rpw - 1, rpw, last - 1, last) if 0 <= r < rows}
    s |= set(np.linspace(0, rows - 1, 64 - len(s)).astype(int).tolist())
    return sorted(s)


def fused_shapes():
    """(rows, p, L): every fused N with p in {1, N/2, N/2+1, N-1} and an odd p at rows_per_workgroup + 1 rows; row
    counts 1, rows_per_workgroup - 1 and a non-multiple in the thousands for every N"""
    s = []
    for n in FUSED:
        rpw = rows_per_workgroup(n)
        odd = n // 4 + 3 if n > 16 else 5
        for p in (1, n // 2, n // 2 + 1, n - 1, odd):
            s.append((rpw + 1, p, n))
        s += [(1, n // 2 + 1, n), (max(rpw - 1, 1), n - 1, n), (1003, odd, n)]
    return s


def general_shapes():
    """(rows, p, L) off the fused kernel: L = 2n-1 for n in {2, 3, 13, 100, 1000, 1013, 4097} (8193 = 3 x 2731: Bluestein),
    and powers of two above 4096 with a few rows"""
    s = [(37, n, 2 * n - 1) for n in (2, 3, 13, 100)]
    s += [(300, 1000, 1999), (300, 1013, 2025), (5, 4097, 8193), (3, 5000, 8192), (3, 40000, 65536), (1, 7, 8)]
    return s


def make_case(bd, rows, p, l, dtype, kind, seed):
    """the matrix (host rows, device), the prepared argument (device) and its unprepared host rows (l points each, the
    p-point template Surround-padded, or 2p-1 by prepare_argument_padded)"""
    x = orc.fill_uniform(rows * 2 * p, seed, -10, 10, dtype).reshape(rows, 2 * p)
    arows = rows if kind == "matrix" else 1
    y = orc.fill_uniform(arows * 2 * p, seed + 7, -10, 10, dtype).reshape(arows, 2 * p)
    if kind == "matrix":
        arg = bd.DspMat(y, is_complex=True)
    else:
        arg = bd.DspVec(y[0], is_complex=True)
    if l == 2 * p - 1:
        assert arg.prepare_argument_padded() == 0
    else:
        assert arg.zero_pad(l, SURROUND) == 0
        assert arg.prepare_argument() == 0
    return x, bd.DspMat(x, is_complex=True), y, arg


def oracle_argument(y_row, p, l):
    yd = y_row.astype(np.float64)
    if l == 2 * p - 1:
        code, ref = orc.prepare_argument(yd, True)
    else:
        code, padded = orc.zero_pad(yd, True, l, SURROUND, buffered=True)  # zero_pad_b: the split the device makes
        assert code == 0
        code, ref = orc.prepare_argument(padded, False)
    assert code == 0
    return ref


def check_meta(m, arg, rows, l, bd):
    assert m.rows() == rows and m.row_points() == l and m.row_len() == 2 * l
    assert m.is_complex() and m.domain() == 0 and m.delta() == 1.0
    assert arg.is_complex() and arg.domain() == 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_equal_the_vector_path(bd, dtype, kind):
    tol = 2 * tol_for(dtype)  # each side is held to the oracle tolerance
    shapes = fused_shapes() + general_shapes()
    if dtype == np.float32:
        shapes.append((16384, 1000, 2048))  # one large batch
    worst = 0.0
    for k, (rows, p, l) in enumerate(shapes):
        x, m, _, arg = make_case(bd, rows, p, l, dtype, kind, 4000 + k)
        before = arg.data().copy()
        assert m.correlate(arg) == 0, (rows, p, l)
        check_meta(m, arg, rows, l, bd)
        assert np.array_equal(before, arg.data()), (rows, p, l)  # `other` is not modified
        got = m.data()
        rpw = rows_per_workgroup(l) if l in FUSED else 0
        for r in sample_rows(rows, rpw):
            v = bd.DspVec(x[r], is_complex=True)
            a = arg.get_row(r) if kind == "matrix" else arg
            assert v.correlate(a) == 0
            e = rel_l2(got[r], v.data())
            worst = max(worst, e)
            assert e < tol, (rows, p, l, r, e)
        if k % 8 == 0:  # no atomics: equal inputs give equal bits
            m2 = bd.DspMat(x, is_complex=True)
            assert m2.correlate(arg) == 0
            assert np.array_equal(m2.data(), got), (rows, p, l)
    print("worst rel-L2 to the vector path (%s, %s): %.3e" % (np.dtype(dtype).name, kind, worst))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_oracle(bd, dtype, kind):
    tol = tol_for(dtype)
    shapes = [(rows_per_workgroup(n) + 1, n // 2 + 1, n) for n in FUSED]
    shapes += [(1003, 1000, 2048), (67, 4095, 4096), (19, 1, 64)] + general_shapes()
    worst_arg = worst = 0.0
    for k, (rows, p, l) in enumerate(shapes):
        x, m, y, arg = make_case(bd, rows, p, l, dtype, kind, 9000 + k)
        argd = arg.data().reshape(-1, 2 * l)
        assert m.correlate(arg) == 0, (rows, p, l)
        got = m.data()
        rpw = rows_per_workgroup(l) if l in FUSED else 0
        for r in sample_rows(rows, rpw):
            ar = r if kind == "matrix" else 0
            ref_arg = oracle_argument(y[ar], p, l)
            ea = rel_l2(argd[ar], ref_arg)
            worst_arg = max(worst_arg, ea)
            assert ea < tol, ("argument", rows, p, l, r, ea)
            code, ref = orc.correlate(x[r].astype(np.float64), ref_arg)
            assert code == 0
            e = rel_l2(got[r], ref)
            worst = max(worst, e)
            assert e < tol, (rows, p, l, r, e)
    print("worst rel-L2 to the oracle (%s, %s): argument %.3e, correlate %.3e" %
          (np.dtype(dtype).name, kind, worst_arg, worst))


@pytest.mark.parametrize("dtype", DTYPES)
def test_prepare_argument_of_real_rows_and_delta(bd, dtype):
    """real rows become complex as in op_fft; delta <- points * delta; rows equal the vector call"""
    tol = tol_for(dtype)
    for rows, p, padded in ((5, 64, False), (5, 64, True), (130, 100, True), (3, 1013, False)):
        x = orc.fill_uniform(rows * p, 77 + p, -10, 10, dtype).reshape(rows, p)
        m = bd.DspMat(x, is_complex=False, delta=0.5)
        assert (m.prepare_argument_padded() if padded else m.prepare_argument()) == 0
        pts = 2 * p - 1 if padded else p
        assert m.is_complex() and m.domain() == 1 and m.row_points() == pts and m.delta() == 0.5 * pts
        got = m.data()
        for r in range(rows):
            v = bd.DspVec(x[r], is_complex=False, delta=0.5)
            assert (v.prepare_argument_padded() if padded else v.prepare_argument()) == 0
            assert v.delta() == m.delta()
            assert rel_l2(got[r], v.data()) < 2 * tol, (rows, p, padded, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_known_answers(bd, dtype):
    # the doc example of correlation.rs:52-62 (as test_gpu_parity.test_correlate_and_prepare_argument states it)
    a = np.array([1, 1, 2, 1, 3, 1], dtype)
    b = np.array([4, 1, 5, 1, 6, 1], dtype)
    want = np.array([7, 5, 19, 8, 35, 9, 25, 4, 13, 1], np.float64)
    for rows in (1, 3, 300):
        for kind in KINDS:
            m = bd.DspMat(np.tile(a, (rows, 1)), is_complex=True)
            arg = bd.DspMat(np.tile(b, (rows, 1)), is_complex=True) if kind == "matrix" else bd.DspVec(b, is_complex=True)
            assert arg.prepare_argument_padded() == 0
            assert arg.domain() == 1 and (arg.row_points() if kind == "matrix" else arg.points()) == 5
            assert m.correlate(arg) == 0
            assert m.delta() == 1.0 and m.domain() == 0 and m.row_points() == 5
            np.testing.assert_allclose(m.data(), np.tile(want, (rows, 1)), atol=1e-4)
    # correlation.rs:171-215, as test_oracle_golden.test_correlate_kats uses them (tolerance 0.1)
    with open(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")) as f:
        kats = json.load(f)
    for name in ("time_correlation_test", "time_correlation_test2"):
        a, b, want = (np.array(kats[name]["arrays"][i]) for i in (0, 1, 2))
        for rows in (1, 3):
            for kind in KINDS:
                m = bd.DspMat(np.tile(a.astype(dtype), (rows, 1)), is_complex=True)
                bb = b.astype(dtype)
                arg = bd.DspMat(np.tile(bb, (rows, 1)), is_complex=True) if kind == "matrix" else bd.DspVec(bb, is_complex=True)
                assert arg.prepare_argument_padded() == 0
                assert m.correlate(arg) == 0
                np.testing.assert_allclose(m.data(), np.tile(want, (rows, 1)), atol=0.1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pulse_compression_end_to_end(bd, dtype):
    """row r = the template delayed by d_r plus 1 % noise; correlate -> magnitude -> statistics()['max_index'] is the lag"""
    rows, n, l = 777, 600, 2048  # fused length, vector argument
    rng = np.random.default_rng(20240607)
    t = np.arange(64)
    chirp = np.exp(1j * np.pi * 0.9 * (t - 32.0) ** 2 / 64.0)  # a 64-point linear FM pulse, amplitude 1
    delays = (np.arange(rows) * 37) % (n - 64)
    z = np.zeros((rows, n), np.complex128)
    for r in range(rows):
        z[r, delays[r]:delays[r] + 64] = chirp
    z += 0.01 * (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))) / np.sqrt(2)
    x = np.ascontiguousarray(z).view(np.float64).astype(dtype)
    tmpl = np.zeros(n, np.complex128)
    tmpl[:64] = chirp
    y = np.ascontiguousarray(tmpl).view(np.float64).astype(dtype)

    arg = bd.DspVec(y, is_complex=True)
    assert arg.zero_pad(l, SURROUND) == 0 and arg.prepare_argument() == 0
    m = bd.DspMat(x, is_complex=True)
    assert m.correlate(arg) == 0 and m.magnitude() == 0
    assert not m.is_complex() and m.row_len() == l
    got = m.statistics()["max_index"]

    ref_arg = oracle_argument(y, n, l)
    want = np.empty(rows, np.int64)
    for r in range(rows):
        code, c = orc.correlate(x[r].astype(np.float64), ref_arg)
        assert code == 0
        mag = np.hypot(c[0::2], c[1::2])
        order = np.argsort(mag)
        # unambiguous: the second-largest magnitude is below half the maximum
        assert mag[order[-2]] < 0.5 * mag[order[-1]], (r, mag[order[-2]], mag[order[-1]])
        want[r] = order[-1]
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    # and the peak moves with the delay, one lag per sample
    assert np.array_equal(want - want[0], delays - delays[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_codes_and_state(bd, dtype):
    def poisoned(m):
        return m.row_len() == 0 and np.isnan(m.delta())

    x = orc.fill_uniform(3 * 16, 5, -10, 10, dtype).reshape(3, 16)  # 3 rows of 8 complex points
    y = orc.fill_uniform(3 * 64, 6, -10, 10, dtype).reshape(3, 64)  # 3 rows of 32
    for kind in KINDS:
        def argument(prepared=True, rows=3):
            a = bd.DspMat(y[:rows], is_complex=True) if kind == "matrix" else bd.DspVec(y[0], is_complex=True)
            if prepared:
                assert a.prepare_argument() == 0
            return a
        # an unprepared (time-domain) argument: 5, m poisoned, later calls -1
        m = bd.DspMat(x, is_complex=True)
        assert m.correlate(argument(prepared=False)) == 5 and poisoned(m)
        assert m.correlate(argument()) == 5  # a poisoned matrix is not complex / time any more: same report
        assert m.scale(2.0) == -1
        # a real matrix: 5, poisoned
        m = bd.DspMat(x, is_complex=False)
        assert m.correlate(argument()) == 5 and poisoned(m) and m.conj() == -1
        # L <= p: 7, data unchanged
        big = orc.fill_uniform(3 * 64, 8, -10, 10, dtype).reshape(3, 64)
        for pts in (32, 40):
            src = big if pts == 32 else orc.fill_uniform(3 * 80, 9, -10, 10, dtype).reshape(3, 80)
            m = bd.DspMat(src, is_complex=True)
            assert m.correlate(argument()) == 7
            assert np.array_equal(m.data(), src) and m.domain() == 0 and m.row_points() == pts
        # zero rows: 0
        m = bd.DspMat(is_complex=True, dtype=dtype, rows=0, row_len=16)
        a0 = bd.DspMat(is_complex=True, domain=1, dtype=dtype, rows=0, row_len=64) if kind == "matrix" else argument()
        assert m.correlate(a0) == 0 and m.rows() == 0
    # unequal row counts: 7, m unchanged
    m = bd.DspMat(x, is_complex=True)
    a2 = bd.DspMat(y[:2], is_complex=True)
    assert a2.prepare_argument() == 0
    assert m.correlate(a2) == 7 and np.array_equal(m.data(), x)
    # prepare_argument_padded on one-point rows: 7, untouched
    one = orc.fill_uniform(3 * 2, 10, -10, 10, dtype).reshape(3, 2)
    m = bd.DspMat(one, is_complex=True)
    assert m.prepare_argument_padded() == 7 and np.array_equal(m.data(), one) and m.domain() == 0
    # prepare_argument on a frequency-domain matrix poisons it, as the vector call reports it
    m = bd.DspMat(x, is_complex=True, domain=1)
    v = bd.DspVec(x[0], is_complex=True, domain=1)
    assert m.prepare_argument() == v.prepare_argument() == -1 and poisoned(m)
    # zero rows
    m = bd.DspMat(is_complex=True, dtype=dtype, rows=0, row_len=16)
    assert m.prepare_argument() == 0 and m.rows() == 0
