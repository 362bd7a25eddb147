"""DspMat.interpolatei / interpolate / interpft / decimatei: every row against the float64 CPU oracle and against the
vector path, on the one-launch (fused) path and on the general path; row isolation, determinism, the codes, and end to
end behind a pulse compressor.

Tolerances are the ones the project holds the vector path to (test_gpu_parity.py,
test_interpolatei_interpolate_decimatei): interpolatei rel-L2 < 5e-6 (f32) / 1e-11 (f64), interpolate / interpft
< 2e-5 / 1e-10, decimatei bit-equal.

Since the second batch of DESIGN.md 4.4 DspVec.decimatei launches k_rs_decimate_rows with one row through the same host
function, so decimatei "against the vector path" no longer spans two implementations (the vector's own reference:
tests/test_gpu_vec_one_row.py); interpolatei, interpolate and interpft against the vector path still do: the vector keeps
k_spectrum_resample and ew_linear_phase, and never takes the fused kernel."""
import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
FUSED = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
SINC, RAISED_COSINE = 0, 1
SURROUND = 1


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def tol_for(op, dtype):
    if op[0] == "interpolatei":
        return 5e-6 if dtype == np.float32 else 1e-11
    return 2e-5 if dtype == np.float32 else 1e-10


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def rows_per_workgroup(n):
    return 256 // (n // 16)  # k_rs_fused: N/16 threads per row, 256 threads per workgroup


def is_fused(points, new_points):
    return new_points in FUSED and new_points > points and new_points % points == 0


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


# an operation: ("interpolatei", function, rolloff, factor) | ("interpolate", function, rolloff, dest_points, delay) |
# ("interpft", dest_points) | ("decimatei", factor, delay)
def apply(obj, op):
    if op[0] == "interpolatei":
        return obj.interpolatei(op[1], op[3], op[2])
    if op[0] == "interpolate":
        return obj.interpolate(op[1], op[3], op[4], op[2])
    if op[0] == "interpft":
        return obj.interpft(op[1])
    return obj.decimatei(op[1], op[2])


def new_points(op, points):
    if op[0] == "interpolatei":
        return points * op[3]
    if op[0] == "interpolate":
        return op[3]
    if op[0] == "interpft":
        return op[1]
    return (points - op[2] + op[1] - 1) // op[1] if op[2] < points else 0


def oracle(xrow, cplx, op, delta):
    """the row in float64 through the oracle"""
    x = xrow.astype(np.float64)
    if op[0] == "interpolatei":
        code, ref = orc.interpolatei(x, cplx, op[1], op[2], op[3])
    elif op[0] == "interpolate":
        code, ref, _ = orc.interpolate(x, cplx, op[1], op[2], op[3], op[4], delta)
    elif op[0] == "interpft":
        code, ref, _ = orc.interpolate(x, cplx, -1, 0.0, op[1], 0.0, delta)
    else:
        return orc.decimatei(xrow, cplx, op[1], op[2])
    assert code == 0
    return ref


def expected_delta(op, points, delta, dtype):
    """interpolate / interpft: delta / (dest_points / points), computed in the matrix's precision; else untouched"""
    t = np.dtype(dtype).type
    if op[0] in ("interpolate", "interpft"):
        return t(delta) / (t(new_points(op, points)) / t(points))
    return t(delta)


def check_case(bd, rows, points, cplx, op, dtype, seed, against, delta=0.5, domain=0):
    """one batched call; sampled rows against the oracle or the vector path.  Returns the worst rel-L2 seen."""
    e = 2 if cplx else 1
    x = orc.fill_uniform(rows * points * e, seed, -10, 10, dtype).reshape(rows, points * e)
    m = bd.DspMat(x, is_complex=cplx, delta=delta, domain=domain)
    assert apply(m, op) == 0, (rows, points, cplx, op)
    npts = new_points(op, points)
    assert m.rows() == rows and m.row_points() == npts and m.row_len() == npts * e, (rows, points, cplx, op)
    assert m.is_complex() == cplx and m.domain() == domain
    assert m.delta() == expected_delta(op, points, delta, dtype), (m.delta(), op, points)
    got = m.data()
    rpw = rows_per_workgroup(npts) if is_fused(points, npts) else 0
    tol = tol_for(op, dtype) * (1 if against == "oracle" else 2)  # the vector path is held to the same tolerance
    worst = 0.0
    for r in sample_rows(rows, rpw):
        if against == "oracle":
            ref = oracle(x[r], cplx, op, delta)
        else:
            v = bd.DspVec(x[r], is_complex=cplx, delta=delta, domain=domain)
            assert apply(v, op) == 0
            assert (v.points(), len(v), v.is_complex(), v.domain()) == (m.row_points(), m.row_len(), m.is_complex(), m.domain())
            assert v.delta() == m.delta(), (v.delta(), m.delta(), op)
            ref = v.data()
        if op[0] == "decimatei":
            assert np.array_equal(got[r], ref), (rows, points, cplx, op, r)
            continue
        err = rel_l2(got[r], ref)
        worst = max(worst, err)
        assert err < tol, (against, rows, points, cplx, op, r, err, tol)
    return worst


def fused_shapes():
    """(rows, points, N): every fused N with the factors 2, 4, 8, 16 (p = N / f >= 1) at rows_per_workgroup + 1, 1 and
    1003 rows"""
    s = []
    for n in FUSED:
        for f in (2, 4, 8, 16):
            p = n // f
            if p >= 1:
                s += [(rows_per_workgroup(n) + 1, p, n), (1, p, n), (1003, p, n)]
    return s


def fused_ops(points, n):
    f = n // points
    return [("interpolatei", SINC, 0.0, f), ("interpolatei", RAISED_COSINE, 0.4, f),
            ("interpolate", SINC, 0.0, n, 0.3), ("interpolate", RAISED_COSINE, 0.4, n, 0.3), ("interpft", n)]


def general_cases():
    """(rows, points, [operations]) off the fused kernel"""
    def up(points, dest, delay=0.0):
        ops = [("interpolate", SINC, 0.0, dest, delay), ("interpolate", RAISED_COSINE, 0.4, dest, 0.3), ("interpft", dest)]
        if dest % points == 0 and dest > points:
            ops += [("interpolatei", SINC, 0.0, dest // points), ("interpolatei", RAISED_COSINE, 0.4, dest // points)]
        return ops
    return [(37, 6, up(6, 12)), (37, 7, up(7, 14)), (37, 6, up(6, 13)), (37, 13, up(13, 6)),
            (300, 1000, up(1000, 1500)),
            (300, 1000, [("interpolatei", SINC, 0.0, 3), ("interpolatei", RAISED_COSINE, 0.4, 3)]),
            (5, 4096, up(4096, 8192)), (3, 2048, up(2048, 1024)), (19, 512, up(512, 512, 0.3)),
            (3, 40000, up(40000, 65536)), (5, 4097, up(4097, 8193))]  # 4097 = 17 x 241, 8193 = 3 x 2731: Bluestein


@pytest.mark.parametrize("against", ("oracle", "vector"))
@pytest.mark.parametrize("cplx", (True, False))
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_rows(bd, dtype, cplx, against):
    worst = {}
    for k, (rows, points, n) in enumerate(fused_shapes()):
        assert is_fused(points, n)
        for j, op in enumerate(fused_ops(points, n)):
            # the vector comparison alternates the domain: neither path looks at it, both must keep it
            domain = (k + j) % 2 if against == "vector" else 0
            e = check_case(bd, rows, points, cplx, op, dtype, 1000 + 7 * k + j, against, domain=domain)
            worst[op[0]] = max(worst.get(op[0], 0.0), e)
    print("fused, worst rel-L2 to the %s (%s, %s): %s" % (
        against, np.dtype(dtype).name, "complex" if cplx else "real",
        ", ".join("%s %.3e" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("against", ("oracle", "vector"))
@pytest.mark.parametrize("cplx", (True, False))
@pytest.mark.parametrize("dtype", DTYPES)
def test_general_rows(bd, dtype, cplx, against):
    worst = {}
    for k, (rows, points, ops) in enumerate(general_cases()):
        for j, op in enumerate(ops):
            assert not is_fused(points, new_points(op, points))
            domain = (k + j) % 2 if against == "vector" else 0
            e = check_case(bd, rows, points, cplx, op, dtype, 5000 + 11 * k + j, against, domain=domain)
            worst[op[0]] = max(worst.get(op[0], 0.0), e)
    print("general, worst rel-L2 to the %s (%s, %s): %s" % (
        against, np.dtype(dtype).name, "complex" if cplx else "real",
        ", ".join("%s %.3e" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("against", ("oracle", "vector"))
def test_large_batches(bd, against):
    """f32 only: 16384 rows on the fused path (1024 -> 4096) and on the general path (1000 -> 2000)"""
    dtype, rows = np.float32, 16384
    cases = [(1024, True, ("interpft", 4096)), (1024, False, ("interpolatei", RAISED_COSINE, 0.4, 4)),
             (1024, True, ("interpolate", SINC, 0.0, 4096, 0.3)),
             (1000, True, ("interpolate", SINC, 0.0, 2000, 0.3)), (1000, False, ("interpft", 2000))]
    for k, (points, cplx, op) in enumerate(cases):
        e = check_case(bd, rows, points, cplx, op, dtype, 8000 + k, against)
        print("large batch %d -> %d (%s, %s), worst rel-L2 to the %s: %.3e" % (
            points, new_points(op, points), "complex" if cplx else "real", op[0], against, e))


@pytest.mark.parametrize("against", ("oracle", "vector"))
@pytest.mark.parametrize("cplx", (True, False))
@pytest.mark.parametrize("dtype", DTYPES)
def test_decimatei_rows(bd, dtype, cplx, against):
    for k, (rows, points) in enumerate(((1, 1001), (37, 1001), (1003, 64), (300, 4096), (3, 100000))):
        for j, (factor, delay) in enumerate(((2, 1), (3, 0), (7, 5), (4, 0), (1, 0), (2000, 3), (5, points - 1), (5, points), (2, points + 7))):
            check_case(bd, rows, points, cplx, ("decimatei", factor, delay), dtype, 9000 + 13 * k + j, against)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_isolation_and_determinism(bd, dtype):
    """changing one input row changes that output row and no other, bit for bit; equal inputs give equal bits"""
    cases = [(40, 256, True, ("interpolatei", SINC, 0.0, 4)), (40, 64, False, ("interpolate", RAISED_COSINE, 0.4, 128, 0.3)),
             (131, 32, True, ("interpft", 64)), (37, 100, True, ("interpolate", SINC, 0.0, 150, 0.3)),
             (37, 100, False, ("interpolatei", RAISED_COSINE, 0.4, 3)), (9, 5000, True, ("interpft", 8192)),
             (37, 150, False, ("interpft", 100)), (37, 100, True, ("decimatei", 3, 1))]
    for k, (rows, points, cplx, op) in enumerate(cases):
        e = 2 if cplx else 1
        x = orc.fill_uniform(rows * points * e, 300 + k, -10, 10, dtype).reshape(rows, points * e)
        outs = []
        for _ in range(2):
            m = bd.DspMat(x, is_complex=cplx)
            assert apply(m, op) == 0
            outs.append(m.data())
        assert np.array_equal(outs[0], outs[1]), (rows, points, cplx, op)
        for r0 in (0, rows // 2, rows - 1):
            y = x.copy()
            y[r0] = orc.fill_uniform(points * e, 900 + k, -10, 10, dtype)
            m = bd.DspMat(y, is_complex=cplx)
            assert apply(m, op) == 0
            got = m.data()
            others = np.arange(rows) != r0
            assert np.array_equal(got[others], outs[0][others]), (rows, points, cplx, op, r0)
            assert not np.array_equal(got[r0], outs[0][r0]), (rows, points, cplx, op, r0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_codes_and_state(bd, dtype):
    def same(m, x, cplx, delta=0.5, domain=0):
        return (np.array_equal(m.data(), x) and m.rows() == x.shape[0] and m.row_len() == x.shape[1] and
                m.is_complex() == cplx and m.delta() == delta and m.domain() == domain)

    for cplx in (True, False):
        x = orc.fill_uniform(3 * 16, 5, -10, 10, dtype).reshape(3, 16)
        # interpolatei with a factor <= 1: 0, bit-identical
        for factor in (1, 0, -3):
            m = bd.DspMat(x, is_complex=cplx, delta=0.5)
            assert m.interpolatei(SINC, factor) == 0 and same(m, x, cplx)
        # dest_points == 0: 7, untouched
        m = bd.DspMat(x, is_complex=cplx, delta=0.5)
        assert m.interpolate(SINC, 0) == 7 and same(m, x, cplx)
        assert m.interpolate(None, 0) == 7 and same(m, x, cplx)
        assert m.interpft(0) == 7 and same(m, x, cplx)
        # decimatei with factor 0: 7, untouched
        assert m.decimatei(0, 0) == 7 and same(m, x, cplx)
        v = bd.DspVec(x[0], is_complex=cplx)
        assert v.interpolate(SINC, 0) == 7 and v.interpft(0) == 7 and v.decimatei(0, 0) == 7 and v.interpolatei(SINC, 1) == 0
        # rows of zero points: 7 for interpolate / interpft, the matrix as it was
        m = bd.DspMat(is_complex=cplx, dtype=dtype, rows=3, row_len=0, delta=0.5)
        assert m.interpolate(SINC, 8) == 7 and m.interpft(8) == 7
        assert m.rows() == 3 and m.row_len() == 0 and m.delta() == 0.5 and m.is_complex() == cplx
        assert m.interpolatei(SINC, 2) == 0 and m.decimatei(2, 0) == 0 and m.rows() == 3 and m.row_len() == 0
        # zero rows: 0
        m = bd.DspMat(is_complex=cplx, dtype=dtype, rows=0, row_len=16, delta=0.5)
        assert m.interpolatei(SINC, 2) == 0 and m.interpolate(SINC, 64) == 0 and m.interpolate(None, 64) == 0
        assert m.interpft(64) == 0 and m.decimatei(2, 0) == 0
        assert m.rows() == 0 and m.delta() == 0.5
        # function=None is interpft
        a, b = bd.DspMat(x, is_complex=cplx), bd.DspMat(x, is_complex=cplx)
        assert a.interpolate(None, 40) == 0 and b.interpft(40) == 0 and np.array_equal(a.data(), b.data())
        # any non-zero function id is the raised cosine, as in the vector facade
        a, b = bd.DspMat(x, is_complex=cplx), bd.DspMat(x, is_complex=cplx)
        assert a.interpolatei(5, 2, 0.4) == 0 and b.interpolatei(RAISED_COSINE, 2, 0.4) == 0
        assert np.array_equal(a.data(), b.data())
        # a delay beyond the rows: empty rows, 0, like the vector
        m = bd.DspMat(x, is_complex=cplx)
        v = bd.DspVec(x[0], is_complex=cplx)
        assert m.decimatei(2, 100) == v.decimatei(2, 100) == 0
        assert m.rows() == 3 and m.row_len() == len(v) == 0

    # a matrix poisoned by wrap on complex data: -1 where the vector reports -1, and the vector's code everywhere
    x = orc.fill_uniform(3 * 16, 6, -10, 10, dtype).reshape(3, 16)
    for call in (lambda o: o.interpolatei(SINC, 2), lambda o: o.decimatei(2, 0), lambda o: o.interpolate(SINC, 32),
                 lambda o: o.interpft(32)):
        m = bd.DspMat(x, is_complex=True)
        v = bd.DspVec(x[0], is_complex=True)
        assert m.wrap(1.0) == -1 and v.wrap(1.0) == -1
        assert call(m) == call(v)
        assert m.row_len() == 0 and np.isnan(m.delta())
    m = bd.DspMat(x, is_complex=True)
    assert m.wrap(1.0) == -1 and m.interpolatei(SINC, 2) == -1 and m.decimatei(2, 0) == -1 and m.scale(2.0) == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_pulse_compression_then_interpft(bd, dtype):
    """correlate 1000-point rows with a chirp template into 2048 points, interpft(8192), magnitude, max_index: the fine
    peak is within one fine sample of four times the coarse peak and is the oracle's peak for the same correlation"""
    rows, n, l, fine = 257, 1000, 2048, 8192
    rng = np.random.default_rng(20240911)
    t = np.arange(64)
    chirp = np.exp(1j * np.pi * 0.9 * (t - 32.0) ** 2 / 64.0)
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
    assert m.correlate(arg) == 0 and m.row_points() == l
    corr = m.data()
    coarse = np.argmax(np.hypot(corr[:, 0::2], corr[:, 1::2]), axis=1)
    assert m.interpft(fine) == 0 and m.row_points() == fine and m.is_complex()
    assert m.delta() == np.dtype(dtype).type(1.0) / (np.dtype(dtype).type(fine) / np.dtype(dtype).type(l))
    assert m.magnitude() == 0 and not m.is_complex() and m.row_len() == fine
    got = m.statistics()["max_index"]
    assert np.all(np.abs(got - 4 * coarse) <= 1), np.nonzero(np.abs(got - 4 * coarse) > 1)[0][:10]
    want = np.empty(rows, np.int64)
    for r in range(rows):
        code, ref, _ = orc.interpolate(corr[r].astype(np.float64), True, -1, 0.0, fine, 0.0, 1.0)
        assert code == 0
        want[r] = np.argmax(np.hypot(ref[0::2], ref[1::2]))
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
