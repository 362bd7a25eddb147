"""DspMat.interpolatef as one launch over all rows, and with one delay per row.

Row r of the batched call must be, bit for bit, what DspVec.interpolatef gives on row r alone (with delay[r] where the
delays are per row): the matrix kernels instantiate the vector kernels' bodies, the plan of one row picks the path and
the kernel for all of them, and wrap-around never leaves a row.  The shapes are the smallest that reach every kernel and
branch of interp.hip (points per row; L = conv_len):

  blocked inner kernel  factor 4, L 8, real rows of 501 points (new_len 2004 >= 2000, rows on 4-byte boundaries, one
                        partial tile) and of 1300 points (more than one tile at every QB); factors 2, 3, 8 at 1300
                        points; complex rows of 251 points (new_len 2008)
  table path            factor 5, L 8, real rows of 401 points (new_len 2005 -> 2006); factor 6; factor 8, L 100, rows of
                        260 points (new_points < 2 ntaps f: every output is an edge)
  scalar path, integer  factor 2, rows of 37 points (new_len < 2000), L 8 and L 30 (clipped to 18)
  fractional path       factors 1.5, 13/6, 0.5, 48/44.1 with sinc and with the raised cosine at roll-off 0.35, L 20, on rows
                        of 300 points; L 70 (141 taps > 127: k_interp_scalar_v2)

Beside the bit comparison every finite row is held to the CPU oracle with the tolerance of the existing matrix test
(e_interpolatef in test_gpu_mat_sequences.py): rel-L2 2e-6 (f32) / 1e-12 (f64) per row; integer factors against the
float64 oracle, fractional ones against the oracle in T with exact weights."""
import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

SINC, RC = 0, 1
DTYPES = (np.float32, np.float64)
F48 = 48.0 / 44.1


@pytest.fixture(scope="module")
def bd():
    import basic_dsp_amd as b
    b.require_gpu()
    return b


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rows_data(rows, points, cplx, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (rows, points * (2 if cplx else 1))).astype(dtype)


def vec_result(bd, row, cplx, delta, fid, factor, delay, conv_len, rolloff):
    v = bd.DspVec(row, is_complex=cplx, delta=delta)
    assert v.interpolatef(fid, factor, delay, conv_len, rolloff) == 0
    return v.data()


def oracle_row(row, cplx, dtype, fid, rolloff, factor, delay, conv_len, delta):
    if factor == int(factor):
        return orc.interpolatef(row.astype(np.float64), cplx, fid, rolloff, factor, delay, conv_len, delta)[0]
    with orc.exact_weights():
        return orc.interpolatef(row, cplx, fid, rolloff, dtype(factor), dtype(delay), conv_len, dtype(delta))[0]


def rel_l2(got, ref):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


# (label, points, complex, function, roll-off, factor, conv_len)
SHAPES = [
    ("blocked f4 501", 501, False, SINC, 0.0, 4.0, 8),
    ("blocked f4 1300", 1300, False, SINC, 0.0, 4.0, 8),
    ("blocked f2 1300", 1300, False, SINC, 0.0, 2.0, 8),
    ("blocked f3 1300", 1300, False, SINC, 0.0, 3.0, 8),
    ("blocked f8 1300", 1300, False, SINC, 0.0, 8.0, 8),
    ("blocked f4 complex 251", 251, True, SINC, 0.0, 4.0, 8),
    ("blocked f2 complex 1300", 1300, True, RC, 0.35, 2.0, 8),
    ("table f5 401", 401, False, SINC, 0.0, 5.0, 8),
    ("table f5 complex 401", 401, True, SINC, 0.0, 5.0, 8),
    ("table f6 401", 401, False, RC, 0.35, 6.0, 8),
    ("table f8 L100 260 all edges", 260, False, SINC, 0.0, 8.0, 100),
    ("scalar f2 37 L8", 37, False, SINC, 0.0, 2.0, 8),
    ("scalar f2 37 L30 clipped", 37, False, SINC, 0.0, 2.0, 30),
    ("scalar f2 complex 37 L8", 37, True, RC, 0.35, 2.0, 8),
    ("frac 1.5 sinc", 300, False, SINC, 0.0, 1.5, 20),
    ("frac 13/6 sinc complex", 300, True, SINC, 0.0, 13.0 / 6.0, 20),
    ("frac 0.5 sinc", 300, False, SINC, 0.0, 0.5, 20),
    ("frac 48/44.1 sinc", 300, False, SINC, 0.0, F48, 20),
    ("frac 1.5 rc", 300, True, RC, 0.35, 1.5, 20),
    ("frac 13/6 rc", 300, False, RC, 0.35, 13.0 / 6.0, 20),
    ("frac 0.5 rc complex", 300, True, RC, 0.35, 0.5, 20),
    ("frac 48/44.1 rc", 300, False, RC, 0.35, F48, 20),
    ("frac 48/44.1 rc complex", 300, True, RC, 0.35, F48, 20),
    ("frac 1.5 rc L70 v2", 300, False, RC, 0.35, 1.5, 70),
    ("frac 1.5 sinc L70 v2 complex", 300, True, SINC, 0.0, 1.5, 70),
]
IDS = [s[0].replace(" ", "_") for s in SHAPES]


def check_shared(bd, dtype, shape, delay, delta, seed):
    _, points, cplx, fid, rolloff, factor, conv_len = shape
    tol = 2e-6 if dtype == np.float32 else 1e-12
    new_len = orc.interpolatef_new_len(points * (2 if cplx else 1), dtype(factor), dtype)
    for rows, nan_rows in ((1, ()), (3, ()), (5, (1, 3))):
        x = rows_data(rows, points, cplx, dtype, seed + rows)
        for r in nan_rows:
            x[r] = np.nan  # a read across a row boundary poisons a finite row
        m = bd.DspMat(x, is_complex=cplx, delta=delta)
        assert m.interpolatef(fid, factor, delay, conv_len, rolloff) == 0
        assert m.rows() == rows and m.row_len() == new_len and m.delta() == delta
        got = m.data()
        for r in range(rows):
            if r in nan_rows:
                continue
            ref = vec_result(bd, x[r], cplx, delta, fid, factor, delay, conv_len, rolloff)
            assert np.all(np.isfinite(got[r])), (shape[0], rows, r)
            assert same_bits(got[r], ref), (shape[0], rows, r, int(np.sum(bits(got[r]) != bits(ref))))
            err = rel_l2(got[r], oracle_row(x[r], cplx, dtype, fid, rolloff, factor, delay, conv_len, delta))
            print("%s rows %d row %d: rel-L2 %.3e (bound %.1e)" % (shape[0], rows, r, err, tol))
            assert err < tol, (shape[0], rows, r, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_equal_the_vector_call_with_a_shared_delay(bd, dtype, shape):
    check_shared(bd, dtype, shape, 0.0, 1.0, 100)


META = [SHAPES[i] for i in (0, 5, 7, 11, 21, 23)]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("delta", (1.0, 0.5))
@pytest.mark.parametrize("shape", META, ids=[s[0].replace(" ", "_") for s in META])
def test_shared_delay_is_divided_by_delta_and_delta_stays(bd, dtype, delta, shape):
    check_shared(bd, dtype, shape, 0.3, delta, 200)


# ---------------------------------------------------------------------------------------------- per-row delays
DELAYS = [0.0, 0.25, -0.4, 1.0, 0.5]
ROW_SHAPES = [SHAPES[0], SHAPES[5], SHAPES[7], SHAPES[8], SHAPES[11], SHAPES[13], SHAPES[21], SHAPES[22]]
ROW_IDS = [s[0].replace(" ", "_") for s in ROW_SHAPES]


def slow_pairs(conv_len, delay, fid, rolloff):
    """frac_slow_pairs of interp.hip: the pairs of taps that can hold j == 0 or a tap near the raised cosine's second
    singularity, for tap k's j in [k - L - 1 + delay, k - L + delay]"""
    ntaps = 2 * conv_len + 1
    beta = abs(rolloff)
    mask = 0
    for k in range(ntaps - 1):
        jlo, jhi = k - conv_len - 1.0 + delay, k - conv_len + delay
        mg = 1e-3 * (1.0 + (-jlo if jhi < 0 else jhi))
        hits = lambda a, b: jlo - mg < b and jhi + mg > a
        special = hits(-0.5, 0.5)
        if fid != 0 and beta > 0:
            lo, hi = 0.375 / beta, 0.625 / beta
            special = special or hits(lo, hi) or hits(-hi, -lo)
        if special:
            mask |= 1 << (k >> 1)
    return mask


def test_the_fractional_case_has_rows_with_different_slow_pair_masks():
    for delta in (1.0, 0.5):
        masks = {slow_pairs(20, d / delta, RC, 0.35) for d in DELAYS}
        assert len(masks) > 1, masks


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("delta", (1.0, 0.5))
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=ROW_IDS)
def test_row_r_equals_the_vector_call_with_its_own_delay(bd, dtype, delta, shape):
    _, points, cplx, fid, rolloff, factor, conv_len = shape
    x = rows_data(5, points, cplx, dtype, 300)
    refs = [vec_result(bd, x[r], cplx, delta, fid, factor, DELAYS[r], conv_len, rolloff) for r in range(5)]
    assert not same_bits(refs[1], vec_result(bd, x[1], cplx, delta, fid, factor, DELAYS[2], conv_len, rolloff))
    for delays in (list(DELAYS), np.array(DELAYS, np.float64), np.array(DELAYS, dtype)):
        m = bd.DspMat(x, is_complex=cplx, delta=delta)
        assert m.interpolatef(fid, factor, delays, conv_len, rolloff) == 0
        assert m.rows() == 5 and m.row_len() == refs[0].size and m.delta() == delta
        got = m.data()
        for r in range(5):
            assert same_bits(got[r], refs[r]), (shape[0], r, int(np.sum(bits(got[r]) != bits(refs[r]))))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=ROW_IDS)
def test_equal_delays_give_the_bits_of_the_scalar_call(bd, dtype, shape):
    _, points, cplx, fid, rolloff, factor, conv_len = shape
    x = rows_data(3, points, cplx, dtype, 400)
    a, b = bd.DspMat(x, is_complex=cplx, delta=0.5), bd.DspMat(x, is_complex=cplx, delta=0.5)
    assert a.interpolatef(fid, factor, 0.3, conv_len, rolloff) == 0
    assert b.interpolatef(fid, factor, [0.3, 0.3, 0.3], conv_len, rolloff) == 0
    assert same_bits(a.data(), b.data())


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_delay_count_poison_and_empty(bd, dtype):
    x = rows_data(5, 501, False, dtype, 500)
    m = bd.DspMat(x)
    before = m.data()
    for n in (4, 6):
        assert m.interpolatef(SINC, 4.0, [0.1] * n, 8) == 7
        assert m.rows() == 5 and m.row_len() == 501 and same_bits(m.data(), before)
    p = bd.DspMat(x)
    assert p.conj() == -1  # real rows: poisoned
    assert p.interpolatef(SINC, 4.0, [0.1] * p.rows(), 8) == -1
    assert p.interpolatef(SINC, 4.0, [0.1] * (p.rows() + 1), 8) == 7  # the argument check comes first
    e = bd.DspMat(rows=0, row_len=0, dtype=dtype)
    assert e.interpolatef(SINC, 4.0, np.zeros(0, dtype), 8) == 0 and e.rows() == 0
    z = bd.DspMat(rows=3, row_len=0, dtype=dtype)
    assert z.interpolatef(SINC, 4.0, [0.0, 0.1, 0.2], 8) == 0 and z.rows() == 3 and z.row_len() == 0


# ---------------------------------------------------------------------------------------------- many rows, repeatability
def test_more_rows_than_a_grid_dimension_on_the_integer_path(bd):
    rows, points = 66000, 500
    x = rows_data(rows, points, False, np.float32, 600)
    m = bd.DspMat(x)
    assert m.interpolatef(SINC, 4.0, 0.0, 8) == 0
    assert m.rows() == rows and m.row_len() == 2000
    for r in (0, 1, 65535, 65536, 65999):
        ref = vec_result(bd, x[r], False, 1.0, SINC, 4.0, 0.0, 8, 0.0)
        assert same_bits(m.get_row(r).data(), ref), r


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[7], SHAPES[22]], ids=("blocked", "table", "fractional"))
def test_the_same_call_twice_gives_the_same_bits(bd, dtype, shape):
    """(the second call finds the shared delay's tap table in the cache)"""
    _, points, cplx, fid, rolloff, factor, conv_len = shape
    x = rows_data(3, points, cplx, dtype, 700)
    out = []
    for delay in (0.125, 0.125, [0.125, 0.5, -0.25], [0.125, 0.5, -0.25]):
        m = bd.DspMat(x, is_complex=cplx)
        assert m.interpolatef(fid, factor, delay, conv_len, rolloff) == 0
        out.append(m.data())
    assert same_bits(out[0], out[1]) and same_bits(out[2], out[3])
    assert same_bits(out[0][0], out[2][0]) and not same_bits(out[0][1], out[2][1])
