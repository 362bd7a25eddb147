"""A vector is a matrix of one row: DspVec's swap_halves / fft_shift / ifft_shift, zero_pad, reverse, mirror, cum_sum,
unwrap and *_smaller launch the matrix kernels with one row, so a matrix row compared with the vector call no longer
checks two implementations there (diff / diff_with_start and multiply_complex_exponential keep a vector kernel, which
measured faster for one long row).  This file holds the vector's independent references for all nine operations at the
shapes where a one-row launch of a row-carrying kernel can go wrong:
  * points 1, 2, 3, 255, 256, 257, 511, 512, 513: the lane groups of the short-row scan end at MS_SCAN_SHORT = 512, a
    workgroup's tile of the mixer at 256;
  * SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1: one workgroup per row ends and the three-step scan begins;
  * L + 1 and 2 L + 3, L = compute units x 8 x 256 = one grid stride of the flat kernels: above it a lane carries its
    (row, position) over a stride that is longer than the row, and the last lanes run one trip fewer.
Real and complex data, f32 and f64.  A vector owns its (aligned) device buffer, so the only offset the API allows is the
host array's: every upload comes from an address that is not 16-byte aligned.

References and bounds:
  * the movers against tests/vec_model.py (VecModel, index arithmetic only) and diff against oracle_lib: bit-equal;
  * unwrap (a sequential recurrence) and *_smaller (one rounding per operation) against oracle_lib: bit-equal, as in
    tests/test_gpu_parity.py; operand lengths 1, points / 3 (where 3 divides points) and points;
  * cum_sum with test_gpu_parity's bound: max |got - prefix sum| / (max |prefix sum| + 1) < 2e-7 (f32), 1e-13 (f64),
    and oracle_lib's sequential sum in T within its own error bound of that prefix sum;
  * multiply_complex_exponential with test_gpu_parity's bounds: rel-L2 < 2e-7 (f32), 1e-14 (f64) against the exact
    phasor exp(j (a k + b)) in double, and against oracle_lib's running product < 5e-5 (f32), 1e-11 (f64) for up to
    3000 points.  The running product's own error grows with the index (measured against the exact phasor on the CPU:
    1.6e-5 at 3000 points, 2.6e-3 at 524289, 5.3e-3 at 1048579 in f32; 2.6e-14, 4.4e-12, 8.7e-12 in f64 -- linear in
    the length), so above 3000 points that bound grows by points / 3000, which keeps test_gpu_parity's margin over the
    reference's own error.

The second batch: multiply_frequency_response (the packet map with OpFreqResp, which carries the position in the row) and
decimatei (k_rs_decimate_rows) launch with one row as well, and convolve_signal, *_smaller, multiply_frequency_response and
decimatei have ONE host function for vectors and matrices.  Windows, the FFT-domain resampling family, interpolate_lin /
interpolate_hermite, convolve(function) and the padding of correlate keep their vector kernels (one long row measured
slower through the row-aware kernel), so the matrix tests still compare two implementations there.
  * multiply_frequency_response: 1 .. 5 scalars (the tail below one 16-byte packet), lengths that make 1023, 1024 and 1025
    packets (k_map_inplace's chunk of 1024 packets) and one grid stride + 1; against oracle_lib with
    test_gpu_mat_basic's bounds: 1e-12 absolute in f64, 4 ulp of max |reference| in f32;
  * decimatei: 1, 2, 3, 127, 128, 129, 255, 256, 257 output points (rs_row_geometry narrows the workgroup below 256 columns
    and leaves blockDim.y > 1 with a single row), and one f32 real case of more than 65 535 x 256 outputs (the x dimension
    of the grid is not clamped); bit-equal to oracle_lib;
  * the merged host functions: poisoned input, wrong number space or domain, empty vector, with the codes of
    tests/test_gpu_vec_sequences.py's tables.
"""
import numpy as np
import pytest

import oracle_lib as orc
from vec_model import PAD_CENTER, PAD_END, PAD_SURROUND, VecModel

pytestmark = pytest.mark.gpu

bd = pytest.importorskip("basic_dsp_amd")
from basic_dsp_amd import DspVec  # noqa: E402
from basic_dsp_amd import vector as V  # noqa: E402

MS_SCAN_SHORT = 512    # mat_scan.hip
SCAN_CHUNK = 4096      # mat_scan_core.h
FLAT_WG, FLAT_WG_PER_CU = 256, 8   # mf_grid / mw_grid / sy_grid: at most 8 workgroups of 256 lanes per compute unit


def _shapes():
    cus = bd.lib.bdsp_hip_compute_units()
    assert cus > 0, bd.last_error()
    stride = cus * FLAT_WG_PER_CU * FLAT_WG
    return [1, 2, 3, 255, 256, 257, MS_SCAN_SHORT - 1, MS_SCAN_SHORT, MS_SCAN_SHORT + 1, SCAN_CHUNK - 1, SCAN_CHUNK,
            SCAN_CHUNK + 1, stride + 1, 2 * stride + 3]


_CACHE = {}


def unaligned(a):
    """a copy of `a` whose first byte is not 16-byte aligned (one scalar into a fresh buffer)"""
    a = np.asarray(a)
    buf = np.empty(a.size + 5, a.dtype)
    start = next(k for k in range(1, 5) if (buf.ctypes.data + k * a.itemsize) % 16)
    out = buf[start:start + a.size]
    out[:] = a
    assert out.ctypes.data % 16 != 0
    return out


def signal(points, cplx, dtype, seed=0):
    """the shared, read-only input of one (points, number space, precision): computed once"""
    key = (points, cplx, np.dtype(dtype).name, seed)
    if key not in _CACHE:
        x = unaligned(orc.fill_uniform(points * (2 if cplx else 1), 20261019 + 7 * seed + points % 1000, -10, 10, dtype))
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(bits(got), bits(ref))


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300)


CASES = [(c, d) for c in (False, True) for d in (np.float32, np.float64)]
IDS = ["%s-%s" % ("complex" if c else "real", np.dtype(d).name) for c, d in CASES]


@pytest.fixture(scope="module")
def shapes():
    bd.require_gpu()
    return _shapes()


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_movers_bit_equal_to_the_model(shapes, cplx, dtype):
    """swap_halves, fft_shift, ifft_shift, reverse, zero_pad (End, Surround, Center; to one point more and to 2 p + 3)
    and mirror: code, length and every bit as VecModel's gather"""
    for p in shapes:
        x = signal(p, cplx, dtype)
        steps = [("swap_halves", ()), ("fft_shift", ()), ("ifft_shift", ()), ("reverse", ())]
        steps += [("zero_pad", (q, o)) for q in (p + 1, 2 * p + 3) for o in (PAD_END, PAD_SURROUND, PAD_CENTER)]
        if cplx:
            steps.append(("mirror", ()))
        for name, args in steps:
            v = DspVec(x, is_complex=cplx, domain=V.FREQ)
            m = VecModel(x, is_complex=cplx, domain=V.FREQ)
            assert getattr(v, name)(*args) == getattr(m, name)(*args) == 0, (name, args, p)
            assert len(v) == len(m) and v.is_complex() == m.is_complex(), (name, args, p)
            assert same_bits(v.data(), m.data()), (name, args, p)
        # two movers in a row: the second reads what the first left in the trade buffer
        v, m = DspVec(x, is_complex=cplx), VecModel(x, is_complex=cplx)
        assert v.reverse() == m.reverse() == 0 and v.ifft_shift() == m.ifft_shift() == 0
        assert same_bits(v.data(), m.data()), p


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_diff_bit_equal_to_the_oracle(shapes, cplx, dtype):
    e = 2 if cplx else 1
    for p in shapes:
        x = signal(p, cplx, dtype)
        for with_start in (False, True):
            v = DspVec(x, is_complex=cplx)
            assert (v.diff_with_start() if with_start else v.diff()) == 0
            ref = orc.diff(np.array(x), cplx, with_start)
            assert len(v) == ref.size == (p if with_start else p - 1) * e, (p, with_start)
            assert same_bits(v.data(), ref), (p, with_start)


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_cum_sum_against_the_prefix_sum(shapes, cplx, dtype):
    e = 2 if cplx else 1
    for p in shapes:
        x = signal(p, cplx, dtype)
        v = DspVec(x, is_complex=cplx)
        assert v.cum_sum() == 0 and len(v) == p * e
        # the prefix sum in extended precision: at 10^6 points a sequential f64 sum's own error is no longer far below 1e-13
        ref = np.cumsum(x.astype(np.longdouble).reshape(-1, e), axis=0).reshape(-1)
        scale = np.max(np.abs(ref)) + 1.0
        err = np.max(np.abs(v.data() - ref)) / scale
        assert err < (2e-7 if dtype == np.float32 else 1e-13), (p, err)
        seq = orc.cum_sum(np.array(x), cplx)
        assert np.max(np.abs(seq - ref)) / scale < (p * 1e-7 if dtype == np.float32 else p * 1e-16), p


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_unwrap_bit_equal_to_the_oracle(shapes, dtype):
    """a phase ramp wrapped into (-pi, pi] (every tile carries the previous tile's unwrapped end) and random data with
    a divisor that makes most steps take the remainder; a complex vector is poisoned"""
    for p in shapes:
        ramp = unaligned(np.angle(np.exp(1j * np.arange(p, dtype=np.float64) * 0.37)).astype(dtype))
        for data, div in ((ramp, 2 * np.pi), (signal(p, False, dtype, seed=1), 7.0)):
            v = DspVec(data)
            assert v.unwrap(dtype(div)) == 0 and len(v) == p
            assert same_bits(v.data(), orc.unwrap(np.array(data), dtype(div))), (p, div)
    c = DspVec(signal(3, True, dtype), is_complex=True)
    assert c.unwrap(dtype(1.0)) == -1 and c.is_erroneous()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_multiply_complex_exponential_against_the_exact_phasor_and_the_oracle(shapes, dtype):
    for p in shapes:
        x = signal(p, True, dtype)
        v = DspVec(x, is_complex=True, delta=0.5)
        assert v.multiply_complex_exponential(0.02, 0.3) == 0 and len(v) == 2 * p
        got = v.data()
        # a and b are multiplied by delta in T first (complex_ops.rs:83-84)
        a, b = float(dtype(0.02) * dtype(0.5)), float(dtype(0.3) * dtype(0.5))
        exact = x.astype(np.float64).view(np.complex128) * np.exp(1j * (a * np.arange(p) + b))
        err = rel_l2(got, exact.view(np.float64))
        assert err < (2e-7 if dtype == np.float32 else 1e-14), (p, err)
        running = orc.multiply_complex_exponential(np.array(x), 0.02, 0.3, 0.5)
        err = rel_l2(got, running)
        assert err < (5e-5 if dtype == np.float32 else 1e-11) * max(1.0, p / 3000.0), (p, err)
    r = DspVec(signal(3, False, dtype))
    assert r.multiply_complex_exponential(0.02, 0.3) == -1 and r.is_erroneous()


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_smaller_bit_equal_to_the_oracle(shapes, cplx, dtype):
    """operand lengths 1, points / 3 and points; an operand whose length does not divide the vector's: code 7"""
    e = 2 if cplx else 1
    for p in shapes:
        x = signal(p, cplx, dtype)
        for yp in sorted({1, p // 3 if p % 3 == 0 else p, p}):
            y = unaligned(orc.fill_uniform(yp * e, 77 + yp % 1000, 1, 10, dtype))
            tiled = np.tile(y.reshape(yp, e), (p // yp, 1)).reshape(-1)
            for op, name in enumerate(("add_smaller", "sub_smaller", "mul_smaller", "div_smaller")):
                v = DspVec(x, is_complex=cplx)
                assert getattr(v, name)(DspVec(y, is_complex=cplx)) == 0, (p, yp, name)
                code, ref = orc.binary(np.array(x), tiled, cplx, op)
                assert code == 0 and len(v) == p * e
                assert same_bits(v.data(), ref), (p, yp, name)
        if p > 2:
            v = DspVec(x, is_complex=cplx)
            assert v.add_smaller(DspVec(np.ones((p - 1) * e, dtype), is_complex=cplx)) == 7
            assert same_bits(v.data(), np.array(x)), p


# ---------------------------------------------------------------------------------------------- second batch
EW_CHUNK = 1024   # ew_map.h: packets of 16 bytes per workgroup chunk
MFR_RATIO, MFR_ROLLOFF = 1.7, 0.35   # tests/test_gpu_mat_basic.py


def _packet_points(cplx, dtype, stride):
    """points whose scalars are 1 .. 5 (complex: 2 and 4), 1023 / 1024 / 1025 packets of 16 bytes, and one grid stride + 1"""
    e, per_packet = (2 if cplx else 1), 16 // np.dtype(dtype).itemsize
    small = [n // e for n in range(1, 6) if n % e == 0]
    return small + [k * per_packet // e for k in (EW_CHUNK - 1, EW_CHUNK, EW_CHUNK + 1)] + [stride + 1]


def _close_where_finite(got, ref, dtype, what):
    """test_gpu_mat_basic's bounds for multiply_frequency_response; one point has no axis (0 / 0): NaN where the oracle's is"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    if nan.all():
        return
    g, r = got[~nan].astype(np.float64), ref[~nan].astype(np.float64)
    if dtype == np.float64:
        assert np.max(np.abs(g - r)) <= 1e-12, (what, np.max(np.abs(g - r)))
    else:
        top = np.max(np.abs(r))
        ulp = float(np.spacing(np.float32(top if top > 0 else 1.0)))
        assert np.max(np.abs(g - r)) <= 4.0 * ulp, (what, np.max(np.abs(g - r)) / ulp)


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_multiply_frequency_response_against_the_oracle(shapes, cplx, dtype):
    e = 2 if cplx else 1
    stride = shapes[-2] - 1
    for p in _packet_points(cplx, dtype, stride):
        x = unaligned(orc.fill_uniform(p * e, 6000 + p % 1000, -1, 1, dtype))
        for fid in (V.CONV_SINC, V.CONV_RAISED_COSINE):
            v = DspVec(x, is_complex=cplx, domain=V.FREQ, delta=0.25)
            assert v.multiply_frequency_response(fid, MFR_RATIO, MFR_ROLLOFF) == 0, (p, fid)
            assert len(v) == p * e and v.is_complex() == cplx and v.domain() == V.FREQ and v.delta() == 0.25
            with np.errstate(all="ignore"):
                ref = orc.multiply_frequency_response(np.array(x), cplx, fid, MFR_ROLLOFF, MFR_RATIO, False)
            _close_where_finite(v.data(), ref, dtype, (p, fid))


DECIMATE_OUT = (1, 2, 3, 127, 128, 129, 255, 256, 257)


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_decimatei_bit_equal_to_the_oracle(cplx, dtype):
    bd.require_gpu()
    e = 2 if cplx else 1
    for out in DECIMATE_OUT:
        for factor, delay in ((3, 2), (2, 0), (1, 1)):
            for p in (delay + (out - 1) * factor + 1, delay + out * factor):   # the shortest and the longest vector with `out` outputs
                x = signal(p, cplx, dtype, seed=2)
                v = DspVec(x, is_complex=cplx)
                assert v.decimatei(factor, delay) == 0, (p, factor, delay)
                ref = orc.decimatei(np.array(x), cplx, factor, delay)
                assert len(v) == ref.size == out * e, (p, factor, delay)
                assert same_bits(v.data(), ref), (p, factor, delay)
    # a delay at or past the end leaves an empty vector
    v = DspVec(signal(5, cplx, dtype, seed=2), is_complex=cplx)
    assert v.decimatei(2, 5) == 0 and len(v) == 0 and not v.is_erroneous()


def test_decimatei_with_more_outputs_than_65535_workgroups_of_256():
    bd.require_gpu()
    out = 65535 * 256 + 257
    x = np.resize(signal(1 << 20, False, np.float32, seed=3), 2 * out + 1)
    v = DspVec(x)
    assert v.decimatei(2, 1) == 0 and len(v) == out
    assert same_bits(v.data(), x[1::2])
    assert same_bits(x[1::2][:4099], orc.decimatei(np.array(x[:8199]), False, 2, 1))   # (the slice is what the oracle computes)


@pytest.mark.parametrize("cplx,dtype", CASES, ids=IDS)
def test_codes_of_the_merged_host_functions(cplx, dtype):
    """op_convolve_signal, op_binary_smaller, op_multiply_frequency_response and op_decimatei serve vectors and matrices: a
    poisoned vector, the wrong number space or domain and an empty vector, with the codes of tests/test_gpu_vec_sequences.py
    (_arg_errors, _poisoners, the unrelated calls on a poisoned vector) and tests/test_gpu_mat_basic.py (convolve_signal on
    a poisoned or empty matrix)"""
    bd.require_gpu()
    e = 2 if cplx else 1
    x13 = signal(13, cplx, dtype, seed=4)
    x = x13[:12 * e]

    def mk(n=12, c=cplx, domain=V.TIME):
        return DspVec(np.array(x13[:n * e] if c == cplx else np.ones(n * (2 if c else 1), dtype)), is_complex=c, domain=domain)

    def poisoned():
        v = mk()
        assert (v.to_complex() if cplx else v.conj()) == -1 and v.is_erroneous()
        return v

    def untouched(v, domain=V.TIME):
        return len(v) == 12 * e and v.domain() == domain and same_bits(v.data(), np.array(x))

    # convolve_signal: 2 number space, 2 domain, 5 both in the frequency domain, 7 filter longer than the vector
    for bad, code in ((mk(6, not cplx), 2), (mk(6, cplx, V.FREQ), 2), (mk(13), 7)):
        v = mk()
        assert v.convolve_signal(bad) == code and untouched(v), code
    v = mk(domain=V.FREQ)
    assert v.convolve_signal(mk(6, cplx, V.FREQ)) == 5 and untouched(v, V.FREQ)
    v = mk()
    assert v.convolve_signal(mk(0)) == 0 and untouched(v)            # an empty filter leaves the vector alone
    assert mk(0).convolve_signal(mk(0)) == 0 and mk(0).convolve_signal(mk(3)) == 7
    assert poisoned().convolve_signal(mk(0)) == -1 and poisoned().convolve_signal(mk(3)) == 7   # an argument error comes first
    # *_smaller: 7 empty operand or a length that does not divide, 2 domain
    for name in ("add_smaller", "sub_smaller", "mul_smaller", "div_smaller"):
        for bad, code in ((mk(0), 7), (mk(5), 7), (mk(6, cplx, V.FREQ), 2)):
            v = mk()
            assert getattr(v, name)(bad) == code and untouched(v), (name, code)
        assert getattr(mk(0), name)(mk(3)) == 0 and getattr(poisoned(), name)(mk(3)) == -1, name
    # multiply_frequency_response: a time-domain vector is poisoned; empty and poisoned vectors
    v = mk()
    assert v.multiply_frequency_response(V.CONV_SINC, 0.5) == -1 and v.is_erroneous()
    v = mk(0, cplx, V.FREQ)
    assert v.multiply_frequency_response(V.CONV_SINC, 0.5) == 0 and len(v) == 0 and not v.is_erroneous()
    assert poisoned().multiply_frequency_response(V.CONV_RAISED_COSINE, 0.5, 0.35) == -1
    # decimatei: 7 by 0; empty and poisoned vectors
    v = mk()
    assert v.decimatei(0, 0) == 7 and untouched(v)
    v = mk(0)
    assert v.decimatei(2, 0) == 0 and len(v) == 0 and not v.is_erroneous()
    v = poisoned()
    assert v.decimatei(2, 0) == -1 and v.is_erroneous() and v.decimatei(0, 0) == 7
