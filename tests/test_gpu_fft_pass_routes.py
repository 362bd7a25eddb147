"""Every route of the global passes of a power-of-two transform above 4096 points, on the device.

tests/fft_pass_shapes.txt states, for 434 transforms, which k_fft_pass instantiations run (the rule is
basic_dsp_amd/csrc/fft_plan_core.h; tests/test_fft_plan_abi.py holds the table to it and shows that the table reaches every
instantiation the rule can choose).  Each line is run here through the entry it names -- DspVec, DspMat, bdsp_hip_dev_fft
or convolve_signal with a filter long enough for the strided first pass -- on uniform data in [-10, 10), and compared with
numpy's float64 transform of the float64 copy of the same data, windowed / shifted / reduced to magnitudes by the oracle.

Tolerances are the suite's own: rel-L2 1e-6 (f32) / 1e-12 (f64) for one transform (BASELINE.json north_star);
windowed_ifft as test_every_reference_window_fused_into_the_first_global_pass treats it (central half for the triangular
and Blackman-Harris windows, all but the first and last 1/64 otherwise, four times the tolerance); convolve_signal as
test_convolve_signal_long_filters (2e-6 / 1e-11).  Every row of a batch is compared, and is bit-equal to the same row
run alone wherever the table gives both the same route.

Worst rel-L2 over all lines on an MI355X (printed by test_worst_errors_are_recorded): one transform f32 3.63e-7, f64
7.17e-16 (both at 2^23 points); windowed_ifft f32 5.89e-7, f64 7.38e-16; convolve_signal f32 5.57e-7, f64 1.36e-15."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import basic_dsp_amd as bd
import oracle_lib as orc
from basic_dsp_amd import DspMat, DspVec
from basic_dsp_amd import vector as V

pytestmark = pytest.mark.gpu

SHAPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fft_pass_shapes.txt")
WINDOWS = {"triangular": (V.WINDOW_TRIANGULAR, 0, 0.0), "hamming": (V.WINDOW_HAMMING, 1, 0.54), "hann": (V.WINDOW_HANN, 1, 0.5),
           "blackman_harris": (V.WINDOW_BLACKMAN_HARRIS, 2, 0.0), "rectangular": (V.WINDOW_RECTANGULAR, 3, 0.0)}
FACADE_WINDOW = {0: (0, 0.0), 1: (1, 0.54), 2: (2, 0.0), 3: (3, 0.0), 4: (1, 0.5)}  # facade id -> oracle id, alpha
WORST = {}  # (dtype name, kind) -> (rel-L2, line)


def read_lines():
    out = []
    for line in open(SHAPES):
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        cu = w[-1] == "cu256"
        rest = w[6:-1] if cu else w[6:]
        out.append((w[0], int(w[1]), int(w[2]), w[3], w[4], " ".join(rest[:-1]), cu))
    return out


LINES = read_lines()
ROUTE = {(d, b, n, e, o): r for d, b, n, e, o, r, _ in LINES}


def rel_l2(got, ref):
    got = np.asarray(got, np.float64).ravel()
    ref = np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def record(dtype, kind, err, line):
    key = (np.dtype(dtype).name, kind)
    if key not in WORST or err > WORST[key][0]:
        WORST[key] = (err, " ".join(str(v) for v in line[:5]))


class Case:
    """The data of one (dtype, bits, batch) and its float64 transforms, computed once and shared by the operations."""

    def __init__(self, dtype, bits, batch):
        self.dtype, self.n, self.batch = dtype, 1 << bits, batch
        self.x = orc.fill_uniform(2 * self.n * batch, 20260000 + 64 * bits + batch, -10, 10, dtype).reshape(batch, 2 * self.n)
        self.x64 = self.x.astype(np.float64)
        self._memo = {}

    def _get(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def z(self):  # complex view of the float64 copy, [batch, n]
        return self.x64.view(np.complex128)

    def fwd(self):
        return self._get("fwd", lambda: np.fft.fft(self.z(), axis=1))

    def inv(self):  # unnormalised
        return self._get("inv", lambda: np.fft.ifft(self.z(), axis=1) * self.n)

    def real_rows(self):  # a real vector per row: the first n scalars of the row
        return self.x[:, :self.n]

    def real_fwd(self):
        return self._get("rfwd", lambda: np.fft.fft(self.real_rows().astype(np.float64), axis=1))


@functools.lru_cache(maxsize=2)
def case(dtype, bits, batch):
    return Case(dtype, bits, batch)


def flat(zrows):  # complex128 [rows, n] -> interleaved float64 [rows, 2 n]
    return np.ascontiguousarray(zrows).view(np.float64)


def shifted(zrows, forward=True):  # fft_shift (forward) / ifft_shift of every row, by the oracle
    return np.stack([orc.swap_halves(r, True, forward) for r in flat(zrows)]).view(np.complex128)


def windowed(rows, is_complex, oid, alpha, unapply=False):  # float64 rows
    return np.stack([orc.apply_window(np.ascontiguousarray(r), is_complex, oid, alpha, unapply=unapply) for r in rows])


def custom_window(i, n):
    return 1.0 + i / n


def custom_table(n):
    i = np.arange(n, dtype=np.float64)
    w = 1.0 + i / n
    half = n - n // 2
    w[half:] = w[:n - half][::-1]  # is_symmetric: h[i] = h[n - 1 - i] for the second half (op_custom_window)
    return w


def reference(c, op):
    """-> (float64 reference rows, is the input real, domain, kind of tolerance, cut) for a facade operation."""
    name, _, arg = op.partition(":")
    real = name.startswith("real_")
    if real:
        name = name[5:]
    n = c.n
    src = c.real_rows().astype(np.float64) if real else c.x64
    zin = (src + 0j) if real else c.z()
    if name == "plain_fft":
        return flat(c.real_fwd() if real else c.fwd()), real, V.TIME, "one", 0
    if name == "fft":
        return flat(shifted(c.real_fwd() if real else c.fwd())), real, V.TIME, "one", 0
    if name == "windowed_fft":
        _, oid, alpha = WINDOWS[arg]
        w = windowed(src, not real, oid, alpha)
        zw = (w + 0j) if real else w.view(np.complex128)
        return flat(shifted(np.fft.fft(zw, axis=1))), real, V.TIME, "one", 0
    if name == "windowed_custom_fft":
        return flat(shifted(np.fft.fft(zin * custom_table(n), axis=1))), real, V.TIME, "one", 0
    if name == "plain_ifft":
        return flat(np.fft.ifft(zin, axis=1) * n if real else c.inv()), real, V.FREQ, "one", 0
    t = np.fft.ifft(shifted(zin, forward=False), axis=1)  # ifft = scale(1/n) -> ifft_shift -> plain_ifft
    if name == "ifft":
        return flat(t), real, V.FREQ, "one", 0
    if name == "windowed_custom_ifft":
        return flat(t / custom_table(n)), real, V.FREQ, "one", 0
    assert name == "windowed_ifft", op
    wid, oid, alpha = WINDOWS[arg]
    t = windowed(flat(t), True, oid, alpha, unapply=True)
    cut = 2 * (n // 4) if wid in (V.WINDOW_TRIANGULAR, V.WINDOW_BLACKMAN_HARRIS) else 2 * (n // 64)
    return t, real, V.FREQ, "windowed_ifft", cut


def run_facade(obj, op):
    name, _, arg = op.partition(":")
    if name.startswith("real_"):
        name = name[5:]
    if name in ("windowed_fft", "windowed_ifft"):
        return getattr(obj, name)(WINDOWS[arg][0])
    if name in ("windowed_custom_fft", "windowed_custom_ifft"):
        return getattr(obj, name)(custom_window, True)
    return getattr(obj, name)()


def dev_fft(dtype, rows, n, flags, scale, window):
    """bdsp_hip_dev_fft on torch-owned memory -> the buffer that holds the result, as [rows, 2 n] scalars."""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    s = torch.empty_like(d)
    flag = C.c_int(0)
    alpha = FACADE_WINDOW[window][1] if window >= 0 else 0.0
    assert bd.lib.bdsp_hip_dev_fft(0 if dtype == np.float32 else 1, d.data_ptr(), s.data_ptr(), n, rows.shape[0], flags, scale, window,
                                   alpha, C.byref(flag), bd._lib.torch_stream_arg()) == 0
    torch.cuda.synchronize()
    return (s if flag.value else d).cpu().numpy()


def dev_reference(c, flags, scaled, window):
    """What bdsp_hip_dev_fft computes (io_load / io_store, fft_impl.h): window, scale and ifft_shift on the input, the
    unnormalised transform, fft_shift and magnitude on the output."""
    rows = c.x64
    if window >= 0:
        oid, alpha = FACADE_WINDOW[window]
        rows = windowed(rows, True, oid, alpha)
    z = rows.view(np.complex128)
    if scaled:
        z = z / c.n
    if flags & bd._lib.FFT_SHIFT_IN:
        z = shifted(z, forward=False)
    plain = window < 0 and not scaled and not (flags & bd._lib.FFT_SHIFT_IN)
    if flags & 1:
        z = c.inv() if plain else np.fft.ifft(z, axis=1) * c.n
    else:
        z = c.fwd() if plain else np.fft.fft(z, axis=1)
    if flags & bd._lib.FFT_SHIFT_OUT:
        z = shifted(z)
    if flags & bd._lib.FFT_MAGNITUDE:
        return np.stack([orc.magnitude(r) for r in flat(z)])
    return flat(z)


@pytest.mark.parametrize("line", LINES, ids=[" ".join(str(v) for v in l[:5]).replace(" ", "-") for l in LINES])
def test_route(line):
    dname, bits, batch, entry, op, route, cu = line
    if cu:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if cus != 256:
            pytest.skip("the route of this line is written for 256 CUs, the device has %d" % cus)
    dtype = np.float32 if dname == "f32" else np.float64
    tol = 1e-6 if dtype == np.float32 else 1e-12
    n = 1 << bits
    if entry == "conv":
        kv = dict(item.split("=") for item in op.split(","))
        taps, points = int(kv["taps"]), int(kv["points"])
        x = orc.fill_uniform(2 * points, 77 + taps, -10, 10, dtype)
        h = orc.fill_uniform(2 * taps, 78 + taps, -1, 1, dtype) / dtype(np.sqrt(taps))
        v = DspVec(x, is_complex=True)
        assert v.convolve_signal(DspVec(h, is_complex=True)) == 0
        code, ref = orc.overlap_discard(x.astype(np.float64), h.astype(np.float64), orc.next_power_of_two(taps), fair=True)
        assert code == 0
        err = rel_l2(v.data(), ref)
        print("%s: rel-L2 %.3e" % (" ".join(str(v) for v in line[:5]), err))
        record(dtype, "conv", err, line)
        assert err < (2e-6 if dtype == np.float32 else 1e-11)
        return
    c = case(dtype, bits, batch)
    if entry == "dev":
        kv = dict(item.split("=") for item in op.split(","))
        flags, scaled, window = int(kv["flags"]), kv["scale"] != "1", int(kv["window"])
        ref = dev_reference(c, flags, scaled, window)
        got = dev_fft(dtype, c.x, n, flags, 1.0 / n if scaled else 1.0, window)
        width = ref.shape[1]
        got = got.reshape(-1)[:batch * width].reshape(batch, width)  # magnitudes: n reals per vector, back to back
        kind, cut = "one", 0
        alone = ROUTE.get((dname, bits, 1, "dev", op)) == route and batch > 1
        if alone:
            for r in range(batch):
                one = dev_fft(dtype, c.x[r:r + 1], n, flags, 1.0 / n if scaled else 1.0, window).reshape(-1)[:width]
                assert np.array_equal(one, got[r]), r
    else:
        ref, real, domain, kind, cut = reference(c, op)
        src = c.real_rows() if real else c.x
        if entry == "vec":
            assert batch == 1
            v = DspVec(np.ascontiguousarray(src[0]), is_complex=not real, domain=domain)
            assert run_facade(v, op) == 0 and v.is_complex() and len(v) == 2 * n
            got = v.data().reshape(1, -1)
        else:
            m = DspMat(np.ascontiguousarray(src), is_complex=not real, domain=domain)
            assert run_facade(m, op) == 0 and m.is_complex() and m.rows() == batch and m.row_len() == 2 * n
            got = m.data()
            if ROUTE.get((dname, bits, 1, "vec", op)) == route:
                for r in range(batch):
                    v = DspVec(np.ascontiguousarray(src[r]), is_complex=not real, domain=domain)
                    assert run_facade(v, op) == 0
                    assert np.array_equal(v.data(), got[r]), r
    assert got.shape == ref.shape
    worst = 0.0
    for r in range(batch):
        g, f = (got[r][cut:-cut], ref[r][cut:-cut]) if cut else (got[r], ref[r])
        worst = max(worst, rel_l2(g, f))
    print("%s: worst row rel-L2 %.3e" % (" ".join(str(v) for v in line[:5]), worst))
    record(dtype, kind, worst, line)
    assert worst < (4 * tol if kind == "windowed_ifft" else tol)


def test_worst_errors_are_recorded():
    """Prints the worst rel-L2 per precision and kind of comparison over the lines that ran before it (DESIGN.md 4.2 quotes
    the figures of a whole run)."""
    for (dname, kind), (err, line) in sorted(WORST.items()):
        print("worst %s %s: rel-L2 %.3e at `%s`" % (dname, kind, err, line))
        assert np.isfinite(err) and err < 1e-5, (dname, kind, line)
