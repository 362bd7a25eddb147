"""A process that has lived long: the scenarios of tests/test_gpu_vec_sequences.py::test_a_process_that_has_lived_long,
each in a process of its own (the process-wide tables they fill would change what every later test exercises).  Not
collected by pytest.  Usage: python vec_long_process.py walk | evict.  Exit status 0 and a last line "ok ..." on success;
an AssertionError names the length and the figure otherwise.

walk  -- the twiddle-table cache (runtime.cpp, twiddle_table / twiddle_table_available) after every length that can ask
         for a table has asked.  Which lengths request which tables, from the callers of twiddle_table:
           * mixed_radix.hip (mr_fft: the resident kernels, mixed_radix_reg2.h / _reg3.h included): the length n itself for
             n <= mr_wg_max (4096 in f32, 2048 in f64); the factors n1, n2 of the four-step form, both <= mr_pass_max(2) =
             147456 / (8 * 5) = 3686 in f32 and 147456 / (16 * 5) = 1843 in f64; the factors of the three-pass form,
             <= mr_pass_max(4).  Every one of them is a 13-smooth length (mr_factor) within the resident range of its
             precision, so the key (n, precision) is one a resident length of the walk below requests as well.
           * fft_impl.h, conv.hip, conv_v2_impl.h, bluestein.hip, mat_*.hip: powers of two only.
         The 13-smooth lengths that are no power of two number 477 in 3 .. 4096 and 339 in 3 .. 2048: the walk requests
         477 + 339 = 816 tables, the powers of two 2 .. 4096 of the probes and of Bluestein's inner transforms add at most
         12 + 11 + a few above 4096 per precision.  That is every key the library can form, and it is below the 1024 at
         which twiddle_table_available stops admitting new lengths: no sequence of DspVec calls closes the admission, so
         the refusal branch of mr_supported (mixed_radix.hip) cannot run, whatever the process did before.  The walk
         therefore ends with the cache as full as it can get, and checks what a long-lived process can observe: every
         length of the walk, the probes before and after it (bit-equal), and lengths never seen before.
evict -- the Bluestein plan cache (capi.cpp, bs_plan) past its 1 GiB: see scenario_evict.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle_lib as orc  # noqa: E402

TIME, FREQ = 0, 1
HAMMING = 1


def rel_l2(got, ref):
    got = np.asarray(got, np.float64).ravel()
    ref = np.ascontiguousarray(ref).view(np.float64).ravel() if np.iscomplexobj(ref) else np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def tol_for(dtype):
    """tests/test_gpu_parity.py:33-34, the bound of test_fft_any_length_bluestein (:236)"""
    return 1e-6 if dtype == np.float32 else 1e-12


def smooth13(n):
    for p in (2, 3, 5, 7, 11, 13):
        while n % p == 0:
            n //= p
    return n == 1


def hamming(n):
    with np.errstate(all="ignore"):
        return orc.apply_window(np.ones(2 * n), True, 1, 0.54)[0::2]


def reference(z, name):
    n = z.size
    if name == "plain_fft":
        return np.fft.fft(z)
    if name == "fft":
        return np.roll(np.fft.fft(z), n // 2)
    if name == "windowed_fft":
        return np.roll(np.fft.fft(z * hamming(n)), n // 2)
    return np.fft.ifft(z) * n   # plain_ifft


def transform(bd, x, name):
    v = bd.DspVec(x, is_complex=True, domain=FREQ if name == "plain_ifft" else TIME)
    code = getattr(v, name)(*((HAMMING,) if name == "windowed_fft" else ()))
    assert code == 0, (name, x.size // 2, code)
    return v.data()


# two workgroup-resident smooth lengths, two four-step lengths, one three-pass length, one Bluestein length
PROBES = (360, 3000, 30000, 46080, 4320000, 1009)   # 4320000 = 2^8 3^3 5^4 > 2048^2: three passes in both precisions
PROBE_OPS = ("plain_fft", "fft", "windowed_fft", "plain_ifft")
DTYPES = (np.float32, np.float64)


_REF = {}


def run_probes(bd):
    out = {}
    for dtype in DTYPES:
        for n in PROBES:
            x = orc.fill_uniform(2 * n, 500 + n, -10, 10, dtype)
            z = np.ascontiguousarray(x.astype(np.float64)).view(np.complex128)
            for name in PROBE_OPS:
                got = transform(bd, x, name)
                key = (np.dtype(dtype).name, n, name)
                if key not in _REF:
                    _REF[key] = reference(z, name)
                err = rel_l2(got, _REF[key])
                assert err < tol_for(dtype), ("probe", n, np.dtype(dtype).name, name, err)
                out[(np.dtype(dtype).name, n, name)] = got
    return out


def scenario_walk(bd):
    first = run_probes(bd)
    walked = 0
    for dtype, top in ((np.float32, 4096), (np.float64, 2048)):
        for n in range(3, top + 1):
            if not smooth13(n) or n & (n - 1) == 0:
                continue
            x = orc.fill_uniform(2 * n, 900 + n, -10, 10, dtype)
            got = transform(bd, x, "plain_fft")
            err = rel_l2(got, np.fft.fft(np.ascontiguousarray(x.astype(np.float64)).view(np.complex128)))
            assert err < tol_for(dtype), ("walk", n, np.dtype(dtype).name, err)
            walked += 1
    assert walked == 477 + 339, walked
    again = run_probes(bd)   # (each probe met the numpy bound again inside run_probes)
    for key, got in again.items():   # every probe's tables existed before the walk: the same kernels, the same bits
        assert np.array_equal(got.view(np.uint8), first[key].view(np.uint8)), ("probe changed after the walk", key)
    # lengths never seen before: a four-step length (factors with tables from the walk), a resident one above the f64
    # range in f64 (four-step there), and a prime
    for dtype in DTYPES:
        for n in (2 * 3 * 5 * 7 * 11 * 13, 3003 * 4, 4099):
            x = orc.fill_uniform(2 * n, 1300 + n, -10, 10, dtype)
            z = np.ascontiguousarray(x.astype(np.float64)).view(np.complex128)
            for name in PROBE_OPS:
                err = rel_l2(transform(bd, x, name), reference(z, name))
                assert err < tol_for(dtype), ("new length", n, np.dtype(dtype).name, name, err)
    print("ok walk: %d lengths, %d probe results bit-equal after it" % (walked, len(again)))


# Four lengths just above 2^22 points that mr_supported rejects (mr_factor wants every prime factor <= 13):
# 4194309 = 3 * 7 * 199729, 4194311 = 11 * 381301, 4194319 and 4194329 are prime.  Bluestein runs them on m = 2^24-point
# transforms; a plan holds the chirp (n complex) and its spectrum (m complex): 8 * (n + m) bytes = 160 MiB in f32, one
# plan per direction.  Eight plans are 1.25 GiB: building the seventh evicts the first (BS_CACHE_BYTES = 1 GiB).  The
# library has no cheaper way to get there (the cap is a constant and a plan's size follows from its length), so these
# are the smallest shapes that reach the eviction.
EVICT_LENGTHS = (4194309, 4194311, 4194319, 4194329)
BINS = 16


def bins_by_definition(z, ks):
    """X[k] = sum_j x[j] exp(-2 pi i (j k mod n) / n) in float64 (as _bin_by_definition of tests/test_gpu_full_size.py)"""
    n = z.size
    j = np.arange(n, dtype=np.int64)
    return np.array([np.sum(z * np.exp(-2j * np.pi * ((j * int(k)) % n) / n)) for k in ks])


def scenario_evict(bd):
    def forward_and_back(n):
        x = orc.fill_uniform(2 * n, 77 + n, -10, 10, np.float32)
        v = bd.DspVec(x, is_complex=True)
        assert v.plain_fft() == 0, n
        spec = v.data()
        assert v.plain_ifft() == 0, n
        return x, spec, v.data()

    first = None
    for n in EVICT_LENGTHS:
        x, spec, back = forward_and_back(n)
        if first is None:
            first = (spec.copy(), back.copy())
        z = np.ascontiguousarray(x.astype(np.float64)).view(np.complex128)
        ks = np.unique(np.concatenate([[0, 1, n // 2, n - 1], np.random.RandomState(n % 1000).randint(0, n, BINS)]))[:BINS]
        got = np.ascontiguousarray(spec.astype(np.float64)).view(np.complex128)[ks]
        # tests/test_gpu_full_size.py:291, test_bluestein_lengths_over_two_pass_transforms: rel-L2 < 2e-6 (f32) for the
        # forward transform -- here over the sampled bins; :293: round trip / n against the input < 4e-6
        err = rel_l2(np.ascontiguousarray(got).view(np.float64), bins_by_definition(z, ks))
        assert err < 2e-6, ("forward", n, err)
        err = rel_l2(back.astype(np.float64) / n, x)
        assert err < 4e-6, ("round trip", n, err)
    # the first length again: both of its plans were evicted and are rebuilt -- the same kernels on the same data
    x, spec, back = forward_and_back(EVICT_LENGTHS[0])
    assert np.array_equal(spec.view(np.uint32), first[0].view(np.uint32)), "forward result changed after the plan was rebuilt"
    assert np.array_equal(back.view(np.uint32), first[1].view(np.uint32)), "round trip changed after the plan was rebuilt"
    print("ok evict: %d lengths, first length bit-equal after its plans were rebuilt" % len(EVICT_LENGTHS))


if __name__ == "__main__":
    import basic_dsp_amd as bd
    bd.require_gpu()
    {"walk": scenario_walk, "evict": scenario_evict}[sys.argv[1]](bd)
