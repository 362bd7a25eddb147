// zoom_fft_core.h -- the index math and the phase arithmetic of zoom_fft.hip, host + device: the convolution length, the
// exact reduction of the chirp phases, the entries of the three chirp tables, what a thread of the fused kernel loads,
// how it multiplies the spectrum between the two transforms and what it stores, and the per-element maps of the general
// path's pre and post kernels.  The kernels call these with raw pointers; tests/host_sim/sim_zoom_fft.cpp calls the SAME
// functions with threads as loops and compares with a direct evaluation of the definition in long double.
//
//     X[k] = sum_{n<N} x[n] exp(-2 pi i (start + k step) n)
//          = post[k] * sum_n (x[n] pre[n]) kern[k - n]                       (k n = (k^2 + n^2 - (k - n)^2) / 2)
//     pre[n]  = exp(-2 pi i (start n + step n^2 / 2))     n < N
//     post[k] = exp(-i pi step k^2)                        k < bins
//     kern[j] = exp(+i pi step j^2)                        -(N - 1) <= j <= bins - 1, wrapped into L points
// a circular convolution of length L = the power of two >= N + bins - 1 (at least 512).
#pragma once

#include <math.h>
#include <stddef.h>

#include "fft_core.h"

#if defined(__HIPCC__)
#define BDSP_ZF_UNROLL _Pragma("unroll")
#else
#define BDSP_ZF_UNROLL
#endif

namespace bdsp {

constexpr size_t ZF_MIN_LEN = 512;              // the fused kernel's shortest workgroup transform
constexpr size_t ZF_MAX_FUSED = 4096;           // ... and its longest
constexpr size_t ZF_MAX_LEN = size_t(1) << 30;  // the longest convolution (j^2 stays below 2^62)

// the convolution length for n >= 1 points and bins >= 1 outputs; 0: above ZF_MAX_LEN
inline size_t zf_conv_len(size_t n, size_t bins)
{
    if (n > ZF_MAX_LEN || bins > ZF_MAX_LEN) return 0;
    const size_t need = n + bins - 1;
    size_t l = ZF_MIN_LEN;
    while (l < need) l <<= 1;
    return l > ZF_MAX_LEN ? 0 : l;
}
inline bool zf_is_fused(size_t l) { return l >= ZF_MIN_LEN && l <= ZF_MAX_FUSED; }

// ---------------------------------------------------------------------------------------------
// phases, in HALF TURNS (the argument of sincospi), reduced exactly before anything is rounded
// ---------------------------------------------------------------------------------------------
// step * j^2 modulo 2 for j < 2^31 and |step| <= 2 (the caller reduces step modulo 2: j^2 is an integer).  j^2 is split
// into two pieces a double holds exactly; each product is an fma pair (hi + lo = the exact product), every half is reduced
// with fmod, which is exact, and only then are they added: three roundings of numbers below 8.
BDSP_HD double zf_phase_sq(double step, unsigned long long j)
{
    const unsigned long long q = j * j;
    const double a = (double)(q >> 32) * 4294967296.0, b = (double)(q & 0xffffffffull);
    const double ha = step * a, la = fma(step, a, -ha);
    const double hb = step * b, lb = fma(step, b, -hb);
    return (fmod(ha, 2.0) + fmod(la, 2.0)) + (fmod(hb, 2.0) + fmod(lb, 2.0));
}
// 2 * frac(start * n) for |start| < 1 (reduced modulo 1 by the caller) and n < 2^31
BDSP_HD double zf_phase_lin(double start, unsigned long long n)
{
    const double x = (double)n, h = start * x, l = fma(start, x, -h);
    return 2.0 * (fmod(h, 1.0) + l);
}

BDSP_HD void zf_sincospi(double h, double* sn, double* cs)
{
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(h, sn, cs);
#else
    const long double a = 3.14159265358979323846264338327950288L * (long double)fmod(h, 2.0);
    *sn = (double)sinl(a);
    *cs = (double)cosl(a);
#endif
}
// exp(i pi h), rounded once to T
template <typename T>
BDSP_HD cpx<T> zf_cis(double h)
{
    double sn, cs;
    zf_sincospi(h, &sn, &cs);
    return cpx<T>{(T)cs, (T)sn};
}

// ---------------------------------------------------------------------------------------------
// the chirp tables
// ---------------------------------------------------------------------------------------------
template <typename T>
BDSP_HD cpx<T> zf_pre_value(double start, double step, unsigned long long n)
{
    return zf_cis<T>(-(zf_phase_lin(start, n) + zf_phase_sq(step, n)));
}
template <typename T>
BDSP_HD cpx<T> zf_post_value(double step, unsigned long long k) { return zf_cis<T>(-zf_phase_sq(step, k)); }
// point i of the wrapped kernel: j = i for i < bins, j = i - l for l - i < n, zero between (l >= n + bins - 1: never both)
template <typename T>
BDSP_HD cpx<T> zf_kern_value(double step, unsigned long long i, unsigned long long n, unsigned long long bins,
                            unsigned long long l)
{
    if (i < bins) return zf_cis<T>(zf_phase_sq(step, i));
    if (l - i < n) return zf_cis<T>(zf_phase_sq(step, l - i));
    return cpx<T>{(T)0, (T)0};
}

// ---------------------------------------------------------------------------------------------
// one input point: x[idx] (a real row reads as (x, 0)) times the pre-chirp, and with a start of the row's own also
// times exp(-2 pi i frac(start_r idx)), evaluated in double and folded into the chirp before the one rounding to T
// ---------------------------------------------------------------------------------------------
template <typename T, bool IN_REAL, bool ROW_START, class In, class Tab>
BDSP_HD cpx<T> zf_in_point(In x, Tab pre, unsigned long long idx, double start_r)
{
    cpx<T> c = pre[idx];
    if (ROW_START) {
        double sn, cs;
        zf_sincospi(-zf_phase_lin(start_r, idx), &sn, &cs);
        const double cx = (double)c.x, cy = (double)c.y;
        c = cpx<T>{(T)(cx * cs - cy * sn), (T)(cx * sn + cy * cs)};
    }
    if constexpr (IN_REAL) {
        const T re = x[idx];
        return cpx<T>{re * c.x, re * c.y};
    } else {
        const cpx<T> xx = x[idx];
        return cmul(xx, c);
    }
}

// ---------------------------------------------------------------------------------------------
// the fused kernel, L in {512, 1024, 2048, 4096}: thread t of the L/16 threads of a row holds 16 points
// ---------------------------------------------------------------------------------------------
template <int L>
struct ZfGeom {
    static constexpr int NT = L / 16;       // threads per row
    static constexpr int B = 256 / NT;      // rows per workgroup
    using P = Radix16Plan<L>;
    static constexpr int R3 = P::R3;
    static_assert(P::R2 == 16 && R3 >= 2, "512 <= L <= 4096");
    static constexpr int NSL = L / R3;
    static constexpr int NTW3 = (16 / R3) * (R3 - 1);
};

// register r <- point t + r NT of the zero-padded, chirped row (x: the row's first element; n points)
template <typename T, int L, bool IN_REAL, bool ROW_START, class In, class Tab>
BDSP_HD void zf_load(cpx<T> (&v)[16], int t, bool active, In x, Tab pre, unsigned n, double start_r)
{
    BDSP_ZF_UNROLL
    for (int r = 0; r < 16; ++r) {
        const unsigned idx = (unsigned)(t + r * ZfGeom<L>::NT);
        cpx<T> a{(T)0, (T)0};
        if (active && idx < n) a = zf_in_point<T, IN_REAL, ROW_START>(x, pre, (unsigned long long)idx, start_r);
        v[r] = a;
    }
}

// between the transforms: after the forward transform register b R3 + r holds spectrum index t + NT (b + r 16/R3); the
// inverse transform's first stage wants index t + NT r' in register r'.  Rename, and multiply by kspec / L on the way.
template <typename T, int L, class Tab>
BDSP_HD void zf_spectrum_mul(cpx<T> (&v)[16], int t, Tab kspec)
{
    using G = ZfGeom<L>;
    const T inv_l = (T)1 / (T)L;
    cpx<T> u[16];
    BDSP_ZF_UNROLL
    for (int b = 0; b < 16 / G::R3; ++b) {
        BDSP_ZF_UNROLL
        for (int r = 0; r < G::R3; ++r) {
            const int rp = b + r * (16 / G::R3);
            const cpx<T> hv = kspec[t + G::NT * rp];
            u[rp] = cmul(v[b * G::R3 + r], cpx<T>{hv.x * inv_l, hv.y * inv_l});
        }
    }
    BDSP_ZF_UNROLL
    for (int r = 0; r < 16; ++r) v[r] = u[r];
}

// after the inverse transform: y[k] = conv[k] post[k] for the k < bins this thread holds (y: the row's first bin)
template <typename T, int L, class Out, class Tab>
BDSP_HD void zf_store(const cpx<T> (&v)[16], int t, Out y, Tab post, unsigned bins)
{
    using G = ZfGeom<L>;
    using F = WgFft<T, L, G::NT>;
    BDSP_ZF_UNROLL
    for (int b = 0; b < 16 / G::R3; ++b) {
        BDSP_ZF_UNROLL
        for (int r = 0; r < G::R3; ++r) {
            const unsigned k = (unsigned)F::template out_index<G::R3, G::NSL>(t, b, r);
            if (k < bins) y[k] = cmul(v[b * G::R3 + r], post[k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the general path: flat element i of the padded workspace (rows x l) and of the result (rows x bins)
// ---------------------------------------------------------------------------------------------
template <typename T, bool IN_REAL, bool ROW_START, class In, class Tab, class Starts>
BDSP_HD cpx<T> zf_pre_point(In x, Tab pre, Starts starts, unsigned long long i, unsigned long long n, unsigned long long l)
{
    const unsigned long long row = i / l, idx = i - row * l;
    if (idx >= n) return cpx<T>{(T)0, (T)0};
    double s = 0.0;
    if (ROW_START) s = starts[row];
    return zf_in_point<T, IN_REAL, ROW_START>(x + row * n, pre, idx, s);
}
template <typename T, class In, class Tab>
BDSP_HD cpx<T> zf_post_point(In conv, Tab post, unsigned long long i, unsigned long long bins, unsigned long long l)
{
    const unsigned long long row = i / bins, k = i - row * bins;
    const cpx<T> z = conv[row * l + k];
    return cmul(z, post[k]);
}

} // namespace bdsp
