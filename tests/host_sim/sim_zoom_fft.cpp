// sim_zoom_fft.cpp -- zoom_fft.hip (basic_dsp_amd/csrc) on the host, threads as loops: the templates of zoom_fft_core.h
// (phase reduction, chirp tables, the fused kernel's load / spectrum multiply / store, the general path's pre and post
// maps) around the workgroup transform of fft_core.h, against a direct O(N bins) evaluation of
//     X[k] = sum_n x[n] exp(-2 pi i (start + k step) n)
// in long double.  f32 and f64, complex and real rows, one start and a start of the row's own, all four fused lengths:
//     (N, bins) = (1, 1) (2, 3) (300, 213) -> 512, (300, 214) -> 1024, (1000, 64) -> 2048, (2048, 2049) -> 4096
// plus one shape of the general path, and the phase reduction alone against exact integer arithmetic (__int128) at
// j = 2^30 - 1 with step in {1/3, 1e-9, -0.49999}.
// Tolerances: rel-L2 per row 1e-6 (f32) / 1e-12 (f64), the project's figures for every transform; the phases 4e-15 half
// turns (three roundings of sums below 8: 3 * 2^-50 = 2.7e-15) and 1e-15 for the linear one (one rounding below 1, doubled).
// g++ -O2 -std=c++17 (optionally -fsanitize=address,undefined) sim_zoom_fft.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "../../basic_dsp_amd/csrc/zoom_fft_core.h"

using namespace bdsp;

static const long double PI_L = 3.14159265358979323846264338327950288L;
static int g_fail = 0;

static unsigned long long g_seed = 0x2545F4914F6CDD1Dull;
static double noise()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (double)(g_seed >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

// ------------------------------------------------------------------ the phase reduction against exact arithmetic
// (v * q) modulo `mod` (1 or 2) for the double v and the integer q < 2^62, exact up to the final conversion
static long double exact_mod(double v, unsigned long long q, int mod)
{
    if (v == 0.0 || q == 0) return 0.0L;
    int e;
    const double f = frexp(fabs(v), &e); // |v| = f 2^e, f in [0.5, 1)
    const unsigned long long m = (unsigned long long)ldexp(f, 53); // 53-bit integer
    e -= 53;                                                        // |v| = m 2^e
    const unsigned __int128 p = (unsigned __int128)m * q;           // < 2^115
    long double r;
    if (e >= 1) r = 0.0L;                                           // an even integer
    else {
        const int s = -e, keep = s + (mod == 2 ? 1 : 0);            // |v| q = p / 2^s; modulo `mod`: the low `keep` bits
        const unsigned __int128 low = keep >= 128 ? p : (p & (((unsigned __int128)1 << keep) - 1));
        r = ldexpl((long double)low, -s);
    }
    return v < 0 ? -r : r;
}
static long double wrap_diff(long double d, int mod)
{
    d = fmodl(d, (long double)mod);
    if (d > mod / 2.0L) d -= mod;
    if (d < -mod / 2.0L) d += mod;
    return fabsl(d);
}
static void check_phases()
{
    const double steps[] = {1.0 / 3.0, 1e-9, -0.49999, 2.0 - 1e-12, -1.75};
    const unsigned long long js[] = {0, 1, 2, 46341, (1ull << 26) + 1, (1ull << 30) - 1, (1ull << 30)};
    long double worst = 0;
    for (double st : steps)
        for (unsigned long long j : js) {
            const long double d = wrap_diff((long double)zf_phase_sq(st, j) - exact_mod(st, j * j, 2), 2);
            if (d > worst) worst = d;
        }
    printf("phase_sq   worst %.3Le half turns\n", worst);
    if (!(worst <= 4e-15L)) { printf("FAIL phase_sq\n"); ++g_fail; }
    const double starts[] = {1.0 / 3.0, 1e-9, -0.99999, 0.5, -0.25};
    worst = 0;
    for (double st : starts)
        for (unsigned long long j : js) {
            const long double d = wrap_diff((long double)zf_phase_lin(st, j) - 2.0L * exact_mod(st, j, 1), 2);
            if (d > worst) worst = d;
        }
    printf("phase_lin  worst %.3Le half turns\n", worst);
    if (!(worst <= 1e-15L)) { printf("FAIL phase_lin\n"); ++g_fail; }
}

// ------------------------------------------------------------------ the definition, in long double
struct CL { long double x, y; };
template <typename T>
static std::vector<CL> direct(const std::vector<T>& x, bool real, unsigned n, unsigned bins, double start, double step)
{
    std::vector<CL> out(bins);
    for (unsigned k = 0; k < bins; ++k) {
        const long double f = (long double)start + (long double)k * (long double)step;
        const long double a1 = -2.0L * PI_L * fmodl(f, 1.0L), wc = cosl(a1), ws = sinl(a1);
        CL acc{0, 0};
        long double c = 1, s = 0;
        for (unsigned i = 0; i < n; ++i) {
            if (i % 32 == 0) { // the phasor afresh every 32 points, rotated in between: 32 roundings of 2^-64 at the most
                const long double a = -2.0L * PI_L * fmodl(f * (long double)i, 1.0L);
                c = cosl(a);
                s = sinl(a);
            } else {
                const long double t = c * wc - s * ws;
                s = c * ws + s * wc;
                c = t;
            }
            const long double re = real ? x[i] : x[2 * i], im = real ? 0 : x[2 * i + 1];
            acc.x += re * c - im * s;
            acc.y += re * s + im * c;
        }
        out[k] = acc;
    }
    return out;
}
template <typename T>
static double rel_l2(const std::vector<cpx<T>>& got, const std::vector<CL>& ref)
{
    long double num = 0, den = 0;
    for (size_t k = 0; k < ref.size(); ++k) {
        const long double dx = (long double)got[k].x - ref[k].x, dy = (long double)got[k].y - ref[k].y;
        num += dx * dx + dy * dy;
        den += ref[k].x * ref[k].x + ref[k].y * ref[k].y;
    }
    return (double)sqrtl(num / den);
}

template <typename T>
struct Tables {
    std::vector<cpx<T>> pre, post, kern;
    Tables(unsigned n, unsigned bins, unsigned l, double start_red, double step_red) : pre(n), post(bins), kern(l)
    {
        for (unsigned i = 0; i < n; ++i) pre[i] = zf_pre_value<T>(start_red, step_red, i);
        for (unsigned i = 0; i < bins; ++i) post[i] = zf_post_value<T>(step_red, i);
        for (unsigned i = 0; i < l; ++i) kern[i] = zf_kern_value<T>(step_red, i, n, bins, l);
    }
};

// ------------------------------------------------------------------ the fused kernel: one row, NT threads as loops
// the forward twiddle table of an L-point transform, and the spectrum of the wrapped kernel: what the plan's one
// power-of-two transform delivers (here a plain DFT in long double; it does not depend on the start)
template <typename T>
struct Spectrum {
    std::vector<cpx<T>> wtab, kspec;
    Spectrum(unsigned n, unsigned bins, int L, double step_red) : wtab(L), kspec(L)
    {
        Tables<T> tb(n, bins, L, 0.0, step_red);
        std::vector<long double> wc(L), ws(L);
        for (int m = 0; m < L; ++m) {
            wc[m] = cosl(-2.0L * PI_L * m / L);
            ws[m] = sinl(-2.0L * PI_L * m / L);
            wtab[m] = cpx<T>{(T)wc[m], (T)ws[m]};
        }
        for (int k = 0; k < L; ++k) {
            long double ax = 0, ay = 0;
            for (int j = 0; j < L; ++j) {
                const int m = (int)(((long long)j * k) % L);
                ax += tb.kern[j].x * wc[m] - tb.kern[j].y * ws[m];
                ay += tb.kern[j].x * ws[m] + tb.kern[j].y * wc[m];
            }
            kspec[k] = cpx<T>{(T)ax, (T)ay};
        }
    }
};

template <typename T, int L, bool REAL, bool ROW_START>
static double run_fused(const Spectrum<T>& sp, unsigned n, unsigned bins, double start, double step)
{
    using G = ZfGeom<L>;
    constexpr int NT = G::NT, R3 = G::R3;
    using F = WgFft<T, L, NT>;
    using XE = typename std::conditional<REAL, T, cpx<T>>::type;
    if (zf_conv_len(n, bins) != (size_t)L) { printf("FAIL conv_len(%u, %u) != %d\n", n, bins, L); ++g_fail; return 0; }
    const double step_red = fmod(step, 2.0) + 0.0, start_row = fmod(start, 1.0), start_red = ROW_START ? 0.0 : start_row + 0.0;
    Tables<T> tb(n, bins, L, start_red, step_red);
    const std::vector<cpx<T>>&wtab = sp.wtab, &kspec = sp.kspec;
    std::vector<T> x((REAL ? 1 : 2) * (size_t)n);
    for (auto& e : x) e = (T)noise();

    struct Regs { cpx<T> v[16]; cpx<T> tw3[G::NTW3]; };
    std::vector<Regs> th(NT);
    std::vector<cpx<T>> lds(F::LDS_ELEMS + 1), tw2l(16 * 17);
    auto tw = [&](int m) { return wtab[m]; };
    for (int t = 0; t < NT; ++t) F::template load_twiddles<R3, 256>(th[t].tw3, t, tw);
    for (int tid = 0; tid < 240; ++tid) {
        const int k = tid / 15, r = tid % 15 + 1;
        tw2l[k * 17 + r - 1] = wtab[r * k * (L / 256)];
    }
    auto fft3 = [&](auto dir) { // a barrier of the kernel = the end of a loop over the threads
        constexpr int DIR = decltype(dir)::value;
        for (int t = 0; t < NT; ++t) F::template compute<16, 1, DIR>(th[t].v, t, tw);
        for (int t = 0; t < NT; ++t) F::template scatter<16, 1>(th[t].v, t, lds.data());
        for (int t = 0; t < NT; ++t) {
            F::template gather<16>(th[t].v, t, lds.data());
            F::template compute_pre<16, 16, DIR>(th[t].v, tw2l.data() + (t & 15) * 17);
        }
        for (int t = 0; t < NT; ++t) F::template scatter<16, 16>(th[t].v, t, lds.data());
        for (int t = 0; t < NT; ++t) {
            F::template gather<R3>(th[t].v, t, lds.data());
            F::template compute_pre<R3, 256, DIR>(th[t].v, th[t].tw3);
        }
    };
    const XE* xv = reinterpret_cast<const XE*>(x.data());
    for (int t = 0; t < NT; ++t) zf_load<T, L, REAL, ROW_START>(th[t].v, t, true, xv, tb.pre.data(), n, start_row);
    fft3(std::integral_constant<int, -1>{});
    for (int t = 0; t < NT; ++t) zf_spectrum_mul<T, L>(th[t].v, t, kspec.data());
    fft3(std::integral_constant<int, 1>{});
    std::vector<cpx<T>> y(bins, cpx<T>{(T)77, (T)77});
    std::vector<int> written(bins, 0);
    struct Out { // counts the writes of every bin
        cpx<T>* y; int* w;
        struct Ref { cpx<T>* p; int* w; void operator=(cpx<T> v) { *p = v; ++*w; } };
        Ref operator[](unsigned k) const { return Ref{y + k, w + k}; }
    };
    for (int t = 0; t < NT; ++t) zf_store<T, L>(th[t].v, t, Out{y.data(), written.data()}, tb.post.data(), bins);
    for (unsigned k = 0; k < bins; ++k)
        if (written[k] != 1) { printf("FAIL bin %u written %d times\n", k, written[k]); ++g_fail; return 0; }
    return rel_l2<T>(y, direct<T>(x, REAL, n, bins, start, step));
}

template <typename T, int L>
static void check_fused(unsigned n, unsigned bins, double start, double step)
{
    const double tol = sizeof(T) == 4 ? 1e-6 : 1e-12;
    const Spectrum<T> sp(n, bins, L, fmod(step, 2.0) + 0.0);
    const double e[4] = {run_fused<T, L, false, false>(sp, n, bins, start, step), run_fused<T, L, true, false>(sp, n, bins, start, step),
                         run_fused<T, L, false, true>(sp, n, bins, start, step), run_fused<T, L, true, true>(sp, n, bins, start, step)};
    printf("f%d L %4d  %4u -> %4u  start %+.6f step %+.3e   complex %.2e real %.2e  row start: complex %.2e real %.2e\n",
           (int)sizeof(T) * 8, L, n, bins, start, step, e[0], e[1], e[2], e[3]);
    for (double v : e)
        if (!(v <= tol)) { printf("FAIL above %.0e\n", tol); ++g_fail; }
}

// ------------------------------------------------------------------ the general path: pre and post maps around a direct
// circular convolution of the bins that are kept
template <typename T, bool REAL, bool ROW_START>
static void check_general(unsigned n, unsigned bins, unsigned rows, double step)
{
    using XE = typename std::conditional<REAL, T, cpx<T>>::type;
    const unsigned l = (unsigned)zf_conv_len(n, bins);
    std::vector<double> starts(rows), red(rows);
    for (unsigned r = 0; r < rows; ++r) { starts[r] = ROW_START ? noise() : 0.3125; red[r] = fmod(starts[r], 1.0); }
    Tables<T> tb(n, bins, l, ROW_START ? 0.0 : red[0] + 0.0, fmod(step, 2.0) + 0.0);
    std::vector<T> x((REAL ? 1 : 2) * (size_t)n * rows);
    for (auto& e : x) e = (T)noise();
    std::vector<cpx<T>> a((size_t)rows * l), conv((size_t)rows * l, cpx<T>{(T)0, (T)0}), y((size_t)rows * bins);
    const XE* xe = reinterpret_cast<const XE*>(x.data());
    for (size_t i = 0; i < a.size(); ++i) a[i] = zf_pre_point<T, REAL, ROW_START>(xe, tb.pre.data(), red.data(), i, n, l);
    for (unsigned r = 0; r < rows; ++r)
        for (unsigned k = 0; k < bins; ++k) {
            long double sx = 0, sy = 0;
            for (unsigned i = 0; i < l; ++i) {
                const cpx<T> u = a[(size_t)r * l + i], h = tb.kern[(k + l - i) % l];
                sx += (long double)u.x * h.x - (long double)u.y * h.y;
                sy += (long double)u.x * h.y + (long double)u.y * h.x;
            }
            conv[(size_t)r * l + k] = cpx<T>{(T)sx, (T)sy};
        }
    for (size_t i = 0; i < y.size(); ++i) y[i] = zf_post_point<T>(conv.data(), tb.post.data(), i, bins, l);
    const double tol = sizeof(T) == 4 ? 1e-6 : 1e-12;
    for (unsigned r = 0; r < rows; ++r) {
        std::vector<T> xr(x.begin() + (size_t)r * n * (REAL ? 1 : 2), x.begin() + (size_t)(r + 1) * n * (REAL ? 1 : 2));
        std::vector<cpx<T>> yr(y.begin() + (size_t)r * bins, y.begin() + (size_t)(r + 1) * bins);
        const double e = rel_l2<T>(yr, direct<T>(xr, REAL, n, bins, starts[r], step));
        printf("f%d general L %u  %u -> %u  row %u %s%s  %.2e\n", (int)sizeof(T) * 8, l, n, bins, r, REAL ? "real" : "complex",
               ROW_START ? " row start" : "", e);
        if (!(e <= tol)) { printf("FAIL above %.0e\n", tol); ++g_fail; }
    }
}

template <typename T>
static void check_all()
{
    check_fused<T, 512>(1, 1, 0.25, 0.125);
    check_fused<T, 512>(2, 3, -0.7, 1.0 / 3.0);
    check_fused<T, 512>(300, 213, 0.1234, 1.0 / 1700.0);
    check_fused<T, 1024>(300, 214, -0.98, -1.0 / 300.0);
    check_fused<T, 2048>(1000, 64, 0.3, 1.0 / 16000.0);
    check_fused<T, 4096>(2048, 2049, 0.5, 1.0 / 2048.0);
    check_fused<T, 512>(100, 37, 0.2, 0.0);
    check_general<T, false, false>(1500, 40, 2, 1.0 / 24000.0);
    check_general<T, true, true>(1500, 40, 2, -1.0 / 24000.0);
}

int main()
{
    if (zf_conv_len(300, 213) != 512 || zf_conv_len(300, 214) != 1024 || zf_conv_len(2048, 2049) != 4096 ||
        zf_conv_len(2049, 2049) != 8192 || zf_conv_len(1, 1) != 512 || zf_conv_len((size_t(1) << 30), 2) != 0 ||
        zf_conv_len((size_t(1) << 29), (size_t(1) << 29) + 1) != (size_t(1) << 30) || !zf_is_fused(4096) || zf_is_fused(8192)) {
        printf("FAIL conv_len\n");
        ++g_fail;
    }
    check_phases();
    check_all<float>();
    check_all<double>();
    printf(g_fail ? "FAILED (%d)\n" : "ok\n", g_fail);
    return g_fail ? 1 : 0;
}
