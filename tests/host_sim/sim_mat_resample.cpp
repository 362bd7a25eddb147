// Host-side emulation of k_rs_fused (basic_dsp_amd/csrc/mat_resample.hip) on the building blocks of fft_core.h: threads
// become a loop, barriers loop boundaries, LDS an array.  Verifies the chain predicated zero-interleave load -> forward
// stages -> x multiplier of the destination bin into natural-order LDS -> gather -> inverse stages -> 1/N on the store
// (real rows: real scalars in, real parts out) against a direct O(N^2) evaluation of zero_interleave / DFT / multiply /
// inverse DFT / 1/N, without a GPU.  The multiplier is an arbitrary complex table: the kernel's own (mask, response,
// ratio, linear phase) is a special case.  Every N = 16 ... 4096 with every factor f = 2 ... N (p = N / f >= 1).
#include <array>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../basic_dsp_amd/csrc/fft_core.h"

using namespace bdsp;
typedef std::complex<double> cd;

// direct evaluation, the roots of unity from a table in double
static std::vector<cd> dft(const std::vector<cd>& x, int dir)
{
    const size_t n = x.size();
    std::vector<cd> w(n), out(n);
    for (size_t m = 0; m < n; ++m) w[m] = cd(cos(2.0 * M_PI * (double)m / (double)n), dir * sin(2.0 * M_PI * (double)m / (double)n));
    for (size_t k = 0; k < n; ++k) {
        cd s = 0;
        for (size_t i = 0; i < n; ++i)
            if (x[i] != cd(0, 0)) s += x[i] * w[(i * k) % n];
        out[k] = s;
    }
    return out;
}

template <typename T, int N, int DIR, class TW>
static void stages(std::vector<std::array<cpx<T>, 16>>& regs, std::vector<cpx<T>>& lds, TW tw)
{
    constexpr int NT = N / 16;
    using F = WgFft<T, N, NT>;
    using P = Radix16Plan<N>;
#define V(t) (*reinterpret_cast<cpx<T>(*)[16]>(regs[t].data()))
    for (int t = 0; t < NT; ++t) F::template compute<16, 1, DIR>(V(t), t, tw);
    if (P::R2 > 1) {
        for (int t = 0; t < NT; ++t) F::template scatter<16, 1>(V(t), t, lds.data());
        for (int t = 0; t < NT; ++t) {
            F::template gather<P::R2>(V(t), t, lds.data());
            F::template compute<P::R2, 16, DIR>(V(t), t, tw);
        }
    }
    if (P::R3 > 1) {
        for (int t = 0; t < NT; ++t) F::template scatter<P::R2, 16>(V(t), t, lds.data());
        for (int t = 0; t < NT; ++t) {
            F::template gather<P::R3>(V(t), t, lds.data());
            F::template compute<P::R3, 16 * P::R2, DIR>(V(t), t, tw);
        }
    }
}

static double g_worst32 = 0, g_worst64 = 0;

template <typename T, int N>
static int check(int lf, bool is_real, double tol)
{
    constexpr int NT = N / 16;
    using F = WgFft<T, N, NT>;
    using P = Radix16Plan<N>;
    constexpr int RL = P::R3 > 1 ? P::R3 : (P::R2 > 1 ? P::R2 : 16);
    constexpr int NSL = N / RL;
    const int p = N >> lf, fmask = (1 << lf) - 1;
    std::vector<T> in(2 * p);
    std::vector<cpx<T>> mult(N), tab(N), out(N), lds(F::LDS_ELEMS);
    srand(N * 31 + lf * 2 + (is_real ? 1 : 0));
    for (auto& v : in) v = (T)(rand() / (double)RAND_MAX * 20 - 10);
    for (auto& v : mult) v = {(T)(rand() / (double)RAND_MAX * 4 - 2), (T)(rand() / (double)RAND_MAX * 4 - 2)};
    for (int m = 0; m < N; ++m) tab[m] = {(T)cos(-2.0 * M_PI * m / N), (T)sin(-2.0 * M_PI * m / N)};
    auto tw = [&](int m) { return tab[m]; };
    const T scale = (T)1 / (T)N;
    const cpx<T>* srcc = reinterpret_cast<const cpx<T>*>(in.data());
    std::vector<std::array<cpx<T>, 16>> regs(NT);
    for (int t = 0; t < NT; ++t)
        for (int r = 0; r < 16; ++r) {
            const int idx = t + r * NT;
            const bool ld = (idx & fmask) == 0;
            const int j = idx >> lf;
            V(t)[r] = ld ? (is_real ? cpx<T>{in[j], 0} : srcc[j]) : cpx<T>{0, 0};
        }
    stages<T, N, -1>(regs, lds, tw);
    for (int t = 0; t < NT; ++t)
        for (int b = 0; b < 16 / RL; ++b)
            for (int r = 0; r < RL; ++r) {
                const int k = F::template out_index<RL, NSL>(t, b, r);
                lds[F::pad(k)] = cmul(V(t)[b * RL + r], mult[k]);
            }
    for (int t = 0; t < NT; ++t)
        for (int r = 0; r < 16; ++r) V(t)[r] = lds[F::pad(F::template in_index<16>(t, 0, r))];
    stages<T, N, 1>(regs, lds, tw);
    for (int t = 0; t < NT; ++t)
        for (int b = 0; b < 16 / RL; ++b)
            for (int r = 0; r < RL; ++r) {
                const int k = F::template out_index<RL, NSL>(t, b, r);
                if (is_real) out[k] = {V(t)[b * RL + r].x * scale, 0};
                else out[k] = cscale(V(t)[b * RL + r], scale);
            }
#undef V
    // direct evaluation
    std::vector<cd> x(N, cd(0, 0));
    for (int j = 0; j < p; ++j) x[(size_t)j << lf] = is_real ? cd(in[j], 0) : cd(in[2 * j], in[2 * j + 1]);
    std::vector<cd> X = dft(x, -1);
    for (int k = 0; k < N; ++k) X[k] *= cd(mult[k].x, mult[k].y);
    std::vector<cd> y = dft(X, 1);
    double num = 0, den = 0;
    for (int k = 0; k < N; ++k) {
        cd want = y[k] / (double)N;
        if (is_real) want = cd(want.real(), 0);
        num += std::norm(cd(out[k].x, out[k].y) - want);
        den += std::norm(want);
    }
    const double e = sqrt(num / den);
    double& worst = sizeof(T) == 4 ? g_worst32 : g_worst64;
    if (e > worst) worst = e;
    if (!(e < tol)) printf("%s N=%5d f=%5d %s  rel-L2 %.3e\n", sizeof(T) == 4 ? "f32" : "f64", N, 1 << lf, is_real ? "real" : "cplx", e);
    return e < tol ? 0 : 1;
}

template <typename T, int N>
static int factors(double tol)
{
    int bad = 0;
    for (int lf = 1; (N >> lf) >= 1; ++lf) bad += check<T, N>(lf, false, tol) + check<T, N>(lf, true, tol);
    printf("%s N=%5d: factors 2 ... %d, real and complex rows: %s\n", sizeof(T) == 4 ? "f32" : "f64", N, N, bad ? "FAIL" : "ok");
    return bad;
}

template <typename T>
static int lengths(double tol)
{
    return factors<T, 16>(tol) + factors<T, 32>(tol) + factors<T, 64>(tol) + factors<T, 128>(tol) + factors<T, 256>(tol) +
           factors<T, 512>(tol) + factors<T, 1024>(tol) + factors<T, 2048>(tol) + factors<T, 4096>(tol);
}

int main()
{
    int bad = lengths<float>(1e-6) + lengths<double>(1e-13);
    printf("worst rel-L2: f32 %.3e, f64 %.3e\n", g_worst32, g_worst64);
    printf(bad ? "FAIL\n" : "OK\n");
    return bad;
}
