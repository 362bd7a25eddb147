// Host-side emulation of k_mc_correlate (basic_dsp_amd/csrc/mat_correlate.hip) on the building blocks of fft_core.h:
// threads become a loop, barriers loop boundaries, LDS an array.  Verifies the chain predicated Surround load ->
// forward stages -> x argument into natural-order LDS -> gather -> inverse stages -> 1/N and swap_halves on the store
// against a direct O(N^2) evaluation of zero_pad / DFT / multiply / inverse DFT / swap_halves, without a GPU.
#include <array>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../basic_dsp_amd/csrc/fft_core.h"

using namespace bdsp;
typedef std::complex<double> cd;

static std::vector<cd> dft(const std::vector<cd>& x, int dir)
{
    const size_t n = x.size();
    std::vector<cd> out(n);
    for (size_t k = 0; k < n; ++k) {
        cd s = 0;
        for (size_t i = 0; i < n; ++i) {
            const double a = dir * 2.0 * M_PI * (double)((i * k) % n) / (double)n;
            s += x[i] * cd(cos(a), sin(a));
        }
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

template <typename T, int N>
static int check(int p, double tol)
{
    constexpr int NT = N / 16;
    using F = WgFft<T, N, NT>;
    using P = Radix16Plan<N>;
    constexpr int RL = P::R3 > 1 ? P::R3 : (P::R2 > 1 ? P::R2 : 16);
    constexpr int NSL = N / RL;
    std::vector<cpx<T>> in(p), arg(N), tab(N), out(N), lds(F::LDS_ELEMS);
    srand(N * 31 + p);
    for (auto& v : in) v = {(T)(rand() / (double)RAND_MAX * 20 - 10), (T)(rand() / (double)RAND_MAX * 20 - 10)};
    for (auto& v : arg) v = {(T)(rand() / (double)RAND_MAX * 20 - 10), (T)(rand() / (double)RAND_MAX * 20 - 10)};
    for (int m = 0; m < N; ++m) tab[m] = {(T)cos(-2.0 * M_PI * m / N), (T)sin(-2.0 * M_PI * m / N)};
    auto tw = [&](int m) { return tab[m]; };
    const int d0 = (N - p) - (N - p) / 2;
    const T scale = (T)1 / (T)N;
    std::vector<std::array<cpx<T>, 16>> regs(NT);
    for (int t = 0; t < NT; ++t)
        for (int r = 0; r < 16; ++r) {
            const int k = t + r * NT - d0;
            V(t)[r] = (k >= 0 && k < p) ? in[k] : cpx<T>{0, 0};
        }
    stages<T, N, -1>(regs, lds, tw);
    for (int t = 0; t < NT; ++t)
        for (int b = 0; b < 16 / RL; ++b)
            for (int r = 0; r < RL; ++r) {
                const int k = F::template out_index<RL, NSL>(t, b, r);
                lds[F::pad(k)] = cmul(V(t)[b * RL + r], arg[k]);
            }
    for (int t = 0; t < NT; ++t)
        for (int r = 0; r < 16; ++r) V(t)[r] = lds[F::pad(F::template in_index<16>(t, 0, r))];
    stages<T, N, 1>(regs, lds, tw);
    for (int t = 0; t < NT; ++t)
        for (int b = 0; b < 16 / RL; ++b)
            for (int r = 0; r < RL; ++r)
                out[F::template out_index<RL, NSL>(t, b, r ^ (RL / 2))] = cscale(V(t)[b * RL + r], scale);
#undef V
    // direct evaluation
    std::vector<cd> x(N, cd(0, 0));
    for (int k = 0; k < p; ++k) x[d0 + k] = cd(in[k].x, in[k].y);
    std::vector<cd> X = dft(x, -1);
    for (int k = 0; k < N; ++k) X[k] *= cd(arg[k].x, arg[k].y);
    std::vector<cd> y = dft(X, 1);
    double num = 0, den = 0;
    for (int k = 0; k < N; ++k) {
        const cd want = y[(k + N - N / 2) % N] / (double)N; // swap_halves: out[(i + N/2) mod N] = y[i]
        num += std::norm(cd(out[k].x, out[k].y) - want);
        den += std::norm(want);
    }
    const double e = sqrt(num / den);
    printf("%s N=%5d p=%5d  rel-L2 %.3e\n", sizeof(T) == 4 ? "f32" : "f64", N, p, e);
    return e < tol ? 0 : 1;
}

template <typename T, int N>
static int sizes(double tol)
{
    return check<T, N>(1, tol) + check<T, N>(N / 2, tol) + check<T, N>(N / 2 + 1, tol) + check<T, N>(N - 1, tol) +
           check<T, N>(N / 4 + 3, tol);
}

int main()
{
    int bad = 0;
    bad += sizes<float, 16>(1e-6);
    bad += sizes<float, 32>(1e-6);
    bad += sizes<float, 64>(1e-6);
    bad += sizes<float, 128>(1e-6);
    bad += sizes<float, 256>(1e-6);
    bad += sizes<float, 512>(1e-6);
    bad += sizes<float, 1024>(1e-6);
    bad += sizes<float, 2048>(1e-6);
    bad += sizes<double, 16>(1e-13);
    bad += sizes<double, 64>(1e-13);
    bad += sizes<double, 512>(1e-13);
    bad += sizes<double, 2048>(1e-13);
    bad += check<float, 4096>(4095, 1e-6);
    bad += check<double, 4096>(2049, 1e-13);
    printf(bad ? "FAIL\n" : "OK\n");
    return bad;
}
