// sim_mat_chol.cpp -- the dispatch rule, launch plan, LDS maps and per-thread arithmetic of
// basic_dsp_amd/csrc/mat_chol_core.h on the host, threads as loops.  usage: sim_mat_chol <tests/mat_chol_shapes.txt>
//
// For every line "path N P" of the shape file, in f32 and f64, real and complex:
//   * la_dispatch returns the path the line names ("empty" for N == 0, which never reaches a kernel);
//   * the launch plan of mat_chol.hip, written out here launch by launch, with the panel kernel and the diagonal solve
//     running the core header's templates (threads as loops, a barrier = the end of a loop over the threads) and the
//     update kernel written as the chain it is (the accumulator starts at C, k ascending; the matrix instruction's order
//     inside a pair of k is not modelled: the bound does not depend on it), writes every element of L and of X exactly
//     once, reads nothing out of bounds, nothing from the upper triangle of a or of L and no imaginary part of a
//     diagonal (they hold NaN here), and never reads in a launch what that launch wrote;
//   * the launch counts are la_chol_launches / la_solve_launches and obey the caps 3 ceil(N / 64) and 2 ceil(N / 64);
//   * L is lower triangular with +0 above the diagonal and in the diagonal's imaginary part, and passes
//     |A - L L^H| <= c(N) eps |L| |L|^H against long double; X passes |B - L X| <= c(N) eps |L| |X| (forward, backward with
//     L^H) and |B - L L^H X| <= c2(N) eps |L| |L|^H |X| (both), element by element;
//   * every LDS access stays inside the kernel's allocation.
// Then the bank conflicts of the panel kernel's column update (the triangle is packed, so they are not 0) are counted
// from the maps and printed.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_chol_core.h"

using namespace bdsp;

static long g_fails = 0;
#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++g_fails < 20) { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                          \
    } while (0)

typedef long double LD;

// a global array with bounds, read permissions, write counts and the launch that wrote each scalar
template <typename T>
struct Arr {
    std::vector<T> v;
    std::vector<int> writes, born;
    std::vector<char> forbidden;
    const char* name = "";
    void init(size_t n, const char* nm) { v.assign(n, (T)0); writes.assign(n, 0); born.assign(n, -1); forbidden.assign(n, 0); name = nm; }
};
static int g_launch = 0;

template <typename T>
struct Glob {
    Arr<T>* a;
    size_t base;
    T ld(size_t i) const
    {
        const size_t g = base + i;
        CHECK(g < a->v.size(), "%s read at %zu of %zu", a->name, g, a->v.size());
        if (g >= a->v.size()) return (T)0;
        CHECK(!a->forbidden[g], "%s read of a forbidden scalar %zu", a->name, g);
        CHECK(a->born[g] != g_launch, "%s scalar %zu read in the launch that wrote it", a->name, g);
        return a->v[g];
    }
    void st(size_t i, T x) const
    {
        const size_t g = base + i;
        CHECK(g < a->v.size(), "%s write at %zu of %zu", a->name, g, a->v.size());
        if (g >= a->v.size()) return;
        a->v[g] = x;
        a->writes[g]++;
        a->born[g] = g_launch;
    }
    void ld2(size_t i, T* re, T* im) const { *re = ld(i); *im = ld(i + 1); }
    void st2(size_t i, T re, T im) const { st(i, re); st(i + 1, im); }
};

template <typename T>
struct Lds {
    std::vector<T>* v;
    T ld(size_t i) const
    {
        CHECK(i < v->size(), "LDS read at %zu of %zu", i, v->size());
        return i < v->size() ? (*v)[i] : (T)0;
    }
    void st(size_t i, T x) const
    {
        CHECK(i < v->size(), "LDS write at %zu of %zu", i, v->size());
        if (i < v->size()) (*v)[i] = x;
    }
};

static unsigned g_rng = 12345u;
static double rnd() // uniform in (-1, 1)
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return ((double)(g_rng >> 8) / (double)(1u << 24)) * 2.0 - 1.0;
}

// ---------------------------------------------------------------------------------------------
// the launches
// ---------------------------------------------------------------------------------------------
template <typename T, bool CPLX>
static unsigned sim_panel(const Glob<T>& src, size_t ld_src, bool masked, T loading, const Glob<T>& out, size_t ld_out, int n,
                          size_t rows_below)
{
    ++g_launch;
    const size_t blocks = rows_below ? (rows_below + LA_BLOCK - 1) / LA_BLOCK : 1;
    unsigned flag = 0;
    for (size_t b = 0; b < blocks; ++b) {
        std::vector<T> mem(la_panel_lds_scalars(CPLX, rows_below != 0), std::numeric_limits<T>::quiet_NaN());
        const LaPanelLds<T, CPLX, Lds<T>> l{{&mem}};
        const size_t sub0 = (size_t)n + (size_t)LA_BLOCK * b, left = rows_below - (size_t)LA_BLOCK * b;
        const int m = rows_below ? (int)(left < (size_t)LA_BLOCK ? left : (size_t)LA_BLOCK) : 0;
        for (int t = 0; t < LA_THREADS; ++t) la_panel_load<T, CPLX>(l, src, ld_src, n, m, sub0, masked, loading, t);
        unsigned bad0 = 0;
        for (int c = 0; c < n; ++c) {
            for (int t = 0; t < LA_THREADS; ++t) {
                const unsigned bad = la_panel_scale<T, CPLX>(l, c, n, m, t);
                if (t == 0) bad0 |= bad;
            }
            for (int t = 0; t < LA_THREADS; ++t) la_panel_update<T, CPLX>(l, c, n, m, t);
        }
        for (int t = 0; t < LA_THREADS; ++t) la_panel_store<T, CPLX>(l, out, ld_out, n, m, sub0, b == 0, t);
        if (b == 0) flag |= bad0;
    }
    return flag;
}

// D = C - A' B' (forms of k_la_update); every element one chain from C over ascending k
template <typename T, bool CPLX>
static void sim_update(int form, const Glob<T>& c, size_t ldc, const Glob<T>& a, size_t lda, const Glob<T>& b, size_t ldb,
                       const Glob<T>& d, size_t ldd, size_t M, size_t NN, size_t K, T loading)
{
    ++g_launch;
    constexpr size_t E = CPLX ? 2 : 1;
    for (size_t row = 0; row < M; ++row)
        for (size_t col = 0; col < NN; ++col) {
            T re = (T)0, im = (T)0;
            const bool upper = form == 0 && col > row;
            if (!upper) {
                if (form == 0 && col == row) re = c.ld((row * ldc + col) * E) + loading;
                else if (CPLX) c.ld2((row * ldc + col) * E, &re, &im);
                else re = c.ld((row * ldc + col) * E);
            }
            if (!upper) // (the device computes the upper half of the diagonal tile too; nobody reads it)
                for (size_t k = 0; k < K; ++k) {
                    T ar, ai = (T)0, br, bi = (T)0;
                    const size_t ia = (form == 2 ? k * lda + row : row * lda + k) * E, ib = (form == 0 ? col * ldb + k : k * ldb + col) * E;
                    if (CPLX) { a.ld2(ia, &ar, &ai); b.ld2(ib, &br, &bi); }
                    else { ar = a.ld(ia); br = b.ld(ib); }
                    if (form == 2) ai = -ai;
                    if (form == 0) bi = -bi;
                    if (CPLX) la_cplx_sub<T>(ar, ai, br, bi, &re, &im);
                    else re = la_fma<T>(-ar, br, re);
                }
            if (CPLX) d.st2((row * ldd + col) * E, re, im);
            else d.st((row * ldd + col) * E, re);
        }
}

template <typename T, bool CPLX, int NB, bool BACK>
static void sim_trsolve_nb(const Glob<T>& l, size_t ldl, const Glob<T>& src, const Glob<T>& dst, size_t P, int n)
{
    std::vector<T> mem((size_t)NB * (NB + 1) / 2 * (CPLX ? 2 : 1), std::numeric_limits<T>::quiet_NaN());
    const Lds<T> s{&mem};
    for (int t = 0; t < LA_THREADS; ++t) la_solve_load_l<T, CPLX, NB>(s, l, ldl, n, t);
    for (size_t col = 0; col < P; ++col) la_solve_column<T, CPLX, NB, BACK>(s, src, dst, P, n, col);
}
template <typename T, bool CPLX, bool BACK>
static void sim_trsolve(const Glob<T>& l, size_t ldl, const Glob<T>& src, const Glob<T>& dst, size_t P, size_t n)
{
    ++g_launch;
    switch (la_solve_nb(n)) {
    case 8: sim_trsolve_nb<T, CPLX, 8, BACK>(l, ldl, src, dst, P, (int)n); break;
    case 16: sim_trsolve_nb<T, CPLX, 16, BACK>(l, ldl, src, dst, P, (int)n); break;
    case 32: sim_trsolve_nb<T, CPLX, 32, BACK>(l, ldl, src, dst, P, (int)n); break;
    default: sim_trsolve_nb<T, CPLX, 64, BACK>(l, ldl, src, dst, P, (int)n); break;
    }
}

// la_chol_run of mat_chol.hip; returns the launches
template <typename T, bool CPLX>
static size_t sim_cholesky(Arr<T>& a, Arr<T>& out, Arr<T>& w, size_t N, T loading, unsigned* flag)
{
    constexpr size_t E = CPLX ? 2 : 1;
    const int first = g_launch;
    *flag = 0;
    if (la_dispatch(N) == LA_PATH_SMALL) {
        *flag |= sim_panel<T, CPLX>(Glob<T>{&a, 0}, N, true, loading, Glob<T>{&out, 0}, N, (int)N, 0);
        return (size_t)(g_launch - first);
    }
    for (size_t c0 = 0; c0 < N; c0 += LA_BLOCK) {
        const size_t n = N - c0 < (size_t)LA_BLOCK ? N - c0 : (size_t)LA_BLOCK, below = N - c0 - n;
        const Glob<T> dst{&out, (c0 * N + c0) * E};
        if (c0 == 0) {
            *flag |= sim_panel<T, CPLX>(Glob<T>{&a, 0}, N, true, loading, dst, N, (int)n, below);
            continue;
        }
        const Glob<T> left{&out, c0 * N * E};
        sim_update<T, CPLX>(0, Glob<T>{&a, (c0 * N + c0) * E}, N, left, N, left, N, Glob<T>{&w, 0}, LA_BLOCK, N - c0, n, c0, loading);
        *flag |= sim_panel<T, CPLX>(Glob<T>{&w, 0}, LA_BLOCK, false, (T)0, dst, N, (int)n, below);
    }
    return (size_t)(g_launch - first);
}

// la_solve_pass of mat_chol.hip
template <typename T, bool CPLX, bool BACK>
static size_t sim_pass(Arr<T>& l, Arr<T>& b, Arr<T>& x, Arr<T>& w, size_t N, size_t P)
{
    constexpr size_t E = CPLX ? 2 : 1;
    const int first = g_launch;
    if (la_dispatch(N) == LA_PATH_SMALL) {
        sim_trsolve<T, CPLX, BACK>(Glob<T>{&l, 0}, N, Glob<T>{&b, 0}, Glob<T>{&x, 0}, P, N);
        return (size_t)(g_launch - first);
    }
    const size_t nb = la_blocks(N);
    for (size_t t = 0; t < nb; ++t) {
        const size_t i = BACK ? nb - 1 - t : t, r0 = i * LA_BLOCK;
        const size_t n = N - r0 < (size_t)LA_BLOCK ? N - r0 : (size_t)LA_BLOCK;
        Glob<T> rhs{&b, r0 * P * E};
        if (t > 0) {
            if (BACK) {
                const size_t k0 = r0 + LA_BLOCK;
                sim_update<T, CPLX>(2, rhs, P, Glob<T>{&l, (k0 * N + r0) * E}, N, Glob<T>{&x, k0 * P * E}, P, Glob<T>{&w, 0}, P, n, P,
                                    N - k0, (T)0);
            } else sim_update<T, CPLX>(1, rhs, P, Glob<T>{&l, r0 * N * E}, N, Glob<T>{&x, 0}, P, Glob<T>{&w, 0}, P, n, P, r0, (T)0);
            rhs = Glob<T>{&w, 0};
        }
        sim_trsolve<T, CPLX, BACK>(Glob<T>{&l, (r0 * N + r0) * E}, N, rhs, Glob<T>{&x, r0 * P * E}, P, n);
    }
    return (size_t)(g_launch - first);
}

// ---------------------------------------------------------------------------------------------
// references in long double
// ---------------------------------------------------------------------------------------------
struct CL { LD re, im; };
static CL cmul(CL a, CL b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename T, bool CPLX> static CL at(const std::vector<T>& v, size_t i)
{
    return {(LD)v[i * (CPLX ? 2 : 1)], CPLX ? (LD)v[i * 2 + 1] : (LD)0};
}

static double g_worst[2][4]; // [path][0 chol, 1 forward, 2 backward, 3 both]

// The write counts, bounds and read rules are checked on every column; the long double residuals on the first and last
// 66 columns and every eighth between (all columns up to P = 132): a column's arithmetic does not depend on its index
// beyond the run of 256 and the tile of 64 it falls in, and those edges are inside the two ends.
static bool residual_column(size_t j, size_t P) { return j < 66 || j + 66 >= P || j % 8 == 0; }

// max over elements of |R - sum_k X[i][k] Y[k][j]| / (c eps sum |X| |Y|), X = op(L) ...: generic through callbacks
template <typename FA, typename FB, typename FR>
static double residual_ratio(size_t rows, size_t cols, size_t K, FA A, FB B, FR R, double c, double eps, bool sample = false)
{
    double worst = 0.0;
    for (size_t i = 0; i < rows; ++i)
        for (size_t j = 0; j < cols; ++j) {
            if (sample && !residual_column(j, cols)) continue;
            CL s = R(i, j);
            LD mod = 0;
            for (size_t k = 0; k < K; ++k) {
                const CL a = A(i, k), b = B(k, j), p = cmul(a, b);
                s.re -= p.re;
                s.im -= p.im;
                mod += hypotl(a.re, a.im) * hypotl(b.re, b.im);
            }
            const LD err = hypotl(s.re, s.im), bound = (LD)c * (LD)eps * mod;
            if (bound == 0) { if (err != 0) worst = 1e30; }
            else if ((double)(err / bound) > worst) worst = (double)(err / bound);
            if (!(err == err)) worst = 1e30;
        }
    return worst;
}

template <typename T, bool CPLX>
static void run_shape(const char* path, size_t N, size_t P)
{
    constexpr size_t E = CPLX ? 2 : 1;
    const double eps = (double)std::numeric_limits<T>::epsilon();
    const T nan = std::numeric_limits<T>::quiet_NaN();
    if (N == 0) {
        CHECK(!strcmp(path, "empty"), "N = 0 is named %s", path);
        CHECK(la_chol_launches(0) == 0 && la_solve_launches(0) == 0, "launches of the empty shape");
        return;
    }
    const LaPath want = !strcmp(path, "small") ? LA_PATH_SMALL : LA_PATH_BLOCKED;
    CHECK(!strcmp(path, "small") || !strcmp(path, "blocked"), "unknown path %s", path);
    CHECK(la_dispatch(N) == want, "N %zu: dispatch gives %d, the line says %s", N, (int)la_dispatch(N), path);
    const int pi = want == LA_PATH_SMALL ? 0 : 1;

    // A = G G^H / 2N + 0.1 I, G random N x 2N, built in long double and rounded; NaN above the diagonal and in the
    // diagonal's imaginary parts, all of them forbidden to read
    std::vector<CL> G(N * 2 * N);
    for (auto& g : G) g = {(LD)rnd(), CPLX ? (LD)rnd() : (LD)0};
    Arr<T> a;
    a.init(N * N * E, "a");
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j < N; ++j) {
            CL s{0, 0};
            if (j <= i)
                for (size_t k = 0; k < 2 * N; ++k) {
                    const CL p = cmul(G[i * 2 * N + k], CL{G[j * 2 * N + k].re, -G[j * 2 * N + k].im});
                    s.re += p.re;
                    s.im += p.im;
                }
            const size_t g = (i * N + j) * E;
            a.v[g] = j <= i ? (T)(s.re / (LD)(2 * N)) : nan;
            if (CPLX) a.v[g + 1] = j < i ? (T)(s.im / (LD)(2 * N)) : nan;
            if (j > i) { a.forbidden[g] = 1; if (CPLX) a.forbidden[g + 1] = 1; }
            if (CPLX && j == i) a.forbidden[g + 1] = 1;
        }
    const T loading = (T)0.1;
    Arr<T> L, w;
    L.init(N * N * E, "L");
    w.init(N * LA_BLOCK * E, "chol temporary");
    unsigned flag = 0;
    const size_t launches = sim_cholesky<T, CPLX>(a, L, w, N, loading, &flag);
    CHECK(flag == 0, "N %zu: a pivot failed on a positive-definite matrix", N);
    CHECK(launches == la_chol_launches(N) && launches <= 3 * la_blocks(N), "N %zu: %zu launches of the factorisation", N, launches);
    for (size_t i = 0; i < N * N * E; ++i) CHECK(L.writes[i] == 1, "N %zu: scalar %zu of L written %d times", N, i, L.writes[i]);
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j < N; ++j) {
            const size_t g = (i * N + j) * E;
            if (j > i) CHECK(L.v[g] == 0 && !signbit(L.v[g]) && (!CPLX || (L.v[g + 1] == 0 && !signbit(L.v[g + 1]))), "L above the diagonal");
            if (j == i) CHECK(L.v[g] > 0 && (!CPLX || (L.v[g + 1] == 0 && !signbit(L.v[g + 1]))), "L's diagonal at %zu", i);
        }
    // |A - L L^H| <= c(N) eps |L| |L|^H on the lower triangle, A the loaded matrix in T
    {
        auto Lf = [&](size_t i, size_t k) { return at<T, CPLX>(L.v, i * N + k); };
        auto Lh = [&](size_t k, size_t j) { CL x = at<T, CPLX>(L.v, j * N + k); x.im = -x.im; return x; };
        auto Af = [&](size_t i, size_t j) { // Hermitian: the upper half from the lower one, which is all that is defined
            const size_t r = i >= j ? i : j, c = i >= j ? j : i;
            if (r == c) return CL{(LD)(T)(a.v[(r * N + c) * E] + loading), 0};
            CL x = at<T, CPLX>(a.v, r * N + c);
            if (j > i) x.im = -x.im;
            return x;
        };
        const double r = residual_ratio(N, N, N, Lf, Lh, Af, la_bound_c(N), eps);
        CHECK(r <= 1.0, "%s N %zu: |A - L L^H| is %.3f of the bound", path, N, r);
        if (r > g_worst[pi][0]) g_worst[pi][0] = r;
    }
    // forbid the upper triangle and the diagonal's imaginary parts of L for the solves
    for (size_t i = 0; i < N; ++i)
        for (size_t j = i; j < N; ++j) {
            const size_t g = (i * N + j) * E;
            if (j > i) { L.forbidden[g] = 1; if (CPLX) L.forbidden[g + 1] = 1; }
            else if (CPLX) L.forbidden[g + 1] = 1;
        }
    Arr<T> b;
    b.init(N * P * E, "b");
    for (auto& x : b.v) x = (T)rnd();
    auto Lf = [&](size_t i, size_t k) { return k <= i ? CL{(LD)L.v[(i * N + k) * E], (CPLX && k < i) ? (LD)L.v[(i * N + k) * E + 1] : (LD)0} : CL{0, 0}; };
    auto Lh = [&](size_t k, size_t j) { CL x = Lf(j, k); x.im = -x.im; return x; };
    auto Bf = [&](size_t i, size_t j) { return at<T, CPLX>(b.v, i * P + j); };
    Arr<T> xf, xb, y, x2, ws;
    ws.init((size_t)LA_BLOCK * P * E, "solve temporary");
    for (int part = 1; part <= 3; ++part) { // forward, backward, both (= forward into y, backward from y)
        Arr<T>& x = part == 1 ? xf : (part == 2 ? xb : x2);
        x.init(N * P * E, "x");
        size_t ln = 0;
        if (part == 1) ln = sim_pass<T, CPLX, false>(L, b, x, ws, N, P);
        else if (part == 2) ln = sim_pass<T, CPLX, true>(L, b, x, ws, N, P);
        else {
            y.init(N * P * E, "y");
            ln = sim_pass<T, CPLX, false>(L, b, y, ws, N, P);
            CHECK(ln == la_solve_launches(N), "forward launches");
            ln = sim_pass<T, CPLX, true>(L, y, x, ws, N, P);
            CHECK(y.v.size() == xf.v.size() && (y.v.empty() || !memcmp(y.v.data(), xf.v.data(), y.v.size() * sizeof(T))), "both: forward half differs");
        }
        CHECK(ln == la_solve_launches(N) && ln <= 2 * la_blocks(N), "N %zu: %zu launches of a triangular pass", N, ln);
        for (size_t i = 0; i < N * P * E; ++i) CHECK(x.writes[i] == 1, "N %zu P %zu part %d: scalar %zu of X written %d times", N, P, part, i, x.writes[i]);
        auto Xf = [&](size_t k, size_t j) { return at<T, CPLX>(x.v, k * P + j); };
        double r;
        if (part == 1) r = residual_ratio(N, P, N, Lf, Xf, Bf, la_bound_c(N), eps, true);
        else if (part == 2) r = residual_ratio(N, P, N, Lh, Xf, Bf, la_bound_c(N), eps, true);
        else {
            // |B - L L^H X| against |L| |L|^H |X|: through M = L^H X and |M|' = |L|^H |X| in long double
            std::vector<CL> Mx(N * P);
            std::vector<LD> Ma(N * P);
            for (size_t k = 0; k < N; ++k)
                for (size_t j = 0; j < P; ++j) {
                    if (!residual_column(j, P)) continue;
                    CL s{0, 0};
                    LD m = 0;
                    for (size_t q = k; q < N; ++q) {
                        const CL lh = Lh(k, q), xx = Xf(q, j), p = cmul(lh, xx);
                        s.re += p.re;
                        s.im += p.im;
                        m += hypotl(lh.re, lh.im) * hypotl(xx.re, xx.im);
                    }
                    Mx[k * P + j] = s;
                    Ma[k * P + j] = m;
                }
            r = 0.0;
            for (size_t i = 0; i < N; ++i)
                for (size_t j = 0; j < P; ++j) {
                    if (!residual_column(j, P)) continue;
                    CL s = Bf(i, j);
                    LD mod = 0;
                    for (size_t k = 0; k <= i; ++k) {
                        const CL lf = Lf(i, k), p = cmul(lf, Mx[k * P + j]);
                        s.re -= p.re;
                        s.im -= p.im;
                        mod += hypotl(lf.re, lf.im) * Ma[k * P + j];
                    }
                    const LD err = hypotl(s.re, s.im), bound = (LD)la_bound_c2(N) * (LD)eps * mod;
                    const double q = bound > 0 ? (double)(err / bound) : (err == 0 ? 0.0 : 1e30);
                    if (q > r || !(err == err)) r = (err == err) ? q : 1e30;
                }
        }
        CHECK(r <= 1.0, "%s N %zu P %zu part %d: the residual is %.3f of the bound", path, N, P, part, r);
        if (r > g_worst[pi][part]) g_worst[pi][part] = r;
    }
}

// the panel kernel's column update, n = m = 64: scalars of `dwords` dwords, lane groups of 32 (4-byte) or 16 (8-byte)
static void count_panel_conflicts(int dwords, int e, long* accesses, long* conflicts)
{
    const int group = dwords == 1 ? 32 : 16;
    auto count = [&](const int* slot, const bool* on) {
        for (int g0 = 0; g0 < 64; g0 += group) {
            int per_bank[32] = {0};
            int addr_seen[64], na = 0, worst = 0;
            for (int l = g0; l < g0 + group; ++l) {
                if (!on[l]) continue;
                bool dup = false;
                for (int q = 0; q < na; ++q) dup |= addr_seen[q] == slot[l];
                if (dup) continue; // a broadcast
                addr_seen[na++] = slot[l];
                for (int d = 0; d < dwords; ++d) { const int bk = (slot[l] * dwords + d) % 32; if (++per_bank[bk] > worst) worst = per_bank[bk]; }
            }
            ++*accesses;
            if (worst > 1) *conflicts += worst - 1;
        }
    };
    for (int c = 0; c < 63; ++c)
        for (int w = 0; w < 4; ++w) {
            int slot[64];
            bool on[64];
            for (int l = 0; l < 64; ++l) { const int k = c + 1 + l; on[l] = k < 64; slot[l] = on[l] ? la_tri_slot(k, c) * e : 0; }
            count(slot, on); // b = L[k][c]
            for (int i = c + 1 + w; i < 64; i += 4) {
                for (int l = 0; l < 64; ++l) { const int k = c + 1 + l; on[l] = k <= i; slot[l] = on[l] ? la_tri_slot(i, k) * e : 0; }
                count(slot, on); // the triangle's row i
            }
            for (int i = w; i < 64; i += 4) {
                for (int l = 0; l < 64; ++l) { const int k = c + 1 + l; on[l] = k < 64; slot[l] = on[l] ? (LA_TRI_SLOTS + la_sub_slot(i, k)) * e : 0; }
                count(slot, on); // the panel's row i
            }
        }
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: sim_mat_chol <shape file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    char line[256];
    int shapes = 0;
    while (fgets(line, sizeof line, f)) {
        char* hash = strchr(line, '#');
        if (hash) *hash = 0;
        char path[32];
        size_t N, P;
        if (sscanf(line, "%31s %zu %zu", path, &N, &P) != 3) continue;
        ++shapes;
        run_shape<float, false>(path, N, P);
        run_shape<float, true>(path, N, P);
        run_shape<double, false>(path, N, P);
        run_shape<double, true>(path, N, P);
    }
    fclose(f);
    // the thresholds and the caps on a grid of N
    for (size_t N = 1; N <= 5000; ++N) {
        CHECK((la_dispatch(N) == LA_PATH_SMALL) == (N <= 64), "dispatch at %zu", N);
        CHECK(la_chol_launches(N) <= 3 * la_blocks(N) && la_solve_launches(N) <= 2 * la_blocks(N), "caps at %zu", N);
    }
    CHECK(la_panel_lds_scalars(true, true) * sizeof(double) == 100352 && la_panel_lds_scalars(true, false) * sizeof(double) == 33792, "LDS sizes");
    static const char* names[2] = {"small", "blocked"};
    for (int p = 0; p < 2; ++p)
        printf("%-8s worst residual / bound: cholesky %.4f, forward %.4f, backward %.4f, both %.4f\n", names[p], g_worst[p][0],
               g_worst[p][1], g_worst[p][2], g_worst[p][3]);
    long acc4 = 0, con4 = 0, acc8 = 0, con8 = 0;
    count_panel_conflicts(1, 1, &acc4, &con4);
    count_panel_conflicts(2, 2, &acc8, &con8);
    printf("LDS (panel update, packed triangle + pitch-65 panel): real f32 %ld accesses, %ld extra bank cycles; complex f64 %ld accesses, %ld extra bank cycles\n",
           acc4, con4, acc8, con8);
    printf("%d shapes (x 4 number kinds), %ld failures\n", shapes, g_fails);
    printf(g_fails ? "FAILED\n" : "ok\n");
    return g_fails ? 1 : 0;
}
