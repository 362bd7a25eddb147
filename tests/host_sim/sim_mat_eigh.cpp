// sim_mat_eigh.cpp -- the dispatch rule, pair schedule, launch plan, LDS maps and per-thread arithmetic of
// basic_dsp_amd/csrc/mat_eigh_core.h on the host, threads as loops.  usage: sim_mat_eigh <tests/mat_eigh_shapes.txt>
//
//   * je_pair: for every n in 1 .. 64 and every block count in 1 .. 32 the pairs of a step are disjoint and a sweep holds
//     every unordered pair exactly once;
//   * for every line "path N" of the shape file, in f32 and f64, real and complex: je_dispatch returns the path the line
//     names ("empty" for N == 0, which never reaches a kernel); the launch plan of mat_eigh.hip, written out here launch
//     by launch with the core header's templates (a barrier = the end of a loop over the threads), writes every element
//     of w and v exactly once, reads nothing out of bounds, nothing from the upper triangle of a and no imaginary part
//     of its diagonal (they hold NaN here), and no workgroup reads what another workgroup of the same launch wrote; the
//     launch count is je_launches(N, sweeps); sweeps <= JE_MAX_SWEEPS; w ascends; both derived bounds hold against long
//     double on A = G G^H / 2N + 0.1 I;
//   * the identity, a shuffled diagonal matrix and the zero matrix take 1 sweep, v a permutation matrix to the bit;
//   * a NaN or an infinity in the lower triangle is reported as not finite;
//   * every LDS access stays inside the kernel's allocation.
// Then the bank conflicts of the two passes and of the tile kernels are counted from the maps and printed.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_eigh_core.h"

using namespace bdsp;

// the four number kinds of a shape run as four host threads: counters are shared, the launch clock and the generator are not
static std::atomic<long> g_fails{0};
static std::mutex g_lock;
#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++g_fails < 20) { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                          \
    } while (0)

typedef long double LD;

// a global array with bounds, read permissions, write counts and the launch and workgroup that wrote each scalar
template <typename T>
struct Arr {
    std::vector<T> v;
    std::vector<int> writes, born, born_wg;
    std::vector<char> forbidden;
    const char* name = "";
    void init(size_t n, const char* nm)
    {
        v.assign(n, std::numeric_limits<T>::quiet_NaN());
        writes.assign(n, 0);
        born.assign(n, -1);
        born_wg.assign(n, -1);
        forbidden.assign(n, 0);
        name = nm;
    }
};
static thread_local int g_launch = 0, g_wg = 0;

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
        CHECK(a->born[g] != g_launch || a->born_wg[g] == g_wg, "%s scalar %zu read by another workgroup of the launch that wrote it", a->name, g);
        return a->v[g];
    }
    void st(size_t i, T x) const
    {
        const size_t g = base + i;
        CHECK(g < a->v.size(), "%s write at %zu of %zu", a->name, g, a->v.size());
        if (g >= a->v.size()) return;
        CHECK(a->born[g] != g_launch || a->born_wg[g] == g_wg, "%s scalar %zu written by two workgroups of one launch", a->name, g);
        a->v[g] = x;
        a->writes[g]++;
        a->born[g] = g_launch;
        a->born_wg[g] = g_wg;
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

static thread_local unsigned g_rng = 12345u;
static double rnd() // uniform in (-1, 1)
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return ((double)(g_rng >> 8) / (double)(1u << 24)) * 2.0 - 1.0;
}

// ---------------------------------------------------------------------------------------------
// the launches
// ---------------------------------------------------------------------------------------------
// je_sweep + je_sweep_total of mat_eigh.hip
template <typename T, bool CPLX>
static unsigned sim_sweep(const JeLds<T, CPLX, Lds<T>>& l, int n, T thr)
{
    std::vector<unsigned> count(JE_THREADS, 0u);
    for (int step = 0; step < je_steps(n); ++step) {
        for (int t = 0; t < JE_THREADS; ++t) count[t] += je_params<T, CPLX>(l, n, step, thr, t);
        for (int t = 0; t < JE_THREADS; ++t) je_row_pass<T, CPLX>(l, n, step, t);
        for (int t = 0; t < JE_THREADS; ++t) je_col_pass<T, CPLX>(l, n, step, t);
    }
    for (int t = 0; t < JE_THREADS; ++t) je_count_put<T, CPLX>(l, count[t], t);
    return je_count_total<T, CPLX>(l);
}

// k_je_small; returns the status word
template <typename T, bool CPLX>
static unsigned sim_small(Arr<T>& a, Arr<T>& w, Arr<T>& v, int n)
{
    ++g_launch;
    g_wg = 0;
    std::vector<T> mem(je_lds_scalars(CPLX), std::numeric_limits<T>::quiet_NaN());
    const JeLds<T, CPLX, Lds<T>> l{{&mem}};
    for (int t = 0; t < JE_THREADS; ++t) je_load_lower<T, CPLX>(l, Glob<T>{&a, 0}, n, t);
    for (int t = 0; t < JE_THREADS; ++t) je_norm_partial<T, CPLX>(l, n, t);
    unsigned finite;
    const T thr = je_norm_total<T>(l.s, l.red(0), (size_t)n, &finite);
    unsigned word = JE_STATUS_NOT_CONVERGED;
    for (int sweep = 1; sweep <= JE_MAX_SWEEPS; ++sweep)
        if (sim_sweep<T, CPLX>(l, n, thr) == 0u) { word = (unsigned)sweep; break; }
    if (!finite) word = JE_STATUS_NOT_FINITE;
    for (int t = 0; t < JE_THREADS; ++t) je_rank_put<T, CPLX>(l, n, t);
    for (int t = 0; t < JE_THREADS; ++t) je_store_sorted<T, CPLX>(l, Glob<T>{&w, 0}, Glob<T>{&v, 0}, n, t);
    return word;
}

// je_run_blocked; returns the status word
template <typename T, bool CPLX>
static unsigned sim_blocked(Arr<T>& a, Arr<T>& w, Arr<T>& v, size_t N, size_t* launches)
{
    constexpr size_t E = CPLX ? 2 : 1;
    const int first_launch = g_launch;
    const int nb = (int)je_blocks(N), steps = je_steps(nb), pairs = je_pair_slots(nb);
    Arr<T> wk, vw, jt;
    wk.init(N * N * E, "work matrix");
    vw.init(N * N * E, "work V");
    jt.init((size_t)pairs * 64 * 64 * E, "pivot transforms");
    std::vector<unsigned> counts(1 + (size_t)steps * pairs, 0u);
    // k_je_complete
    ++g_launch;
    for (size_t i = 0; i < N; ++i) {
        g_wg = (int)i;
        for (int t = 0; t < JE_THREADS; ++t) je_complete_row<T, CPLX>(Glob<T>{&a, 0}, Glob<T>{&wk, 0}, Glob<T>{&vw, 0}, N, i, t);
    }
    // k_je_norm
    ++g_launch;
    g_wg = 0;
    T thr;
    {
        std::vector<T> red(JE_THREADS, std::numeric_limits<T>::quiet_NaN());
        const Lds<T> s{&red};
        for (int t = 0; t < JE_THREADS; ++t) je_norm_partial_global<T, CPLX>(s, 0, Glob<T>{&wk, 0}, N, t);
        unsigned finite;
        thr = je_norm_total<T>(s, 0, N, &finite);
        counts[0] = finite ? 0u : 1u;
    }
    unsigned word = JE_STATUS_NOT_CONVERGED;
    for (int sweep = 1; sweep <= JE_MAX_SWEEPS; ++sweep) {
        for (int step = 0; step < steps; ++step) {
            ++g_launch; // k_je_pivot
            for (int k = 0; k < pairs; ++k) {
                g_wg = k;
                JeMap mp;
                if (!je_block_map(N, nb, step, k, &mp)) continue;
                std::vector<T> mem(je_lds_scalars(CPLX), std::numeric_limits<T>::quiet_NaN());
                const JeLds<T, CPLX, Lds<T>> l{{&mem}};
                for (int t = 0; t < JE_THREADS; ++t) je_load_pivot<T, CPLX>(l, Glob<T>{&wk, 0}, N, mp, t);
                unsigned first = 0;
                for (int in = 0; in < JE_INNER_SWEEPS; ++in) {
                    const unsigned total = sim_sweep<T, CPLX>(l, mp.m(), thr);
                    if (in == 0) first = total;
                    if (total == 0u) break;
                }
                for (int t = 0; t < JE_THREADS; ++t)
                    je_store_pivot<T, CPLX>(l, Glob<T>{&wk, 0}, N, Glob<T>{&jt, (size_t)k * 64 * 64 * E}, mp, t);
                counts[1 + (size_t)step * pairs + k] = first;
            }
            ++g_launch; // k_je_rows
            for (int b = 0; b < pairs * 2 * nb; ++b) {
                g_wg = b;
                const int k = b / (2 * nb), tile = b % (2 * nb);
                JeMap mp;
                if (!je_block_map(N, nb, step, k, &mp)) continue;
                const bool onv = tile >= nb;
                const size_t c0 = (size_t)(onv ? tile - nb : tile) * JE_BLOCK;
                if (!onv && (c0 == mp.p0 || c0 == mp.q0)) continue;
                const int nc = N - c0 < (size_t)JE_BLOCK ? (int)(N - c0) : JE_BLOCK;
                std::vector<T> mem(je_tile_lds_scalars(CPLX), std::numeric_limits<T>::quiet_NaN());
                const Lds<T> s{&mem};
                const Glob<T> x{onv ? &vw : &wk, 0};
                for (int t = 0; t < JE_THREADS; ++t) je_tile_load_vt<T, CPLX>(s, Glob<T>{&jt, (size_t)k * 64 * 64 * E}, mp.m(), t);
                for (int t = 0; t < JE_THREADS; ++t) je_rows_load<T, CPLX>(s, x, N, mp, c0, nc, t);
                for (int t = 0; t < JE_THREADS; ++t) je_rows_apply<T, CPLX>(s, x, N, mp, c0, nc, t);
            }
            ++g_launch; // k_je_cols
            for (int b = 0; b < pairs * nb; ++b) {
                g_wg = b;
                const int k = b / nb, tile = b % nb;
                JeMap mp;
                if (!je_block_map(N, nb, step, k, &mp)) continue;
                const size_t r0 = (size_t)tile * JE_BLOCK;
                if (r0 == mp.p0 || r0 == mp.q0) continue;
                const int nr = N - r0 < (size_t)JE_BLOCK ? (int)(N - r0) : JE_BLOCK;
                std::vector<T> mem(je_tile_lds_scalars(CPLX), std::numeric_limits<T>::quiet_NaN());
                const Lds<T> s{&mem};
                const Glob<T> x{&wk, 0};
                for (int t = 0; t < JE_THREADS; ++t) je_tile_load_vt<T, CPLX>(s, Glob<T>{&jt, (size_t)k * 64 * 64 * E}, mp.m(), t);
                for (int t = 0; t < JE_THREADS; ++t) je_cols_load<T, CPLX>(s, x, N, mp, r0, nr, t);
                for (int t = 0; t < JE_THREADS; ++t) je_cols_apply<T, CPLX>(s, x, N, mp, r0, nr, t);
            }
        }
        if (counts[0]) { *launches = (size_t)(g_launch - first_launch); return JE_STATUS_NOT_FINITE; }
        unsigned any = 0;
        for (size_t i = 1; i < counts.size(); ++i) any |= counts[i];
        if (!any) { word = (unsigned)sweep; break; }
    }
    if (word != JE_STATUS_NOT_CONVERGED) {
        ++g_launch; // k_je_sorted
        for (size_t k = 0; k < N; ++k) {
            g_wg = (int)k;
            std::vector<T> red(JE_THREADS, std::numeric_limits<T>::quiet_NaN());
            const Lds<T> s{&red};
            for (int t = 0; t < JE_THREADS; ++t) je_rank_partial<T, CPLX>(s, Glob<T>{&wk, 0}, N, k, t);
            for (int t = 0; t < JE_THREADS; ++t)
                je_rank_store<T, CPLX>(s, Glob<T>{&wk, 0}, Glob<T>{&vw, 0}, Glob<T>{&w, 0}, Glob<T>{&v, 0}, N, k, t);
        }
    }
    *launches = (size_t)(g_launch - first_launch);
    return word;
}

template <typename T, bool CPLX>
static unsigned sim_eigh(Arr<T>& a, Arr<T>& w, Arr<T>& v, size_t N, size_t* launches)
{
    w.init(N, "w");
    v.init(N * N * (CPLX ? 2 : 1), "v");
    if (je_dispatch(N) == JE_PATH_SMALL) { *launches = 1; return sim_small<T, CPLX>(a, w, v, (int)N); }
    return sim_blocked<T, CPLX>(a, w, v, N, launches);
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
// the Hermitian completion of what is read
template <typename T, bool CPLX> static CL herm(const std::vector<T>& a, size_t N, size_t i, size_t j)
{
    const size_t r = i >= j ? i : j, c = i >= j ? j : i;
    if (r == c) return CL{(LD)a[(r * N + c) * (CPLX ? 2 : 1)], 0};
    CL x = at<T, CPLX>(a, r * N + c);
    if (j > i) x.im = -x.im;
    return x;
}

static double g_worst[2][2]; // [path][0 residual, 1 orthogonality]
static unsigned g_sweeps[2];

// both bounds; returns false on a failure
template <typename T, bool CPLX>
static void check_bounds(const char* what, const Arr<T>& a, const Arr<T>& w, const Arr<T>& v, size_t N, unsigned sweeps, int pi)
{
    const LD eps = (LD)std::numeric_limits<T>::epsilon();
    LD na = 0, res = 0, orth = 0;
    std::vector<CL> dv(N * N); // diag(w) v
    for (size_t k = 0; k < N; ++k)
        for (size_t j = 0; j < N; ++j) {
            const CL x = at<T, CPLX>(v.v, k * N + j);
            dv[k * N + j] = {x.re * (LD)w.v[k], x.im * (LD)w.v[k]};
        }
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j < N; ++j) {
            CL s = herm<T, CPLX>(a.v, N, i, j), o{i == j ? (LD)-1 : (LD)0, 0};
            na += s.re * s.re + s.im * s.im;
            for (size_t k = 0; k < N; ++k) {
                CL vh = at<T, CPLX>(v.v, k * N + i); // (v^H)[i][k] = conj(v[k][i])
                vh.im = -vh.im;
                const CL p = cmul(vh, dv[k * N + j]);
                s.re -= p.re;
                s.im -= p.im;
                CL c = at<T, CPLX>(v.v, j * N + k); // (v v^H)[i][j] = sum_k v[i][k] conj(v[j][k])
                c.im = -c.im;
                const CL q = cmul(at<T, CPLX>(v.v, i * N + k), c);
                o.re += q.re;
                o.im += q.im;
            }
            res += s.re * s.re + s.im * s.im;
            orth += o.re * o.re + o.im * o.im;
        }
    na = sqrtl(na); res = sqrtl(res); orth = sqrtl(orth);
    const LD br = (LD)je_bound_res(N, sweeps, CPLX) * eps * na, bo = (LD)je_bound_orth(N, sweeps, CPLX) * eps;
    const double rr = br > 0 ? (double)(res / br) : (res == 0 ? 0.0 : 1e30), ro = bo > 0 ? (double)(orth / bo) : (orth == 0 ? 0.0 : 1e30);
    CHECK(res == res && rr <= 1.0, "%s N %zu: the residual is %.4g of the bound", what, N, rr);
    CHECK(orth == orth && ro <= 1.0, "%s N %zu: the orthogonality defect is %.4g of the bound", what, N, ro);
    const std::lock_guard<std::mutex> hold(g_lock);
    if (rr > g_worst[pi][0]) g_worst[pi][0] = rr;
    if (ro > g_worst[pi][1]) g_worst[pi][1] = ro;
    if (sweeps > g_sweeps[pi]) g_sweeps[pi] = sweeps;
}

template <typename T, bool CPLX>
static void check_outputs(const char* what, const Arr<T>& w, const Arr<T>& v, size_t N)
{
    for (size_t i = 0; i < w.v.size(); ++i) CHECK(w.writes[i] == 1, "%s N %zu: scalar %zu of w written %d times", what, N, i, w.writes[i]);
    for (size_t i = 0; i < v.v.size(); ++i) CHECK(v.writes[i] == 1, "%s N %zu: scalar %zu of v written %d times", what, N, i, v.writes[i]);
    for (size_t i = 1; i < N; ++i) CHECK(w.v[i - 1] <= w.v[i], "%s N %zu: w does not ascend at %zu", what, N, i);
}

template <typename T, bool CPLX>
static void run_shape(const char* path, size_t N)
{
    constexpr size_t E = CPLX ? 2 : 1;
    const T nan = std::numeric_limits<T>::quiet_NaN();
    if (N == 0) {
        CHECK(!strcmp(path, "empty"), "N = 0 is named %s", path);
        CHECK(je_launches(0, 1) == 0 && je_launches_per_sweep(0) == 0, "launches of the empty shape");
        return;
    }
    const JePath want = !strcmp(path, "small") ? JE_PATH_SMALL : JE_PATH_BLOCKED;
    CHECK(!strcmp(path, "small") || !strcmp(path, "blocked"), "unknown path %s", path);
    CHECK(je_dispatch(N) == want, "N %zu: dispatch gives %d, the line says %s", N, (int)je_dispatch(N), path);
    const int pi = want == JE_PATH_SMALL ? 0 : 1;

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
            a.v[g] = j <= i ? (T)(s.re / (LD)(2 * N) + (i == j ? (LD)0.1 : (LD)0)) : nan;
            if (CPLX) a.v[g + 1] = j < i ? (T)(s.im / (LD)(2 * N)) : nan;
            if (j > i) { a.forbidden[g] = 1; if (CPLX) a.forbidden[g + 1] = 1; }
            if (CPLX && j == i) a.forbidden[g + 1] = 1;
        }
    Arr<T> w, v;
    size_t launches = 0;
    const unsigned sweeps = sim_eigh<T, CPLX>(a, w, v, N, &launches);
    CHECK(sweeps >= 1 && sweeps <= (unsigned)JE_MAX_SWEEPS, "N %zu: status %u", N, sweeps);
    CHECK(launches == je_launches(N, sweeps), "N %zu: %zu launches, the plan says %zu", N, launches, je_launches(N, sweeps));
    check_outputs<T, CPLX>("gram", w, v, N);
    check_bounds<T, CPLX>("gram", a, w, v, N, sweeps, pi);

    // the identity, a shuffled diagonal matrix and the zero matrix: 1 sweep, v a permutation matrix to the bit; then a
    // NaN and an infinity in the lower triangle.  On the sizes where the schedule differs: the smallest, an odd one, the
    // edges of the paths
    if (N == 1 || N == 2 || N == 17 || N == 64 || N == 65 || N == 130) {
        for (int kind = 0; kind < 3; ++kind) {
            Arr<T> d;
            d.init(N * N * E, "structured a");
            for (auto& x : d.v) x = (T)0;
            for (size_t i = 0; i < N; ++i) d.v[(i * N + i) * E] = kind == 0 ? (T)1 : (kind == 1 ? (T)(double)((i * 7 + 3) % N) - (T)2 : (T)0);
            const unsigned s1 = sim_eigh<T, CPLX>(d, w, v, N, &launches);
            CHECK(s1 == 1, "N %zu kind %d: %u sweeps on a diagonal matrix", N, kind, s1);
            check_outputs<T, CPLX>("diagonal", w, v, N);
            std::vector<int> hit(N, 0);
            for (size_t k = 0; k < N; ++k) {
                size_t ones = 0, col = 0;
                for (size_t j = 0; j < N; ++j) {
                    const T re = v.v[(k * N + j) * E], im = CPLX ? v.v[(k * N + j) * E + 1] : (T)0;
                    if (re == (T)1 && im == (T)0 && !signbit(im)) { ++ones; col = j; }
                    else CHECK(re == (T)0 && !signbit(re) && im == (T)0 && !signbit(im), "N %zu kind %d: v[%zu][%zu] is no bit of a permutation", N, kind, k, j);
                }
                CHECK(ones == 1, "N %zu kind %d: row %zu of v has %zu ones", N, kind, k, ones);
                if (ones == 1) { hit[col]++; CHECK(w.v[k] == d.v[(col * N + col) * E], "N %zu kind %d: w[%zu]", N, kind, k); }
            }
            for (size_t j = 0; j < N; ++j) CHECK(hit[j] == 1, "N %zu kind %d: column %zu of v", N, kind, j);
            if (kind == 2) for (size_t k = 0; k < N; ++k) CHECK(w.v[k] == (T)0 && !signbit(w.v[k]), "N %zu: w of the zero matrix", N);
        }
        if (N >= 17)
            for (int kind = 0; kind < 2; ++kind) {
                Arr<T> d = a;
                for (auto& f : d.forbidden) f = 0;
                for (size_t i = 0; i < N; ++i)
                    for (size_t j = i; j < N; ++j) {
                        if (j > i) d.v[(i * N + j) * E] = (T)0;
                        if (CPLX) d.v[(i * N + j) * E + 1] = (T)0;
                    }
                d.v[((N - 3) * N + 7) * E] = kind ? std::numeric_limits<T>::infinity() : nan;
                const unsigned s1 = sim_eigh<T, CPLX>(d, w, v, N, &launches);
                CHECK(s1 == JE_STATUS_NOT_FINITE, "N %zu: status %u for a matrix that is not finite", N, s1);
            }
    }
}

// ---------------------------------------------------------------------------------------------
// the schedule
// ---------------------------------------------------------------------------------------------
static void check_schedule(int n)
{
    std::vector<int> met((size_t)n * n, 0);
    for (int step = 0; step < je_steps(n); ++step) {
        std::vector<int> used(n, 0);
        for (int k = 0; k < JE_MAX_PAIRS + 1; ++k) {
            int p = -1, q = -1;
            if (!je_pair(n, step, k, &p, &q)) continue;
            CHECK(k < je_pair_slots(n), "n %d: pair slot %d past je_pair_slots", n, k);
            CHECK(0 <= p && p < q && q < n, "n %d step %d slot %d: pair (%d, %d)", n, step, k, p, q);
            if (!(0 <= p && p < q && q < n)) continue;
            CHECK(!used[p] && !used[q], "n %d step %d: pair (%d, %d) is not disjoint from the others", n, step, p, q);
            used[p] = used[q] = 1;
            met[(size_t)p * n + q]++;
        }
    }
    for (int p = 0; p < n; ++p)
        for (int q = p + 1; q < n; ++q) CHECK(met[(size_t)p * n + q] == 1, "n %d: pair (%d, %d) met %d times in a sweep", n, p, q, met[(size_t)p * n + q]);
}

// ---------------------------------------------------------------------------------------------
// bank conflicts: 32 banks of 4 bytes; lane groups of 32 (4-byte scalars) or 16 (8-byte)
// ---------------------------------------------------------------------------------------------
static void count_group(const int* slot, int dwords, long* accesses, long* conflicts)
{
    const int group = dwords == 1 ? 32 : 16;
    for (int g0 = 0; g0 < 64; g0 += group) {
        int per_bank[32] = {0}, seen[64], ns = 0, worst = 0;
        for (int l = g0; l < g0 + group; ++l) {
            bool dup = false;
            for (int q = 0; q < ns; ++q) dup |= seen[q] == slot[l];
            if (dup) continue; // a broadcast
            seen[ns++] = slot[l];
            for (int d = 0; d < dwords; ++d) { const int bk = (slot[l] * dwords + d) % 32; if (++per_bank[bk] > worst) worst = per_bank[bk]; }
        }
        ++*accesses;
        if (worst > 1) *conflicts += worst - 1;
    }
}
static void count_conflicts(int dwords, long* accesses, long* conflicts)
{
    const JeLds<float, true, int> l{0};
    int slot[64];
    for (int step = 0; step < 63; ++step)
        for (int k = 0; k < 32; ++k) {
            int p, q;
            if (!je_pair(64, step, k, &p, &q)) continue;
            for (int r = 0; r < 2; ++r) {
                for (int j = 0; j < 64; ++j) slot[j] = l.a(r ? q : p, j, 0); // the row pass: lanes along the columns
                count_group(slot, dwords, accesses, conflicts);
                for (int i = 0; i < 64; ++i) slot[i] = l.a(i, r ? q : p, 0); // the column pass: lanes along the rows
                count_group(slot, dwords, accesses, conflicts);
            }
        }
    for (int k = 0; k < 64; ++k) { // the tile kernels: the transform along its rows (columns kernel), the tiles along theirs
        for (int j = 0; j < 64; ++j) slot[j] = je_vt_slot(j, k, 0, true);
        count_group(slot, dwords, accesses, conflicts);
        for (int j = 0; j < 64; ++j) slot[j] = k * 32 + (j & 31); // rows kernel: two rows of the transform per wave are broadcasts
        count_group(slot, dwords, accesses, conflicts);
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: sim_mat_eigh <shape file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    for (int n = 1; n <= 64; ++n) check_schedule(n); // (block counts 1 .. 32 are among them: one schedule serves both)
    for (int n = 1; n <= 64; ++n) CHECK(je_steps(n) == (n < 2 ? 0 : (n % 2 ? n : n - 1)), "steps of %d", n);
    char line[256];
    int shapes = 0;
    while (fgets(line, sizeof line, f)) {
        char* hash = strchr(line, '#');
        if (hash) *hash = 0;
        char path[32];
        size_t N;
        if (sscanf(line, "%31s %zu", path, &N) != 2) continue;
        ++shapes;
        const unsigned seed = 12345u + 16u * (unsigned)shapes;
        std::thread kinds[4] = {std::thread([=] { g_rng = seed; run_shape<float, false>(path, N); }),
                                std::thread([=] { g_rng = seed + 1; run_shape<float, true>(path, N); }),
                                std::thread([=] { g_rng = seed + 2; run_shape<double, false>(path, N); }),
                                std::thread([=] { g_rng = seed + 3; run_shape<double, true>(path, N); })};
        for (auto& k : kinds) k.join();
    }
    fclose(f);
    for (size_t N = 1; N <= 5000; ++N) {
        CHECK((je_dispatch(N) == JE_PATH_SMALL) == (N <= 64), "dispatch at %zu", N);
        const size_t nb = je_blocks(N);
        CHECK(je_launches_per_sweep(N) == (N <= 64 ? 0 : 3 * (nb % 2 ? nb : nb - 1)), "launches per sweep at %zu", N);
    }
    CHECK(je_lds_scalars(true) * sizeof(double) == 136192 && je_lds_scalars(false) * sizeof(float) == 34816, "LDS sizes");
    CHECK(je_lds_scalars(true) * sizeof(double) <= 160 * 1024 && je_tile_lds_scalars(true) * sizeof(double) == 99840, "LDS sizes of the tile kernels");
    static const char* names[2] = {"small", "blocked"};
    for (int p = 0; p < 2; ++p)
        printf("%-8s worst error / bound: residual %.6f, orthogonality %.6f; most sweeps %u of %d\n", names[p], g_worst[p][0], g_worst[p][1],
               g_sweeps[p], JE_MAX_SWEEPS);
    long acc4 = 0, con4 = 0, acc8 = 0, con8 = 0;
    count_conflicts(1, &acc4, &con4);
    count_conflicts(2, &acc8, &con8);
    printf("LDS (row pass, column pass, tile kernels; pitch 65): f32 %ld accesses, %ld extra bank cycles; f64 %ld accesses, %ld extra bank cycles\n",
           acc4, con4, acc8, con8);
    printf("%d shapes (x 4 number kinds), %ld failures\n", shapes, g_fails.load());
    printf(g_fails.load() ? "FAILED\n" : "ok\n");
    return g_fails.load() ? 1 : 0;
}
