// mat_eigh_core.h -- the dispatch rule, pair schedule, LDS maps, per-thread arithmetic and error bounds of mat_eigh.hip,
// host + device: the eigendecomposition of a Hermitian matrix by the cyclic two-sided Jacobi method in a round-robin
// ordering.  The kernels call these templates with raw pointers; tests/host_sim/sim_mat_eigh.cpp calls the SAME templates
// with threads as loops and bounds-checking, write-counting arrays.
//
// Every matrix is dense and row-major; an ELEMENT is one real scalar or one interleaved (re, im) pair (E scalars).
//
// The iteration.  The work matrix A holds BOTH triangles, V starts as I.  One STEP takes floor(n / 2)
// disjoint pairs (p, q), p < q, from je_pair; for each pair whose |a_pq| > thr = eps |A|_F / N it computes
//     tau = (a_qq - a_pp) / (2 |a_pq|),  t = sign(tau) / (|tau| + sqrt(1 + tau^2)),  c = 1 / sqrt(1 + t^2),  s = t c,
//     phi = a_pq / |a_pq|,  u = s phi
// then the row pass  (row p, row q) <- (c row p - u row q, c row q + conj(u) row p)  on A and on V  (J^H A, J^H V),
// then the column pass  (col p, col q) <- (c col p - conj(u) col q, c col q + u col p)  on A  (A J),
// and stores a_pq = a_qp = +0 and the imaginary parts of a_pp, a_qq as +0.  A SWEEP is the n - 1 steps (n for odd n) of
// the tournament.  THE LOWER TRIANGLE GOVERNS: a_pq is read as conj(a[q][p]), q > p, and a_pp, a_qq as re(a[p][p]),
// re(a[q][q]); the upper triangle is carried along by the same rotations and only ever read by the passes.
// Every product-sum is one fma (a complex product is four real ones, as la_cplx_sub), divisions and square roots are the
// correctly rounded ones.  The iteration ends after the first whole sweep without a rotation.
#pragma once

#include <math.h>
#include <stddef.h>

#include "mat_chol_core.h"

namespace bdsp {

constexpr int JE_THREADS = 256;
// the largest N of the one-launch path: A and V of 64 x 64 complex f64 are 2 x 65 KB of LDS, what one CU holds
constexpr size_t JE_SMALL_MAX_N = 64; // not measured (N <= 64 is what one workgroup's LDS holds)
// columns per block of the blocked path: a pair of blocks is one 64 x 64 pivot problem of the small path's code
constexpr int JE_BLOCK = 32; // not measured: no other block size was built
// sweeps of the pivot problem per block step
constexpr int JE_INNER_SWEEPS = 2; // not measured on the device (a host emulation: as many outer sweeps as full inner convergence)
// sweeps (outer sweeps of the blocked path) after which the call gives up with code 8
constexpr int JE_MAX_SWEEPS = 30; // not measured (a host emulation needed at most 11)
constexpr int JE_MAX_PAIRS = 32;  // pairs of one step at most: 64 players

enum JePath { JE_PATH_SMALL = 0, JE_PATH_BLOCKED = 1 };
// the status word of the one-launch path: the sweeps taken (1 .. JE_MAX_SWEEPS) or one of
constexpr unsigned JE_STATUS_NOT_FINITE = 0u, JE_STATUS_NOT_CONVERGED = (unsigned)JE_MAX_SWEEPS + 1u;

// a function of N alone -- never of the number kind, the CU count, timing or the data.  N > 0
inline JePath je_dispatch(size_t N) { return N <= JE_SMALL_MAX_N ? JE_PATH_SMALL : JE_PATH_BLOCKED; }
inline size_t je_blocks(size_t N) { return (N + JE_BLOCK - 1) / JE_BLOCK; }
// steps of one sweep over n players: n - 1, n for odd n (a bye), 0 for a single player
BDSP_LA_HD int je_steps(int n) { return n < 2 ? 0 : (n & 1 ? n : n - 1); }
// pair slots of one step, the bye's included
BDSP_LA_HD int je_pair_slots(int n) { return (n + 1) / 2; }
// launches per (outer) sweep: the small path is one launch for the whole call; blocked: pivot, rows, columns per block step
inline size_t je_launches_per_sweep(size_t N)
{
    return N == 0 || je_dispatch(N) == JE_PATH_SMALL ? 0 : 3 * (size_t)je_steps((int)je_blocks(N));
}
// launches of a call that took S sweeps: blocked adds the completion, the norm and the final ranking
inline size_t je_launches(size_t N, size_t S) { return N == 0 ? 0 : (je_dispatch(N) == JE_PATH_SMALL ? 1 : 3 + S * je_launches_per_sweep(N)); }

// pair k (0 <= k < JE_MAX_PAIRS) of step `step` of the round-robin tournament on n players (circle method: the last of
// an even field stays, the others turn; an odd field gets a phantom player whose partner has the bye).  False for a bye
// or a k past the field.  No division: step + k < 2 (m - 1)
BDSP_LA_HD bool je_pair(int n, int step, int k, int* p, int* q)
{
    const int m = n + (n & 1);
    if (k >= m / 2) return false;
    int a, b;
    if (k == 0) { a = m - 1; b = step; }
    else {
        a = step + k;
        if (a >= m - 1) a -= m - 1;
        b = step - k;
        if (b < 0) b += m - 1;
    }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
    return *q < n;
}

// ---------------------------------------------------------------------------------------------
// derived bounds in units of eps, S the sweeps the call reports:
//     |A - v^H diag(w) v|_F <= je_bound_res(N, S, cplx) eps |A|_F        |v v^H - I|_F <= je_bound_orth(N, S, cplx) eps
// rho: the relative 2-norm error of one plane rotation, the roundings of c, s, phi and of the fma chain and the stored
// zero counted together.  kappa: rho times the steps of a sweep; on the blocked path a block step counts as the 2 x 64
// inner steps of its pivot problem plus the (2 * 64 + 4) eps of its tile products, times sqrt(64) for the pivot transform's
// Frobenius norm.
// ---------------------------------------------------------------------------------------------
inline double je_rho(bool cplx) { return cplx ? 40.0 : 24.0; }
inline double je_kappa(size_t N, bool cplx)
{
    if (N == 0 || je_dispatch(N) == JE_PATH_SMALL) return je_rho(cplx) * (double)N;
    return 8.0 * ((double)(JE_INNER_SWEEPS * 2 * JE_BLOCK) * je_rho(cplx) + (double)(2 * 2 * JE_BLOCK + 4)) * (double)je_steps((int)je_blocks(N));
}
inline double je_bound_orth(size_t N, size_t S, bool cplx) { return 2.0 * je_kappa(N, cplx) * (double)S * sqrt((double)N); }
inline double je_bound_res(size_t N, size_t S, bool cplx) { return 2.0 * je_kappa(N, cplx) * (double)S * (1.0 + sqrt((double)N)) + 1.0; }

// ---------------------------------------------------------------------------------------------
// LDS image of the Jacobi kernels (scalars of T): A then V, each E planes (re, im) of 64 rows at pitch 65 -- lanes along
// a row hit consecutive banks, lanes along a column banks 65 (f32) or 130 dwords (f64) apart: no conflict either way --
// then the rotation table (JE_MAX_PAIRS x 4: c, re u, im u, rotated), then 256 scalars of exchange (the partial sums of
// the norm, the rotation counts, the ranks).
// ---------------------------------------------------------------------------------------------
constexpr int JE_PITCH = 65;
constexpr int JE_PLANE = 64 * JE_PITCH;
constexpr int JE_TAB = 4 * JE_MAX_PAIRS;
constexpr size_t je_lds_scalars(bool cplx) { return (size_t)(cplx ? 4 : 2) * JE_PLANE + JE_TAB + JE_THREADS; }
// the tile kernels: the pivot transform (E planes as above), then a tile of 64 x 32 (rows kernel, pitch 32) or 32 x 64
// (columns kernel, pitch 65) elements, E planes
constexpr int JE_TILE_PLANE = 32 * JE_PITCH;
constexpr size_t je_tile_lds_scalars(bool cplx) { return (size_t)(cplx ? 2 : 1) * (JE_PLANE + JE_TILE_PLANE); }

template <typename T> BDSP_LA_HD T je_eps();
template <> BDSP_LA_HD float je_eps<float>() { return 1.1920928955078125e-07f; }
template <> BDSP_LA_HD double je_eps<double>() { return 2.220446049250313e-16; }
template <typename T> BDSP_LA_HD bool je_finite(T x) { return x > -(T)INFINITY && x < (T)INFINITY; } // NaN compares false

template <typename T, bool CPLX, typename S>
struct JeLds {
    S s;
    static constexpr int E = CPLX ? 2 : 1;
    BDSP_LA_HD int a(int i, int j, int c) const { return c * JE_PLANE + i * JE_PITCH + j; }
    BDSP_LA_HD int v(int i, int j, int c) const { return (E + c) * JE_PLANE + i * JE_PITCH + j; }
    BDSP_LA_HD int tab(int k, int f) const { return 2 * E * JE_PLANE + 4 * k + f; }
    BDSP_LA_HD int red(int t) const { return 2 * E * JE_PLANE + JE_TAB + t; }
};

// row / column i (0 <= i < bp + bq) of a pivot problem in the whole matrix
struct JeMap {
    size_t p0, q0;
    int bp, bq;
    BDSP_LA_HD int m() const { return bp + bq; }
    BDSP_LA_HD size_t at(int i) const { return i < bp ? p0 + (size_t)i : q0 + (size_t)(i - bp); }
};
// the map of pair k of a block step; false for a bye
BDSP_LA_HD bool je_block_map(size_t N, int nb, int step, int k, JeMap* mp)
{
    int p, q;
    if (!je_pair(nb, step, k, &p, &q)) return false;
    mp->p0 = (size_t)p * JE_BLOCK;
    mp->q0 = (size_t)q * JE_BLOCK;
    mp->bp = JE_BLOCK; // p < q: only the last block is short
    const size_t left = N - mp->q0;
    mp->bq = left < (size_t)JE_BLOCK ? (int)left : JE_BLOCK;
    return true;
}

// (xr, xi), (yr, yi) <- c x - u y,  c y + conj(u) x: the plane rotation of both passes
template <typename T, bool CPLX>
BDSP_LA_HD void je_rotate(T c, T ur, T ui, T* xr, T* xi, T* yr, T* yi)
{
    if (CPLX) {
        T pr = c * *xr, pi = c * *xi, qr = c * *yr, qi = c * *yi;
        la_cplx_sub<T>(ur, ui, *yr, *yi, &pr, &pi);
        la_cplx_sub<T>(-ur, ui, *xr, *xi, &qr, &qi);
        *xr = pr; *xi = pi; *yr = qr; *yi = qi;
    } else {
        const T pr = la_fma<T>(-ur, *yr, c * *xr), qr = la_fma<T>(ur, *xr, c * *yr);
        *xr = pr; *yr = qr;
    }
}

// ---------------------------------------------------------------------------------------------
// phases of the Jacobi kernels, thread `tid` of 256; a barrier stands between two phases.
//   G: global accessor, ld(i) / st(i, v) on scalars, ld2(i, &re, &im) / st2(i, re, im) on the pair at scalars i, i + 1.
//   S: ld / st on LDS scalars.
// ---------------------------------------------------------------------------------------------
// the one-launch path's load: src is the caller's matrix (ld = n).  Only j <= i is read, of the diagonal the real part;
// the thread that reads (i, j) writes (j, i) = its conjugate too.  V = I
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void je_load_lower(const JeLds<T, CPLX, S>& l, const G& src, int n, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    for (int idx = tid; idx < n * 64; idx += JE_THREADS) {
        const int i = idx >> 6, j = idx & 63;
        if (j >= n) continue;
        l.s.st(l.v(i, j, 0), i == j ? (T)1 : (T)0);
        if (CPLX) l.s.st(l.v(i, j, 1), (T)0);
        if (j > i) continue;
        const size_t g = ((size_t)i * (size_t)n + (size_t)j) * E;
        T re, im = (T)0;
        if (CPLX && i != j) src.ld2(g, &re, &im);
        else re = src.ld(g);
        l.s.st(l.a(i, j, 0), re);
        if (CPLX) l.s.st(l.a(i, j, 1), im);
        if (i != j) {
            l.s.st(l.a(j, i, 0), re);
            if (CPLX) l.s.st(l.a(j, i, 1), -im);
        }
    }
}

// the pivot problem's load: w is the blocked path's work matrix (both triangles, ld = N).  V = I
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void je_load_pivot(const JeLds<T, CPLX, S>& l, const G& w, size_t ld, const JeMap& mp, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    const int m = mp.m();
    for (int idx = tid; idx < m * 64; idx += JE_THREADS) {
        const int i = idx >> 6, j = idx & 63;
        if (j >= m) continue;
        const size_t g = (mp.at(i) * ld + mp.at(j)) * E;
        T re, im = (T)0;
        if (CPLX) w.ld2(g, &re, &im);
        else re = w.ld(g);
        l.s.st(l.a(i, j, 0), re);
        if (CPLX) l.s.st(l.a(i, j, 1), im);
        l.s.st(l.v(i, j, 0), i == j ? (T)1 : (T)0);
        if (CPLX) l.s.st(l.v(i, j, 1), (T)0);
    }
}

// |A|_F^2 in one fixed order: thread tid sums its elements (idx = tid, tid + 256, ...) of the n x n image into red(tid);
// after a barrier je_norm_total adds the 256 partial sums in ascending order, the same bits in every thread
template <typename T, bool CPLX, typename S>
BDSP_LA_HD void je_norm_partial(const JeLds<T, CPLX, S>& l, int n, int tid)
{
    T sum = (T)0;
    for (int idx = tid; idx < n * 64; idx += JE_THREADS) {
        const int i = idx >> 6, j = idx & 63;
        if (j >= n) continue;
        const T re = l.s.ld(l.a(i, j, 0));
        sum = la_fma<T>(re, re, sum);
        if (CPLX) { const T im = l.s.ld(l.a(i, j, 1)); sum = la_fma<T>(im, im, sum); }
    }
    l.s.st(l.red(tid), sum);
}
// the same over a whole matrix in global memory (ld = n = N): the blocked path's norm kernel, one workgroup
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void je_norm_partial_global(const S& s, int red0, const G& w, size_t N, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    T sum = (T)0;
    for (size_t idx = (size_t)tid; idx < N * N; idx += JE_THREADS) {
        T re, im = (T)0;
        if (CPLX) w.ld2(idx * E, &re, &im);
        else re = w.ld(idx);
        sum = la_fma<T>(re, re, sum);
        if (CPLX) sum = la_fma<T>(im, im, sum);
    }
    s.st(red0 + tid, sum);
}
// thr = eps |A|_F / N; *finite = 0 unless the norm is finite
template <typename T, typename S>
BDSP_LA_HD T je_norm_total(const S& s, int red0, size_t N, unsigned* finite)
{
    T sum = (T)0;
    for (int t = 0; t < JE_THREADS; ++t) sum = sum + s.ld(red0 + t);
    const T norm = la_sqrt<T>(sum);
    *finite = je_finite<T>(norm) ? 1u : 0u;
    return (je_eps<T>() * norm) / (T)N;
}

// step, first phase: thread k < JE_MAX_PAIRS fills row k of the rotation table.  Returns 1 if its pair rotates
template <typename T, bool CPLX, typename S>
BDSP_LA_HD unsigned je_params(const JeLds<T, CPLX, S>& l, int n, int step, T thr, int tid)
{
    if (tid >= JE_MAX_PAIRS) return 0u;
    int p, q;
    unsigned rot = 0u;
    if (je_pair(n, step, tid, &p, &q)) {
        const T gr = l.s.ld(l.a(q, p, 0)), gi = CPLX ? l.s.ld(l.a(q, p, 1)) : (T)0; // a_pq = conj(a[q][p])
        const T mag = CPLX ? la_sqrt<T>(la_fma<T>(gr, gr, gi * gi)) : (gr < (T)0 ? -gr : gr);
        if (mag > thr) { // (NaN compares false)
            const T tau = (l.s.ld(l.a(q, q, 0)) - l.s.ld(l.a(p, p, 0))) / ((T)2 * mag);
            const T at = tau < (T)0 ? -tau : tau;
            T t = (T)1 / (at + la_sqrt<T>(la_fma<T>(tau, tau, (T)1)));
            if (tau < (T)0) t = -t;
            const T c = (T)1 / la_sqrt<T>(la_fma<T>(t, t, (T)1)), sn = t * c;
            l.s.st(l.tab(tid, 0), c);
            l.s.st(l.tab(tid, 1), sn * (gr / mag));
            l.s.st(l.tab(tid, 2), CPLX ? sn * (-gi / mag) : (T)0);
            rot = 1u;
        }
    }
    l.s.st(l.tab(tid, 3), rot ? (T)1 : (T)0);
    return rot;
}

// step, second phase: the row pass on A and V, lanes along the columns; a wave works on one pair and one matrix
template <typename T, bool CPLX, typename S>
BDSP_LA_HD void je_row_pass(const JeLds<T, CPLX, S>& l, int n, int step, int tid)
{
    const int items = je_pair_slots(n) * 128;
    for (int idx = tid; idx < items; idx += JE_THREADS) {
        const int j = idx & 63, onv = (idx >> 6) & 1, k = idx >> 7;
        if (j >= n || l.s.ld(l.tab(k, 3)) == (T)0) continue;
        int p, q;
        je_pair(n, step, k, &p, &q);
        const T c = l.s.ld(l.tab(k, 0)), ur = l.s.ld(l.tab(k, 1)), ui = l.s.ld(l.tab(k, 2));
        const int xp = onv ? l.v(p, j, 0) : l.a(p, j, 0), xq = onv ? l.v(q, j, 0) : l.a(q, j, 0);
        T xr = l.s.ld(xp), yr = l.s.ld(xq), xi = (T)0, yi = (T)0;
        if (CPLX) { xi = l.s.ld(xp + JE_PLANE); yi = l.s.ld(xq + JE_PLANE); }
        je_rotate<T, CPLX>(c, ur, ui, &xr, &xi, &yr, &yi);
        l.s.st(xp, xr);
        l.s.st(xq, yr);
        if (CPLX) { l.s.st(xp + JE_PLANE, xi); l.s.st(xq + JE_PLANE, yi); }
    }
}

// step, third phase: the column pass on A, lanes along the rows; the lanes of rows p and q store the pivot's zeros
template <typename T, bool CPLX, typename S>
BDSP_LA_HD void je_col_pass(const JeLds<T, CPLX, S>& l, int n, int step, int tid)
{
    const int items = je_pair_slots(n) * 64;
    for (int idx = tid; idx < items; idx += JE_THREADS) {
        const int i = idx & 63, k = idx >> 6;
        if (i >= n || l.s.ld(l.tab(k, 3)) == (T)0) continue;
        int p, q;
        je_pair(n, step, k, &p, &q);
        const T c = l.s.ld(l.tab(k, 0)), ur = l.s.ld(l.tab(k, 1)), ui = l.s.ld(l.tab(k, 2));
        const int xp = l.a(i, p, 0), xq = l.a(i, q, 0);
        T xr = l.s.ld(xp), yr = l.s.ld(xq), xi = (T)0, yi = (T)0;
        if (CPLX) { xi = l.s.ld(xp + JE_PLANE); yi = l.s.ld(xq + JE_PLANE); }
        je_rotate<T, CPLX>(c, ur, -ui, &xr, &xi, &yr, &yi);
        if (i == p) { xi = (T)0; yr = (T)0; yi = (T)0; }
        if (i == q) { xr = (T)0; xi = (T)0; yi = (T)0; }
        l.s.st(xp, xr);
        l.s.st(xq, yr);
        if (CPLX) { l.s.st(xp + JE_PLANE, xi); l.s.st(xq + JE_PLANE, yi); }
    }
}

// after a sweep: the threads of the table publish their counts; after a barrier every thread adds them up (small
// integers, exact in T); another barrier before red() is written again
template <typename T, bool CPLX, typename S>
BDSP_LA_HD void je_count_put(const JeLds<T, CPLX, S>& l, unsigned count, int tid)
{
    if (tid < JE_MAX_PAIRS) l.s.st(l.red(tid), (T)count);
}
template <typename T, bool CPLX, typename S>
BDSP_LA_HD unsigned je_count_total(const JeLds<T, CPLX, S>& l)
{
    T sum = (T)0;
    for (int k = 0; k < JE_MAX_PAIRS; ++k) sum = sum + l.s.ld(l.red(k));
    return (unsigned)sum;
}

// rank of eigenvalue k among d[0 .. n): the number of j with d[j] < d[k], or d[j] == d[k] and j < k
template <typename T, typename D>
BDSP_LA_HD int je_rank_of(const D& d, int n, int k)
{
    const T dk = d(k);
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const T dj = d(j);
        r += (dj < dk || (dj == dk && j < k)) ? 1 : 0;
    }
    return r;
}
// the one-launch path's ranking: thread k < n puts the rank of a[k][k] into red(k) ...
template <typename T, bool CPLX, typename S>
BDSP_LA_HD void je_rank_put(const JeLds<T, CPLX, S>& l, int n, int tid)
{
    if (tid >= n) return;
    const auto d = [&](int j) { return l.s.ld(l.a(j, j, 0)); };
    l.s.st(l.red(tid), (T)je_rank_of<T>(d, n, tid));
}
// ... and after a barrier the store: w[rank k] = a[k][k], row rank k of v = row k of V; every element exactly once
template <typename T, bool CPLX, typename S, typename GW, typename GV>
BDSP_LA_HD void je_store_sorted(const JeLds<T, CPLX, S>& l, const GW& w, const GV& v, int n, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    if (tid < n) w.st((size_t)(int)l.s.ld(l.red(tid)), l.s.ld(l.a(tid, tid, 0)));
    for (int idx = tid; idx < n * 64; idx += JE_THREADS) {
        const int i = idx >> 6, j = idx & 63;
        if (j >= n) continue;
        const size_t g = ((size_t)(int)l.s.ld(l.red(i)) * (size_t)n + (size_t)j) * E;
        if (CPLX) v.st2(g, l.s.ld(l.v(i, j, 0)), l.s.ld(l.v(i, j, 1)));
        else v.st(g, l.s.ld(l.v(i, j, 0)));
    }
}

// the pivot problem's store: the block back into the work matrix, the accumulated transform (m x m, pitch 64) into jt
template <typename T, bool CPLX, typename S, typename GW, typename GJ>
BDSP_LA_HD void je_store_pivot(const JeLds<T, CPLX, S>& l, const GW& w, size_t ld, const GJ& jt, const JeMap& mp, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    const int m = mp.m();
    for (int idx = tid; idx < m * 64; idx += JE_THREADS) {
        const int i = idx >> 6, j = idx & 63;
        if (j >= m) continue;
        const size_t g = (mp.at(i) * ld + mp.at(j)) * E, h = (size_t)idx * E;
        if (CPLX) {
            w.st2(g, l.s.ld(l.a(i, j, 0)), l.s.ld(l.a(i, j, 1)));
            jt.st2(h, l.s.ld(l.v(i, j, 0)), l.s.ld(l.v(i, j, 1)));
        } else {
            w.st(g, l.s.ld(l.a(i, j, 0)));
            jt.st(h, l.s.ld(l.v(i, j, 0)));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The tile kernels of the blocked path.  LDS: the pivot transform Vt (m x m) as planes at pitch 65, then the tile.
// Every output element is one chain over ascending k from +0, one rounding per fma.
// ---------------------------------------------------------------------------------------------
BDSP_LA_HD int je_vt_slot(int i, int k, int c, bool cplx) { return c * JE_PLANE + i * JE_PITCH + k; }
template <bool CPLX> BDSP_LA_HD int je_tile0() { return (CPLX ? 2 : 1) * JE_PLANE; }

template <typename T, bool CPLX, typename S, typename GJ>
BDSP_LA_HD void je_tile_load_vt(const S& s, const GJ& jt, int m, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    for (int idx = tid; idx < m * 64; idx += JE_THREADS) {
        const int i = idx >> 6, k = idx & 63;
        if (k >= m) continue;
        T re, im = (T)0;
        if (CPLX) jt.ld2((size_t)idx * E, &re, &im);
        else re = jt.ld((size_t)idx);
        s.st(je_vt_slot(i, k, 0, CPLX), re);
        if (CPLX) s.st(je_vt_slot(i, k, 1, CPLX), im);
    }
}

// rows kernel: X[rows of the pair][c0 .. c0 + nc) <- Vt X, nc <= 32.  Tile element (k, j) at plane c: c * 2048 + k * 32 + j
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void je_rows_load(const S& s, const G& x, size_t ld, const JeMap& mp, size_t c0, int nc, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    const int m = mp.m(), t0 = je_tile0<CPLX>();
    for (int idx = tid; idx < m * 32; idx += JE_THREADS) {
        const int k = idx >> 5, j = idx & 31;
        if (j >= nc) continue;
        const size_t g = (mp.at(k) * ld + c0 + (size_t)j) * E;
        T re, im = (T)0;
        if (CPLX) x.ld2(g, &re, &im);
        else re = x.ld(g);
        s.st(t0 + idx, re);
        if (CPLX) s.st(t0 + 2048 + idx, im);
    }
}
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void je_rows_apply(const S& s, const G& x, size_t ld, const JeMap& mp, size_t c0, int nc, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    const int m = mp.m(), t0 = je_tile0<CPLX>(), j = tid & 31;
    if (j >= nc) return;
    for (int i = tid >> 5; i < m; i += JE_THREADS / 32) {
        T re = (T)0, im = (T)0;
        for (int k = 0; k < m; ++k) {
            const T vr = s.ld(je_vt_slot(i, k, 0, CPLX)), xr = s.ld(t0 + k * 32 + j);
            if (CPLX) {
                const T vi = s.ld(je_vt_slot(i, k, 1, CPLX)), xi = s.ld(t0 + 2048 + k * 32 + j);
                la_cplx_sub<T>(-vr, -vi, xr, xi, &re, &im);
            } else re = la_fma<T>(vr, xr, re);
        }
        const size_t g = (mp.at(i) * ld + c0 + (size_t)j) * E;
        if (CPLX) x.st2(g, re, im);
        else x.st(g, re);
    }
}

// columns kernel: X[r0 .. r0 + nr)[columns of the pair] <- X Vt^H, nr <= 32.  Tile element (i, k) at plane c:
// c * JE_TILE_PLANE + i * 65 + k
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void je_cols_load(const S& s, const G& x, size_t ld, const JeMap& mp, size_t r0, int nr, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    const int m = mp.m(), t0 = je_tile0<CPLX>();
    for (int idx = tid; idx < nr * 64; idx += JE_THREADS) {
        const int i = idx >> 6, k = idx & 63;
        if (k >= m) continue;
        const size_t g = ((r0 + (size_t)i) * ld + mp.at(k)) * E;
        T re, im = (T)0;
        if (CPLX) x.ld2(g, &re, &im);
        else re = x.ld(g);
        s.st(t0 + i * JE_PITCH + k, re);
        if (CPLX) s.st(t0 + JE_TILE_PLANE + i * JE_PITCH + k, im);
    }
}
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void je_cols_apply(const S& s, const G& x, size_t ld, const JeMap& mp, size_t r0, int nr, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    const int m = mp.m(), t0 = je_tile0<CPLX>(), j = tid & 63;
    if (j >= m) return;
    for (int i = tid >> 6; i < nr; i += JE_THREADS / 64) {
        T re = (T)0, im = (T)0;
        for (int k = 0; k < m; ++k) {
            const T vr = s.ld(je_vt_slot(j, k, 0, CPLX)), xr = s.ld(t0 + i * JE_PITCH + k);
            if (CPLX) { // x conj(v)
                const T vi = s.ld(je_vt_slot(j, k, 1, CPLX)), xi = s.ld(t0 + JE_TILE_PLANE + i * JE_PITCH + k);
                la_cplx_sub<T>(-xr, -xi, vr, -vi, &re, &im);
            } else re = la_fma<T>(xr, vr, re);
        }
        const size_t g = ((r0 + (size_t)i) * ld + mp.at(j)) * E;
        if (CPLX) x.st2(g, re, im);
        else x.st(g, re);
    }
}

// the completion: row i of the work matrix from the lower triangle of a (only j <= i is read, of the diagonal the real
// part), row i of V = I; thread tid of the workgroup of row i
template <typename T, bool CPLX, typename GA, typename G>
BDSP_LA_HD void je_complete_row(const GA& a, const G& w, const G& v, size_t N, size_t i, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    for (size_t j = (size_t)tid; j < N; j += JE_THREADS) {
        T re, im = (T)0;
        if (j < i) { if (CPLX) a.ld2((i * N + j) * E, &re, &im); else re = a.ld(i * N + j); }
        else if (j == i) re = a.ld((i * N + j) * E);
        else { if (CPLX) { a.ld2((j * N + i) * E, &re, &im); im = -im; } else re = a.ld(j * N + i); }
        const size_t g = (i * N + j) * E;
        if (CPLX) { w.st2(g, re, im); v.st2(g, i == j ? (T)1 : (T)0, (T)0); }
        else { w.st(g, re); v.st(g, i == j ? (T)1 : (T)0); }
    }
}

// the final ranking: the workgroup of row k.  Thread tid counts over j = tid, tid + 256, ... into red[tid]; after a barrier
// every thread adds the 256 counts (exact in T up to 2^24 rows), then the row is copied to its place
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void je_rank_partial(const S& s, const G& w, size_t N, size_t k, int tid)
{
    constexpr size_t E = CPLX ? 2 : 1;
    const T dk = w.ld((k * N + k) * E);
    unsigned r = 0;
    for (size_t j = (size_t)tid; j < N; j += JE_THREADS) {
        const T dj = w.ld((j * N + j) * E);
        r += (dj < dk || (dj == dk && j < k)) ? 1u : 0u;
    }
    s.st(tid, (T)r);
}
template <typename T, bool CPLX, typename S, typename G, typename GW, typename GV>
BDSP_LA_HD void je_rank_store(const S& s, const G& w, const G& vw, const GW& wout, const GV& vout, size_t N, size_t k, int tid)
{
    constexpr size_t E = CPLX ? 2 : 1;
    T sum = (T)0;
    for (int t = 0; t < JE_THREADS; ++t) sum = sum + s.ld(t);
    const size_t r = (size_t)sum;
    if (tid == 0) wout.st(r, w.ld((k * N + k) * E));
    for (size_t j = (size_t)tid; j < N; j += JE_THREADS) {
        if (CPLX) { T re, im; vw.ld2((k * N + j) * E, &re, &im); vout.st2((r * N + j) * E, re, im); }
        else vout.st(r * N + j, vw.ld(k * N + j));
    }
}

} // namespace bdsp
