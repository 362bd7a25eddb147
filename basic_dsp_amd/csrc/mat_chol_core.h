// mat_chol_core.h -- the dispatch rule, launch counts, LDS maps and per-thread arithmetic of mat_chol.hip, host + device:
// the Cholesky factorisation A = L L^H of a Hermitian positive-definite matrix and the triangular solves with L.
// The kernels call these templates with raw pointers; tests/host_sim/sim_mat_chol.cpp calls the SAME templates with
// threads as loops and bounds-checking, write-counting arrays.
//
// Every matrix is dense and row-major; an ELEMENT is one real scalar or one interleaved (re, im) pair (E scalars).
//
// Order of operations, every path, the whole contract of the error bound: element (i, j), j <= i, of L is
//     s = a[i][j]  (the diagonal: re(a[i][i]) + loading, rounded once);  s -= L[i][k] conj(L[j][k]) for k = 0 .. j - 1;
//     L[j][j] = sqrt(s),  L[i][j] = s / L[j][j]
// one chain per element over ascending k (the f32 matrix instruction takes k in pairs), one rounding per fma -- a complex
// step is four of them, two on the real and two on the imaginary sum -- one per division and square root.  The blocked
// path stores the chain's value between launches in the same precision, so it rounds exactly where the small path does.
// The solves are the same chain on x[i] = (b[i] - sum_k L[i][k] x[k]) / L[i][i].
#pragma once

#include <math.h>
#include <stddef.h>

#include "mat_mul_core.h"

#define BDSP_LA_HD BDSP_MM_HD
// The diagonal solve is one straight line of up to 2016 steps.  Left alone, the compiler sinks the arithmetic towards
// the guarded stores at the end and the scheduler lifts the LDS reads of many steps to the front, and both run out of
// registers: the pin (an empty statement that takes and returns the value) keeps every finished unknown where it is
// computed, the fence keeps the scheduler to a few steps at a time.
#if defined(__HIP_DEVICE_COMPILE__)
#define BDSP_LA_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define BDSP_LA_PIN(x) __asm__ volatile("" : "+v"(x))
#else
#define BDSP_LA_SCHED_FENCE() ((void)0)
#define BDSP_LA_PIN(x) ((void)0)
#endif

namespace bdsp {

constexpr int LA_THREADS = 256;
// the block of the blocked path and the largest N of the small path: one 64 x 64 triangle of complex f64 is 33 KB of
// LDS, and 64 complex f64 unknowns per thread are 256 registers, the most a thread of a 256-thread workgroup can hold
// next to its temporaries.  Not measured: no other block size was built.
constexpr int LA_BLOCK = 64;
constexpr size_t LA_SMALL_MAX_N = 64; // not measured (N <= LA_BLOCK is what one workgroup's LDS and registers hold)
// workgroups of the triangular solve at most, each walking runs of 256 columns: 8 per CU of a 256-CU part; not measured
constexpr size_t LA_SOLVE_MAX_BLOCKS = 2048;
constexpr int LA_SOLVE_COLS = LA_THREADS; // columns of B per workgroup and trip: one per thread

enum LaPath { LA_PATH_SMALL = 0, LA_PATH_BLOCKED = 1 };
enum LaPart { LA_PART_BOTH = 0, LA_PART_FORWARD = 1, LA_PART_BACKWARD = 2 };

// a function of N alone -- never of P, the number kind, the CU count, timing or the data.  N > 0
inline LaPath la_dispatch(size_t N) { return N <= LA_SMALL_MAX_N ? LA_PATH_SMALL : LA_PATH_BLOCKED; }
inline size_t la_blocks(size_t N) { return (N + LA_BLOCK - 1) / LA_BLOCK; }
// launches: small 1; blocked one panel kernel per block column and one update before each but the first
inline size_t la_chol_launches(size_t N) { return N == 0 ? 0 : (la_dispatch(N) == LA_PATH_SMALL ? 1 : 2 * la_blocks(N) - 1); }
// per triangular pass: one diagonal solve per block row and one update before each but the first
inline size_t la_solve_launches(size_t N) { return N == 0 ? 0 : (la_dispatch(N) == LA_PATH_SMALL ? 1 : 2 * la_blocks(N) - 1); }
// unknowns per thread of the diagonal solve: the smallest of 8, 16, 32, 64 that holds n
inline int la_solve_nb(size_t n) { return n <= 8 ? 8 : (n <= 16 ? 16 : (n <= 32 ? 32 : 64)); }

// derived bounds in units of eps: |A - L L^H| <= c(N) eps |L| |L|^H, the same for one triangular pass,
// and c2(N) for both passes
inline double la_bound_c(size_t N) { return 2.0 * (double)N + 4.0; }
inline double la_bound_c2(size_t N) { return 3.0 * la_bound_c(N); }

// ---------------------------------------------------------------------------------------------
// LDS images.  The triangle: element (i, j), j <= i, at slot i (i + 1) / 2 + j (2080 slots for 64 rows), E scalars per
// slot.  The panel below it: 64 rows x 64 columns at pitch 65.  Then 64 scalars for the diagonal of L (the triangle's own
// diagonal keeps the pivots until the store).
// ---------------------------------------------------------------------------------------------
constexpr int LA_TRI_SLOTS = LA_BLOCK * (LA_BLOCK + 1) / 2;
constexpr int LA_SUB_PITCH = LA_BLOCK + 1;
constexpr int LA_SUB_SLOTS = LA_BLOCK * LA_SUB_PITCH;
BDSP_LA_HD int la_tri_slot(int i, int j) { return i * (i + 1) / 2 + j; }
BDSP_LA_HD int la_sub_slot(int i, int j) { return i * LA_SUB_PITCH + j; }
// scalars of the panel kernel's LDS: triangle, panel (if there are rows below the block), diagonal
constexpr size_t la_panel_lds_scalars(bool cplx, bool with_sub)
{
    return (size_t)(cplx ? 2 : 1) * (size_t)(LA_TRI_SLOTS + (with_sub ? LA_SUB_SLOTS : 0)) + LA_BLOCK;
}

template <typename T> BDSP_LA_HD T la_fma(T a, T b, T c);
template <> BDSP_LA_HD float la_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> BDSP_LA_HD double la_fma<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T> BDSP_LA_HD T la_sqrt(T a);
template <> BDSP_LA_HD float la_sqrt<float>(float a) { return __builtin_sqrtf(a); }
template <> BDSP_LA_HD double la_sqrt<double>(double a) { return __builtin_sqrt(a); }

// (cr, ci) -= (ar, ai) (br, bi): four real products, two roundings on either sum
template <typename T>
BDSP_LA_HD void la_cplx_sub(T ar, T ai, T br, T bi, T* cr, T* ci)
{
    *cr = la_fma<T>(-ar, br, *cr);
    *cr = la_fma<T>(ai, bi, *cr);
    *ci = la_fma<T>(-ar, bi, *ci);
    *ci = la_fma<T>(-ai, br, *ci);
}

// a pivot is good when it is > 0 and finite (NaN compares false)
template <typename T> BDSP_LA_HD unsigned la_bad_pivot(T p) { return (p > (T)0 && p < (T)INFINITY) ? 0u : 1u; }

// ---------------------------------------------------------------------------------------------
// The panel kernel, thread `tid` of 256, in phases; a barrier stands between two phases.  It factors the n x n diagonal
// block (n <= 64) held as a triangle and carries the m rows (m <= 64, 0 for none) of the panel below it along: column by
// column, right-looking, so every element sees its chain in ascending k.
//   G: global accessor, ld(i) / st(i, v) on scalars, ld2(i, &re, &im) / st2(i, re, im) on the pair at scalars i, i + 1.
//   S: ld / st on LDS scalars.
// ---------------------------------------------------------------------------------------------
template <typename T, bool CPLX, typename S>
struct LaPanelLds {
    S s;
    BDSP_LA_HD int tri(int i, int j, int c) const { return la_tri_slot(i, j) * (CPLX ? 2 : 1) + c; }
    BDSP_LA_HD int sub(int i, int j, int c) const { return (LA_TRI_SLOTS + la_sub_slot(i, j)) * (CPLX ? 2 : 1) + c; }
    // (without a panel the diagonal follows the triangle directly)
    BDSP_LA_HD int dia(int i, bool with_sub) const { return (LA_TRI_SLOTS + (with_sub ? LA_SUB_SLOTS : 0)) * (CPLX ? 2 : 1) + i; }
};

// load: src is the origin of the block column's panel, element (row, col) at (row * ld + col) * E; the diagonal block's
// rows are 0 .. n - 1, the panel's sub0 .. sub0 + m - 1.  Only j <= i of the diagonal block is read, of the diagonal the
// real part alone (its imaginary part is +0); masked (src is the caller's matrix): plus loading, with one rounding.
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void la_panel_load(const LaPanelLds<T, CPLX, S>& l, const G& src, size_t ld, int n, int m, size_t sub0, bool masked,
                              T loading, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    for (int idx = tid; idx < n * LA_BLOCK; idx += LA_THREADS) {
        const int i = idx >> 6, j = idx & 63;
        if (j > i) continue;
        const size_t g = ((size_t)i * ld + (size_t)j) * E;
        T re, im = (T)0;
        if (CPLX && i != j) src.ld2(g, &re, &im);
        else re = src.ld(g);
        if (masked && i == j) re = re + loading;
        l.s.st(l.tri(i, j, 0), re);
        if (CPLX) l.s.st(l.tri(i, j, 1), im);
    }
    for (int idx = tid; idx < m * LA_BLOCK; idx += LA_THREADS) {
        const int i = idx >> 6, j = idx & 63;
        if (j >= n) continue;
        const size_t g = ((sub0 + (size_t)i) * ld + (size_t)j) * E;
        T re, im = (T)0;
        if (CPLX) src.ld2(g, &re, &im);
        else re = src.ld(g);
        l.s.st(l.sub(i, j, 0), re);
        if (CPLX) l.s.st(l.sub(i, j, 1), im);
    }
}

// column c, first phase: every thread reads the pivot (the same bits in all of them) and takes its root; the rows below
// are divided by it, one row per thread; thread 0 keeps the root.  Returns 1 for a bad pivot
template <typename T, bool CPLX, typename S>
BDSP_LA_HD unsigned la_panel_scale(const LaPanelLds<T, CPLX, S>& l, int c, int n, int m, int tid)
{
    const T p = l.s.ld(l.tri(c, c, 0));
    const T d = la_sqrt<T>(p);
    const int below = n - 1 - c;
    if (tid < below + m) {
        const bool in_tri = tid < below;
        const int i = in_tri ? c + 1 + tid : tid - below;
        for (int e = 0; e < (CPLX ? 2 : 1); ++e) {
            const int slot = in_tri ? l.tri(i, c, e) : l.sub(i, c, e);
            l.s.st(slot, l.s.ld(slot) / d);
        }
    }
    if (tid == 0) l.s.st(l.dia(c, m > 0), d);
    return la_bad_pivot<T>(p);
}

// column c, second phase: a[i][k] -= a[i][c] conj(a[k][c]) for c < k <= i (the triangle) and all rows of the panel;
// lane (tid & 63) owns column k = c + 1 + lane, wave (tid >> 6) every fourth row.  On the diagonal only the real part
// moves: its imaginary part is +0 by definition, not by cancellation
template <typename T, bool CPLX, typename S>
BDSP_LA_HD void la_panel_update(const LaPanelLds<T, CPLX, S>& l, int c, int n, int m, int tid)
{
    const int k = c + 1 + (tid & 63), w = tid >> 6;
    if (k >= n) return;
    const T br = l.s.ld(l.tri(k, c, 0)), bi = CPLX ? l.s.ld(l.tri(k, c, 1)) : (T)0;
    for (int i = c + 1 + w; i < n; i += LA_THREADS / 64) {
        if (k > i) continue;
        const T ar = l.s.ld(l.tri(i, c, 0)), ai = CPLX ? l.s.ld(l.tri(i, c, 1)) : (T)0;
        T cr = l.s.ld(l.tri(i, k, 0)), ci = (CPLX && k < i) ? l.s.ld(l.tri(i, k, 1)) : (T)0;
        if (CPLX) {
            if (k < i) la_cplx_sub<T>(ar, ai, br, -bi, &cr, &ci);
            else { cr = la_fma<T>(-ar, br, cr); cr = la_fma<T>(-ai, bi, cr); }
        } else cr = la_fma<T>(-ar, br, cr);
        l.s.st(l.tri(i, k, 0), cr);
        if (CPLX && k < i) l.s.st(l.tri(i, k, 1), ci);
    }
    for (int i = w; i < m; i += LA_THREADS / 64) {
        const T ar = l.s.ld(l.sub(i, c, 0)), ai = CPLX ? l.s.ld(l.sub(i, c, 1)) : (T)0;
        T cr = l.s.ld(l.sub(i, k, 0)), ci = CPLX ? l.s.ld(l.sub(i, k, 1)) : (T)0;
        if (CPLX) la_cplx_sub<T>(ar, ai, br, -bi, &cr, &ci);
        else cr = la_fma<T>(-ar, br, cr);
        l.s.st(l.sub(i, k, 0), cr);
        if (CPLX) l.s.st(l.sub(i, k, 1), ci);
    }
}

// store: out is L's element (c0, c0), ld = N.  Workgroup 0 writes the n x n diagonal block with +0 above the diagonal
// and in the diagonal's imaginary part; the workgroup of panel rows sub0 .. sub0 + m - 1 writes them and the +0 of the
// mirrored block above the diagonal (rows 0 .. n - 1, columns sub0 .. sub0 + m - 1): every element exactly once
template <typename T, bool CPLX, typename S, typename G>
BDSP_LA_HD void la_panel_store(const LaPanelLds<T, CPLX, S>& l, const G& out, size_t ld, int n, int m, size_t sub0, bool first,
                               int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    if (first) {
        for (int idx = tid; idx < n * LA_BLOCK; idx += LA_THREADS) {
            const int i = idx >> 6, j = idx & 63;
            if (j >= n) continue;
            const size_t g = ((size_t)i * ld + (size_t)j) * E;
            T re = (T)0, im = (T)0;
            if (j < i) { re = l.s.ld(l.tri(i, j, 0)); if (CPLX) im = l.s.ld(l.tri(i, j, 1)); }
            else if (j == i) re = l.s.ld(l.dia(i, m > 0));
            if (CPLX) out.st2(g, re, im);
            else out.st(g, re);
        }
    }
    for (int idx = tid; idx < m * LA_BLOCK; idx += LA_THREADS) {
        const int i = idx >> 6, j = idx & 63;
        if (j >= n) continue;
        const size_t g = ((sub0 + (size_t)i) * ld + (size_t)j) * E;
        if (CPLX) out.st2(g, l.s.ld(l.sub(i, j, 0)), l.s.ld(l.sub(i, j, 1)));
        else out.st(g, l.s.ld(l.sub(i, j, 0)));
    }
    for (int idx = tid; idx < n * LA_BLOCK; idx += LA_THREADS) { // the mirrored block: lanes along its columns
        const int i = idx >> 6, j = idx & 63;
        if (j >= m) continue;
        const size_t g = ((size_t)i * ld + sub0 + (size_t)j) * E;
        if (CPLX) out.st2(g, (T)0, (T)0);
        else out.st(g, (T)0);
    }
}

// ---------------------------------------------------------------------------------------------
// The diagonal solve: an n x n triangle (n <= NB) of L in LDS, padded to NB rows with the identity; one thread owns one
// column of B, NB unknowns in registers (rows from n on: +0, which the padding leaves +0), walks down the rows (forward,
// L x = b) or up (backward, L^H x = b), and writes its column of X.  Every LDS read is a broadcast.
// ---------------------------------------------------------------------------------------------
// lsrc is L's element (r0, r0) of the block, ld = N: only j <= i is read, of the diagonal the real part
template <typename T, bool CPLX, int NB, typename S, typename G>
BDSP_LA_HD void la_solve_load_l(const S& s, const G& lsrc, size_t ld, int n, int tid)
{
    constexpr int E = CPLX ? 2 : 1;
    for (int idx = tid; idx < NB * NB; idx += LA_THREADS) {
        const int i = idx / NB, j = idx % NB;
        if (j > i) continue;
        T re = i == j ? (T)1 : (T)0, im = (T)0;
        if (i < n) {
            const size_t g = ((size_t)i * ld + (size_t)j) * E;
            if (CPLX && i != j) lsrc.ld2(g, &re, &im);
            else re = lsrc.ld(g);
        }
        s.st(la_tri_slot(i, j) * E, re);
        if (CPLX) s.st(la_tri_slot(i, j) * E + 1, im);
    }
}

// The chain itself, written as two compile-time recursions so that every register index is a constant: a triangular loop
// nest is not unrolled in full by the compiler, and the unknowns would then live in scratch.  Row II (counted in the
// direction of the walk), steps KK .. II - 1, then the division.
template <typename T, bool CPLX, int NB, bool BACK, int II, int KK, typename S>
BDSP_LA_HD void la_solve_steps(const S& s, T (&xr)[NB], T (&xi)[NB])
{
    constexpr int E = CPLX ? 2 : 1, i = BACK ? NB - 1 - II : II;
    if constexpr (KK < II) {
        constexpr int k = BACK ? NB - 1 - KK : KK;
        constexpr int slot = (BACK ? (k * (k + 1) / 2 + i) : (i * (i + 1) / 2 + k)) * E; // la_tri_slot; backward: conj(L[k][i])
        const T lr = s.ld(slot);
        if (CPLX) la_cplx_sub<T>(lr, BACK ? -s.ld(slot + 1) : s.ld(slot + 1), xr[k], xi[k], &xr[i], &xi[i]);
        else xr[i] = la_fma<T>(-lr, xr[k], xr[i]);
        if ((KK & 3) == 3) BDSP_LA_SCHED_FENCE();
        la_solve_steps<T, CPLX, NB, BACK, II, KK + 1>(s, xr, xi);
    } else {
        const T d = s.ld((i * (i + 1) / 2 + i) * E);
        xr[i] = xr[i] / d;
        if (CPLX) xi[i] = xi[i] / d;
        BDSP_LA_PIN(xr[i]);
        if (CPLX) BDSP_LA_PIN(xi[i]);
        BDSP_LA_SCHED_FENCE();
    }
}
template <typename T, bool CPLX, int NB, bool BACK, int II, typename S>
BDSP_LA_HD void la_solve_rows(const S& s, T (&xr)[NB], T (&xi)[NB])
{
    if constexpr (II < NB) {
        la_solve_steps<T, CPLX, NB, BACK, II, 0>(s, xr, xi);
        la_solve_rows<T, CPLX, NB, BACK, II + 1>(s, xr, xi);
    }
}

// src / dst: row i of the block at (i * ld + col) * E
template <typename T, bool CPLX, int NB, bool BACK, typename S, typename GI, typename GO>
BDSP_LA_HD void la_solve_column(const S& s, const GI& src, const GO& dst, size_t ld, int n, size_t col)
{
    constexpr int E = CPLX ? 2 : 1;
    T xr[NB], xi[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        // no branch here: a row past n re-reads row n - 1 (n < NB only; from the cache) and keeps +0, so the unknowns
        // stay plain registers instead of values merged after every branch
        const size_t g = ((size_t)(i < n ? i : n - 1) * ld + col) * E;
        T re, im = (T)0;
        if (CPLX) src.ld2(g, &re, &im);
        else re = src.ld(g);
        xr[i] = i < n ? re : (T)0;
        xi[i] = i < n ? im : (T)0;
    }
    la_solve_rows<T, CPLX, NB, BACK, 0>(s, xr, xi);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        if (i < n) {
            const size_t g = ((size_t)i * ld + col) * E;
            if (CPLX) dst.st2(g, xr[i], xi[i]);
            else dst.st(g, xr[i]);
        }
    }
}

} // namespace bdsp
