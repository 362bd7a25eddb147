// iir_core.h -- the tile plan, the LDS map, the per-lane arithmetic, the scan tree with its table indices and the host
// tables of iir.hip, host + device: sosfilt, a cascade of second-order sections applied along every row.  The kernels call
// these functions with registers and cross-lane operations; tests/host_sim/sim_iir.cpp calls the SAME functions with
// threads as loops.
//
// One section, direct form II transposed (the form and state convention of scipy.signal.sosfilt), coefficients divided by
// a0 in double on the host and rounded once to T:
//     y = b0 x + s1,   s1 <- b1 x - a1 y + s2,   s2 <- b2 x - a2 y
// Every product-sum is one fma (iir_step); the lone product a2 y has nothing to contract with.  With x = 0 a step is
// s <- A s, A = [[-a1, 1], [-a2, 0]]: the state after a run of points from state s is A^len s + (the state after the same
// run from zero), an affine map whose linear part depends on the run's LENGTH alone.
//
// A row is cut into tiles of IIR_TILE points, a tile into 256 chunks of IIR_CHUNK points, one per lane.  Complex rows are
// two independent real signals (C = 2 channels) with the same coefficients.  Per section:
//   1. every lane runs its chunk from a zero state -- lane 0 from the tile's true incoming state -- and keeps only the end
//      state e;
//   2. the chunk maps s -> A^16 s + e are combined by a fixed tree: inside a wave the six Hillis-Steele steps
//      v_j += P_k v_(j - 2^k), j >= 2^k, with P_k = A^(16 * 2^k), k = 0 .. 5 (cross-lane moves); the four wave totals meet
//      in LDS, and the state entering wave q is the Horner chain in_q = P_6 in_(q-1) + W_(q-1) from in_1 = W_0;
//   3. the state entering lane j of wave q is v_(j-1) + A^(16 j) in_q, the power applied as the product of the P_k over
//      the set bits of j in ascending k (iir_advance): no table per lane;
//   4. THE LANE RE-RUNS ITS CHUNK FROM THAT TRUE STATE and the outputs replace the inputs in registers.  Re-running was
//      chosen over adding the homogeneous response h_j s from two 16-entry tables: a chunk's outputs are then exactly
//      the serial recurrence from the chunk's incoming state, so the blocked scheme's own error sits in 256 chunk states
//      per tile and nowhere else, the tables fall away, and the integrator and the pure FIR section stay exact where the
//      serial recurrence is.  It costs 5 fmas per point against 2 for the correction (the difference was not measured).
// The state after the row's last point is the re-run's state in the lane that owns that point (iir_last_lane): points past
// the end are loaded as zeros and can only reach lanes that own no point.
//
// Rows longer than a tile take three launches (iir_launches): the tile kernel from zero states on every tile but the last,
// storing each tile's 2S end states v_t; the carry kernel s_(t+1) = M s_t + v_t with M the (2S x 2S) transition of the
// whole cascade over IIR_TILE points, in double in both precisions, one wave per row and channel, lane i the component i
// (iir_carry_dot: ascending j from v_t[i]); the tile kernel again from the true states.  No workgroup waits for another.
// The result is a function of (row length, sos, number kind, precision, incoming state) only.
#pragma once

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define BDSP_IIR_HD __host__ __device__ __forceinline__
#else
#define BDSP_IIR_HD inline
#endif

namespace bdsp {

constexpr int IIR_THREADS = 256;
constexpr int IIR_WAVE = 64;
constexpr int IIR_WAVES = IIR_THREADS / IIR_WAVE;
constexpr int IIR_CHUNK = 16; // points per lane; with IIR_THREADS it makes the tile
// points per tile: 256 lanes x 16 points; a complex f64 tile is 64 KB of LDS
constexpr int IIR_TILE = 4096; // not measured: no other tile was built
// sections per call at most: the carry kernel holds the 2S state components in the lanes of half a wave
constexpr int IIR_MAX_SECTIONS = 16; // not measured (32 state components; M is 8 KB of LDS)
// end states the carry kernel requests ahead of its serial chain
constexpr int IIR_CARRY_BATCH = 8; // not measured
constexpr int IIR_IN_WAVE_STEPS = 6;              // 2^6 lanes
constexpr int IIR_POWERS = IIR_IN_WAVE_STEPS + 1; // P_k = A^(16 * 2^k), k = 0 .. 6; P_6 advances by one wave

static_assert(IIR_TILE == IIR_THREADS * IIR_CHUNK, "one chunk per lane");
static_assert(2 * IIR_MAX_SECTIONS <= IIR_WAVE, "one state component per lane of the carry kernel");

// one section as the kernels read it: b0 b1 b2 -a1 -a2 (divided by a0, rounded to T), then P_k row-major
template <typename T>
struct IirSec {
    T b0, b1, b2, na1, na2;
    T p[IIR_POWERS][4];
};

// ---------------------------------------------------------------------------------------------
// the plan: a function of the row length alone
// ---------------------------------------------------------------------------------------------
BDSP_IIR_HD size_t iir_tiles(size_t n) { return (n + IIR_TILE - 1) / IIR_TILE; }
BDSP_IIR_HD int iir_launches(size_t n) { return n == 0 ? 0 : (iir_tiles(n) == 1 ? 1 : 3); }
BDSP_IIR_HD int iir_tile_points(size_t n, size_t tile)
{
    const size_t left = n - tile * (size_t)IIR_TILE;
    return left < (size_t)IIR_TILE ? (int)left : IIR_TILE;
}
// the lane that owns the last of a tile's `points` (> 0) points, and how many points of its chunk exist
BDSP_IIR_HD int iir_last_lane(int points) { return (points - 1) / IIR_CHUNK; }
BDSP_IIR_HD int iir_last_count(int points) { return (points - 1) % IIR_CHUNK + 1; }
// doubles of the carry buffer: per row, tile and channel the 2S components
BDSP_IIR_HD size_t iir_carry_index(size_t row, size_t tiles, size_t tile, int C, int c, int S, int comp)
{
    return ((row * tiles + tile) * (size_t)C + (size_t)c) * (size_t)(2 * S) + (size_t)comp;
}
// scalars of a state operand: s1, s2 of section 0, then of section 1, ..., each a point (C scalars)
BDSP_IIR_HD size_t iir_state_index(size_t row, int C, int c, int S, int comp)
{
    return row * (size_t)(2 * S * C) + (size_t)comp * (size_t)C + (size_t)c;
}

// ---------------------------------------------------------------------------------------------
// LDS map (scalars of T).  Scalar g of the tile (point g / C, channel g % C) belongs to the chunk g / (16 C) and lands at
// chunk * (16 C + 1) + g % (16 C): an odd pitch, 17 (real) or 33 (complex), as ms_lds_stride.
//   chunk side (lane l reads / writes scalar j of its own chunk, address l * pitch + j):
//     f32: ds_read_b32 / ds_write_b32, bank (a / 4) % 32 per 32-lane half: l * odd mod 32 takes 32 distinct values over
//          32 consecutive lanes -- conflict-free.
//     f64: ds_read_b64, bank (a / 4) % 64 per 32-lane half: dwords 2 (l * odd mod 32), 32 distinct even banks, each lane
//          its pair; ds_write_b64, groups of 16 contiguous lanes at (a / 4) % 32: 2 (l * odd mod 16) -- conflict-free.
//   row side (lane t moves scalar 256 k + t, consecutive lanes consecutive scalars): a 32-lane group of a complex tile
//     lies inside one chunk (32 scalars): consecutive addresses, conflict-free.  A 32-lane group of a REAL tile spans two
//     chunks with the pad between them, 33 addresses for 32 lanes: the first and the last lane share a bank, ONE extra
//     cycle per group for b32 both ways and for ds_read_b64; ds_write_b64's 16-lane groups lie inside one chunk, none.
// sim_iir.cpp counts exactly this.  After the map: 2 slots (section parity) x 4 waves x 2 C scalars of wave totals.
// ---------------------------------------------------------------------------------------------
BDSP_IIR_HD int iir_lds_pitch(int C) { return IIR_CHUNK * C + 1; }
BDSP_IIR_HD int iir_lds_slot(int g, int C) { return (g / (IIR_CHUNK * C)) * iir_lds_pitch(C) + g % (IIR_CHUNK * C); }
BDSP_IIR_HD int iir_lds_chunk(int lane, int C) { return lane * iir_lds_pitch(C); }
BDSP_IIR_HD int iir_lds_map_scalars(int C) { return IIR_THREADS * iir_lds_pitch(C); }
BDSP_IIR_HD int iir_lds_total(int sec, int wave, int C, int c, int i)
{
    return iir_lds_map_scalars(C) + (((sec & 1) * IIR_WAVES + wave) * C + c) * 2 + i;
}
BDSP_IIR_HD int iir_lds_scalars(int C) { return iir_lds_map_scalars(C) + 2 * IIR_WAVES * C * 2; }

// ---------------------------------------------------------------------------------------------
// per-lane arithmetic
// ---------------------------------------------------------------------------------------------
BDSP_IIR_HD float iir_fma(float a, float b, float c) { return fmaf(a, b, c); }
BDSP_IIR_HD double iir_fma(double a, double b, double c) { return fma(a, b, c); }

// one point through one section
template <typename T>
BDSP_IIR_HD T iir_step(const IirSec<T>& s, T x, T* s1, T* s2)
{
    const T y = iir_fma(s.b0, x, *s1);
    *s1 = iir_fma(s.b1, x, iir_fma(s.na1, y, *s2));
    *s2 = iir_fma(s.b2, x, s.na2 * y);
    return y;
}

// (r1, r2) = P (v1, v2) + (a1, a2), P row-major
template <typename T>
BDSP_IIR_HD void iir_affine(const T* p, T v1, T v2, T a1, T a2, T* r1, T* r2)
{
    *r1 = iir_fma(p[0], v1, iir_fma(p[1], v2, a1));
    *r2 = iir_fma(p[2], v1, iir_fma(p[3], v2, a2));
}
// (r1, r2) = P (v1, v2)
template <typename T>
BDSP_IIR_HD void iir_linear(const T* p, T v1, T v2, T* r1, T* r2)
{
    *r1 = iir_fma(p[0], v1, p[1] * v2);
    *r2 = iir_fma(p[2], v1, p[3] * v2);
}

// step k of the in-wave tree for lane j: (f1, f2) is lane j - 2^k's value before the step
BDSP_IIR_HD bool iir_scan_takes(int j, int k) { return j >= (1 << k); }
template <typename T>
BDSP_IIR_HD void iir_scan_step(const IirSec<T>& s, int k, int j, T f1, T f2, T* v1, T* v2)
{
    if (iir_scan_takes(j, k)) iir_affine<T>(s.p[k], f1, f2, *v1, *v2, v1, v2);
}

// the state entering wave q >= 1 from the totals w[2 p], w[2 p + 1] of the waves p < q, `stride` scalars apart
template <typename T>
BDSP_IIR_HD void iir_wave_in(const IirSec<T>& s, const T* w, int stride, int q, T* r1, T* r2)
{
    T a = w[0], b = w[1];
    for (int p = 1; p < q; ++p) iir_affine<T>(s.p[IIR_POWERS - 1], a, b, w[p * stride], w[p * stride + 1], &a, &b);
    *r1 = a;
    *r2 = b;
}

// A^(16 j) (v1, v2), j < 64: the P_k of the set bits of j, ascending k
template <typename T>
BDSP_IIR_HD void iir_advance(const IirSec<T>& s, int j, T* v1, T* v2)
{
    for (int k = 0; k < IIR_IN_WAVE_STEPS; ++k)
        if ((j >> k) & 1) iir_linear<T>(s.p[k], *v1, *v2, v1, v2);
}

// the state entering lane j of wave q: ex the value of lane j - 1 after the tree (anything for j == 0), in the wave's
// incoming state (anything for q == 0), s0 the tile's incoming state
template <typename T>
BDSP_IIR_HD void iir_lane_in(const IirSec<T>& s, int q, int j, T ex1, T ex2, T in1, T in2, T s01, T s02, T* r1, T* r2)
{
    if (q == 0) {
        *r1 = j == 0 ? s01 : ex1;
        *r2 = j == 0 ? s02 : ex2;
        return;
    }
    iir_advance<T>(s, j, &in1, &in2);
    *r1 = j == 0 ? in1 : ex1 + in1;
    *r2 = j == 0 ? in2 : ex2 + in2;
}

// component i of M s + v: mt is M transposed (mt[j * n2 + i] = M[i][j], lanes along i: consecutive banks), M is block
// lower triangular, so the sum stops at the component's own section
BDSP_IIR_HD double iir_carry_dot(const double* mt, const double* s, int n2, int i, double v)
{
    double acc = v;
    for (int j = 0; j <= (i | 1); ++j) acc = fma(mt[j * n2 + i], s[j], acc);
    return acc;
}

// ---------------------------------------------------------------------------------------------
// host tables (host code only), in long double from the coefficients AS ROUNDED to T.  False for a0 == 0 or a coefficient that is not
// finite.  m (may be null): the (2S x 2S) transition of the cascade over IIR_TILE points, row-major.
// ---------------------------------------------------------------------------------------------
inline bool iir_sos_valid(const double* sos, size_t S)
{
    for (size_t k = 0; k < S; ++k) {
        for (int i = 0; i < 6; ++i)
            if (!(fabs(sos[6 * k + i]) <= 1.7976931348623157e308)) return false;
        if (sos[6 * k + 3] == 0.0) return false;
    }
    return true;
}

inline void iir_mat_mul(const long double* a, const long double* b, long double* c, int n)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            long double acc = 0;
            for (int k = 0; k < n; ++k) acc += a[i * n + k] * b[k * n + j];
            c[i * n + j] = acc;
        }
}

template <typename T>
inline void iir_make_tables(const double* sos, size_t S, IirSec<T>* tab, double* m)
{
    for (size_t k = 0; k < S; ++k) {
        const double* c = sos + 6 * k;
        IirSec<T>& t = tab[k];
        t.b0 = (T)(c[0] / c[3]);
        t.b1 = (T)(c[1] / c[3]);
        t.b2 = (T)(c[2] / c[3]);
        t.na1 = -(T)(c[4] / c[3]);
        t.na2 = -(T)(c[5] / c[3]);
        long double p[4] = {(long double)t.na1, 1.0L, (long double)t.na2, 0.0L}, q[4];
        for (int sq = 0; sq < 4; ++sq) { // A^16
            iir_mat_mul(p, p, q, 2);
            for (int i = 0; i < 4; ++i) p[i] = q[i];
        }
        for (int e = 0; e < IIR_POWERS; ++e) {
            for (int i = 0; i < 4; ++i) t.p[e][i] = (T)p[i];
            iir_mat_mul(p, p, q, 2);
            for (int i = 0; i < 4; ++i) p[i] = q[i];
        }
    }
    if (!m || !S) return;
    // one step of the cascade with input 0, column by column, then 12 squarings
    const int n2 = 2 * (int)S;
    long double *f = new long double[3 * (size_t)n2 * n2], *g = f + (size_t)n2 * n2, *st = g + (size_t)n2 * n2;
    for (int col = 0; col < n2; ++col) {
        for (int i = 0; i < n2; ++i) st[i] = i == col ? 1.0L : 0.0L;
        long double u = 0.0L;
        for (size_t k = 0; k < S; ++k) {
            const IirSec<T>& t = tab[k];
            const long double y = (long double)t.b0 * u + st[2 * k];
            f[(2 * k) * n2 + col] = (long double)t.b1 * u + (long double)t.na1 * y + st[2 * k + 1];
            f[(2 * k + 1) * n2 + col] = (long double)t.b2 * u + (long double)t.na2 * y;
            u = y;
        }
    }
    int steps = 0;
    for (int len = IIR_TILE; len > 1; len >>= 1) ++steps;
    for (int sq = 0; sq < steps; ++sq) {
        iir_mat_mul(f, f, g, n2);
        for (int i = 0; i < n2 * n2; ++i) f[i] = g[i];
    }
    for (int i = 0; i < n2 * n2; ++i) m[i] = (double)f[i];
    delete[] f;
}

} // namespace bdsp
