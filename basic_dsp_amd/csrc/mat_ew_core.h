// mat_ew_core.h -- what mat_ew.hip shares with the vector unit elementwise.hip and with the host simulation
// (tests/host_sim/sim_mat_ew.cpp), host + device:
//   * the per-element arithmetic of multiply_complex_exponential -- elementwise.hip's OpMulCexp (the vector's kernel) and
//     mat_ew.hip compile the SAME expressions, so a row of a matrix is bit-equal to the vector call on that row (both
//     objects are built without FMA contraction) -- and of the wrap-around binary operations;
//   * the lane -> (row, position) map of the shared-phasor mixer k_mw_cexp;
//   * the flat element walk of k_mw_reverse and k_mw_smaller: one divide per lane, the position in the row, the row and
//     the operand's period are carried from one grid stride to the next.
#pragma once

#ifndef _GNU_SOURCE
#define _GNU_SOURCE // sincos on the host
#endif
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define BDSP_MW_HD __host__ __device__ __forceinline__
#else
#define BDSP_MW_HD inline
#endif

namespace bdsp {

// ---------------------------------------------------------------------------------------------
// multiply_complex_exponential (complex_ops.rs:81-105): z[k] *= exp(j (a k + b)), a and b already multiplied by delta.
// The reference advances a running product per element, whose error grows with the index; here every position gets its
// own phase, reduced in double, so the result is at least as close to the exact value (compared with tolerance).
// ---------------------------------------------------------------------------------------------
// the phasor of position k: the phase in double, then rounded to T
template <typename T>
BDSP_MW_HD void cexp_phasor(double a, double b, double k, T* wr, T* wi)
{
    double s, c;
    sincos(a * k + b, &s, &c);
    *wr = (T)c;
    *wi = (T)s;
}

// (zr, zi) *= (wr, wi), every product and sum rounded on its own (num-complex Mul)
template <typename T>
BDSP_MW_HD void cexp_mul(T* zr, T* zi, T wr, T wi)
{
    const T re = *zr, im = *zi;
    *zr = re * wr - im * wi;
    *zi = re * wi + im * wr;
}

// ---------------------------------------------------------------------------------------------
// add_smaller / sub_smaller / mul_smaller / div_smaller (elementary.rs:591-640): op 0 .. 3
// ---------------------------------------------------------------------------------------------
template <typename T>
BDSP_MW_HD T smaller_real(T a, T b, int op)
{
    return op == 0 ? a + b : (op == 1 ? a - b : (op == 2 ? a * b : a / b));
}

template <typename T>
BDSP_MW_HD void smaller_complex(T ar, T ai, T br, T bi, int op, T* re, T* im)
{
    if (op == 0) { *re = ar + br; *im = ai + bi; }
    else if (op == 1) { *re = ar - br; *im = ai - bi; }
    else if (op == 2) { *re = ar * br - ai * bi; *im = ar * bi + ai * br; }
    else { T nn = br * br + bi * bi; *re = (ar * br + ai * bi) / nn; *im = (ai * br - ar * bi) / nn; } // num-complex Div
}

// ---------------------------------------------------------------------------------------------
// k_mw_cexp: a workgroup of MW_WG lanes owns a tile of MW_WG consecutive points of the row (blockIdx.x) and walks down
// the row groups blockIdx.y, blockIdx.y + gridDim.y, ...; rows shorter than the workgroup share it, `rps` side by
// side, and a row group is `rps` consecutive rows.  A lane keeps its position, so it forms its phasor once.
// ---------------------------------------------------------------------------------------------
constexpr unsigned MW_WG = 256;

struct MwCexpGeom {
    unsigned long long rows, points; // complex points per row
    unsigned long long row_groups;   // ceil(rows / rps)
    unsigned long long tiles_per_row;
    unsigned rps;                    // rows side by side in a workgroup
};

inline MwCexpGeom mw_cexp_geom(size_t rows, size_t points)
{
    MwCexpGeom g = {};
    g.rows = rows; g.points = points;
    g.rps = 1; g.tiles_per_row = 1;
    if (rows == 0 || points == 0) return g;
    if (points < MW_WG) g.rps = MW_WG / (unsigned)points;
    else g.tiles_per_row = (points + MW_WG - 1) / MW_WG;
    g.row_groups = (rows + g.rps - 1) / g.rps;
    return g;
}

// lane of tile `tile` -> the row of its group (sub) and its position in the row (k); false: the lane has no point
BDSP_MW_HD bool mw_cexp_lane(const MwCexpGeom& g, unsigned long long tile, unsigned lane, unsigned* sub,
                             unsigned long long* k)
{
    if (g.points < MW_WG) {
        const unsigned p = (unsigned)g.points, s = lane / p;
        *sub = s;
        *k = lane - s * p;
        return s < g.rps;
    }
    *sub = 0;
    *k = tile * MW_WG + lane;
    return *k < g.points;
}

// row of a lane in row group rg; the caller checks it against g.rows
BDSP_MW_HD unsigned long long mw_cexp_row(const MwCexpGeom& g, unsigned long long rg, unsigned sub)
{
    return rg * g.rps + sub;
}

// ---------------------------------------------------------------------------------------------
// k_mw_reverse / k_mw_smaller: lane -> flat element o of [rows][points], then o += stride (grid-stride).  The row r and
// the position i come from ONE divide per lane and are carried; stride = s_r * points + s_i is split on the host.
// ---------------------------------------------------------------------------------------------
template <typename IDX>
BDSP_MW_HD void mw_flat_start(IDX o, IDX points, IDX* r, IDX* i)
{
    const IDX q = o / points;
    *r = q;
    *i = o - q * points;
}

template <typename IDX>
BDSP_MW_HD void mw_flat_step(IDX points, IDX s_r, IDX s_i, IDX* r, IDX* i)
{
    *r += s_r;
    *i += s_i; // i + s_i < 2 * points
    if (*i >= points) { *i -= points; ++*r; }
}

// reverse: the element that lands at flat index o = r * points + i is r * points + (points - 1 - i)
template <typename IDX>
BDSP_MW_HD IDX mw_reverse_src(IDX o, IDX points, IDX i) { return (o - i) + (points - 1 - i); }

// the operand's period: j = i mod ypoints = o mod ypoints (ypoints divides points), carried with s_j = stride mod ypoints
template <typename IDX>
BDSP_MW_HD IDX mw_period_step(IDX j, IDX s_j, IDX ypoints)
{
    j += s_j;
    return j >= ypoints ? j - ypoints : j;
}

// operand element of row r, period position j: rows ystride elements apart (0: one vector for every row)
template <typename IDX>
BDSP_MW_HD IDX mw_operand_index(IDX r, IDX ystride, IDX j) { return r * ystride + j; }

// 32-bit indices while every flat index plus one grid stride and 2 * points stay below 2^32
inline bool mw_fits_32(size_t total, size_t operand_total)
{
    return total < (size_t(1) << 31) && operand_total < (size_t(1) << 31);
}

} // namespace bdsp
