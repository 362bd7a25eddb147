// mat_interp_core.h -- what the matrix unit mat_interp.hip shares with the vector unit interp.hip and with the host
// simulation (tests/host_sim/sim_mat_interp.cpp), host + device:
//   * the per-output arithmetic of interpolate_lin / interpolate_hermite and the host computation of the Hermite
//     regions -- interp.hip (k_interp_lin, k_interp_hermite) and mat_interp.hip (k_mt_interp_*) compile the SAME
//     expressions, so a row of a matrix is bit-equal to the vector call on that row (both objects are built without
//     FMA contraction);
//   * the flat output index -> (row, position) map of the batched interpolation kernels;
//   * the tiling and staging maps of the batched direct circular convolution k_mt_conv_direct.
#pragma once

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define BDSP_MT_HD __host__ __device__ __forceinline__
#else
#define BDSP_MT_HD inline
#endif

namespace bdsp {

// ---------------------------------------------------------------------------------------------
// interpolate_lin / interpolate_hermite (time_freq/real_interpolation.rs:33-176), one output each
// ---------------------------------------------------------------------------------------------
BDSP_MT_HD float mt_floor(float x) { return floorf(x); }
BDSP_MT_HD double mt_floor(double x) { return floor(x); }

template <typename T>
BDSP_MT_HD T mt_clamped(const T* x, long long len, long long i)
{
    i = i < 0 ? 0 : (i >= len ? len - 1 : i);
    return x[i];
}

// output n of dest_len from the `len` samples at `in`
template <typename T>
BDSP_MT_HD T interp_lin_value(const T* in, long long len, long long dest_len, long long n, T factor, T delay)
{
    if (n == dest_len - 1) return in[len - 1]; // :68
    T rounded = (T)n / factor + delay;
    T beforef = mt_floor(rounded);
    long long before = (long long)beforef;
    T y0 = mt_clamped(in, len, before), y1 = mt_clamped(in, len, before + 1);
    return y0 + (y1 - y0) * (rounded - beforef);
}

// outputs below `start` extrapolate the point before the first sample, outputs from `tail` on the points behind the last
template <typename T>
BDSP_MT_HD T interp_hermite_value(const T* in, long long len, long long n, T factor, T delay, long long start,
                                  long long tail)
{
    const T half = (T)0.5, c15 = (T)1.5, two = (T)2, c25 = (T)2.5;
    T rounded = (T)n / factor + delay;
    T beforef = mt_floor(rounded);
    long long before = (long long)beforef;
    T x = rounded - beforef;
    T y0, y1, y2, y3;
    if (n < start) { // :103-124
        y1 = mt_clamped(in, len, before); y2 = mt_clamped(in, len, before + 1); y3 = mt_clamped(in, len, before + 2);
        y0 = y1 - (y2 - y1);
    } else if (n < tail) { // :126-145
        y0 = mt_clamped(in, len, before - 1); y1 = mt_clamped(in, len, before);
        y2 = mt_clamped(in, len, before + 1); y3 = mt_clamped(in, len, before + 2);
    } else { // :147-172
        y0 = mt_clamped(in, len, before - 1); y1 = mt_clamped(in, len, before);
        y2 = (before >= 0 && before < len - 1) ? in[before + 1] : y1 + (y1 - y0);
        y3 = (before >= 0 && before + 2 < len) ? in[before + 2] : y2 + (y2 - y1);
    }
    T x2 = x * x;
    T a0 = -half * y0 + c15 * y1 - c15 * y2 + half * y3;
    T a1 = y0 - c25 * y1 + two * y2 - half * y3;
    T a2 = -half * y0 + half * y2;
    T a3 = y1;
    return (a0 * x * x2) + (a1 * x2) + (a2 * x) + a3;
}

// the regions of interp_hermite_value for dest_len outputs (host)
template <typename T>
inline void interp_hermite_regions(size_t dest_len, T factor, T delay, long long* start_out, long long* tail_out)
{
    T st = ((T)1 - delay) * factor;
    double c = sizeof(T) == 4 ? (double)ceilf((float)st) : ceil((double)st);
    long long start = c < 0 ? 0 : (long long)c, end = start + 1;
    if (start > (long long)dest_len) start = (long long)dest_len;
    long long tail = (long long)dest_len > end ? (long long)dest_len - end : 0;
    if (tail < start) tail = start;
    *start_out = start;
    *tail_out = tail;
}

// ---------------------------------------------------------------------------------------------
// batched interpolation: one lane per element of the flat output [rows][dest_len], grid-stride
// ---------------------------------------------------------------------------------------------
template <typename IDX>
BDSP_MT_HD void mt_flat_pos(IDX flat, IDX dest_len, IDX* row, IDX* n)
{
    const IDX r = flat / dest_len;
    *row = r;
    *n = flat - r * dest_len;
}

// 32-bit indices while every flat index of input and output plus one grid stride stays below 2^32
inline bool mt_fits_32(size_t in_total, size_t out_total) { return in_total < (size_t(1) << 31) && out_total < (size_t(1) << 31); }

// ---------------------------------------------------------------------------------------------
// batched direct circular convolution  y[r][i] = sum_{k=0}^{2L} x[r][(i - L + k) mod N] * w[k]
//
// A workgroup of MT_WG lanes works on one "virtual block" after the other (grid-stride).  Virtual block vb owns
// `rpb` whole rows (rows shorter than the workgroup: tile == N, tiles_per_row == 1) or one tile of `tile` outputs of
// one row.  Per owned row ("segment") it stages x[(start - L + j) mod N], j < cnt + 2L, at LDS element
// seg * seg_stride + j; output i of the tile then reads elements seg * seg_stride + i + k, k = 0 .. 2L.  Lane t
// computes the block-local outputs t + MT_WG * u, u < per.
// ---------------------------------------------------------------------------------------------
constexpr unsigned MT_WG = 256;
// the staged kernel holds positions within a row in 32 bits: m0 + j < N + tile + 2L <= 3N + 1024
constexpr unsigned long long MT_STAGED_MAX_POINTS = 1ull << 30;

struct MtConvGeom {
    unsigned long long rows, n, l; // rows, points per row, L (already clipped to n)
    unsigned long long nblocks;    // virtual blocks
    unsigned tile, rpb, tiles_per_row, per;
    unsigned seg_stride;           // LDS elements per segment: tile + 2L
    unsigned x_scalars;            // scalars of the staged rows (even), the weights follow
    bool staged;
    size_t lds_bytes;
};

// elem = scalars per element (2: complex rows), welem = scalars per weight (2: complex weights)
inline MtConvGeom mt_conv_geom(size_t rows, size_t n, size_t l, unsigned elem, unsigned welem, size_t scalar_bytes,
                               size_t lds_budget)
{
    MtConvGeom g = {};
    g.rows = rows; g.n = n; g.l = l;
    g.staged = false;
    g.per = 1; g.rpb = 1; g.tile = MT_WG; g.tiles_per_row = 1;
    if (rows == 0 || n == 0) return g;
    // staged if the rows of a virtual block with their halos and the weights fit the budget
    auto fit = [&](unsigned tile, unsigned rpb, unsigned per) {
        const unsigned long long seg = (unsigned long long)tile + 2ull * l;
        unsigned long long xs = seg * rpb * elem;
        xs += xs & 1;
        const unsigned long long bytes = (xs + (2ull * l + 1) * welem) * scalar_bytes;
        if (bytes > lds_budget) return false;
        g.staged = true;
        g.tile = tile; g.rpb = rpb; g.per = per;
        g.seg_stride = (unsigned)seg;
        g.x_scalars = (unsigned)xs;
        g.lds_bytes = (size_t)bytes;
        return true;
    };
    if (n < MT_WG) fit((unsigned)n, MT_WG / (unsigned)n, 1);                   // whole short rows
    else if (n < MT_STAGED_MAX_POINTS) {
        if (n < 3 * MT_WG || !fit(4 * MT_WG, 1, 4)) fit(MT_WG, 1, 1);         // four outputs per lane, or one
    }
    if (!g.staged) { // global reads with the modular index: tiles of one workgroup, or whole short rows
        g.tile = n < MT_WG ? (unsigned)n : MT_WG;
        g.rpb = n < MT_WG ? MT_WG / g.tile : 1;
        g.per = 1;
        g.seg_stride = 0; g.x_scalars = 0; g.lds_bytes = 0;
    }
    g.tiles_per_row = (unsigned)((n + g.tile - 1) / g.tile);
    g.nblocks = ((rows + g.rpb - 1) / g.rpb) * g.tiles_per_row;
    return g;
}

// virtual block -> its first row, the first output of its tile and the outputs of the tile that exist
BDSP_MT_HD void mt_conv_block(const MtConvGeom& g, unsigned long long vb, unsigned long long* row0, unsigned* start,
                              unsigned* cnt)
{
    const unsigned long long rg = vb / g.tiles_per_row;
    const unsigned t = (unsigned)(vb - rg * g.tiles_per_row);
    *row0 = rg * g.rpb;
    *start = t * g.tile;
    const unsigned long long left = g.n - (unsigned long long)t * g.tile;
    *cnt = left < g.tile ? (unsigned)left : g.tile;
}

// segments of a virtual block that are rows of the matrix
BDSP_MT_HD unsigned mt_conv_segments(const MtConvGeom& g, unsigned long long row0)
{
    const unsigned long long left = g.rows - row0;
    return left < g.rpb ? (unsigned)left : g.rpb;
}

// block-local output j -> segment and output within the tile; false: no such output
BDSP_MT_HD bool mt_conv_out(const MtConvGeom& g, unsigned j, unsigned nseg, unsigned cnt, unsigned* seg, unsigned* i)
{
    const unsigned s = j / g.tile;
    *seg = s;
    *i = j - s * g.tile;
    return s < nseg && *i < cnt;
}

// source point of staged element 0 of a tile: (start - L) mod N, L <= N
BDSP_MT_HD unsigned mt_conv_first_src(const MtConvGeom& g, unsigned start)
{
    return (unsigned)(((unsigned long long)start + g.n - g.l) % g.n);
}

// source point of staged element j (2L + 1 may exceed N: the window wraps more than once)
BDSP_MT_HD unsigned mt_conv_src(unsigned first_src, unsigned j, unsigned n) { return (first_src + j) % n; }

} // namespace bdsp
