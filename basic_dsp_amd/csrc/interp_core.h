// interp_core.h -- the index maps of interpolatef's kernels (interp.hip), for one vector and for the rows of a matrix.
//
// Plain integer arithmetic, compiled by hipcc for the kernels and their launchers and by g++ for the host simulation
// (tests/host_sim/sim_mat_interpf.cpp), which runs the kernels' loops over these maps with threads as loops.
//
// A matrix is `rows` equally long rows back to back; everything below is RELATIVE TO ONE ROW (the kernels add the row's
// base, row * points and row * new_points elements, once per virtual block or per output), so a vector is the one-row
// case and wrap-around never leaves a row.
//
//   integer path  a row's outputs are the inner region [f * q_lo, f * q_hi) -- tiles of `tile` input positions for the
//                 blocked kernel -- and the two edge runs around it, walked by `edge_blocks` workgroups of 256 lanes.
//                 Virtual block vb of rows * (inner_blocks + edge_blocks) is (row, k) = (vb / per_row, vb % per_row):
//                 k < inner_blocks is tile k, the others are edge workgroup k - inner_blocks.  The grid is flat and
//                 capped; a workgroup walks its virtual blocks with the grid's stride.
//   scalar paths  a lane owns the flat output g of rows * new_points, (row, i) = (g / new_points, g % new_points) by
//                 one division (if_pos), and moves on by the grid's stride with two adds and a compare (if_advance).
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define BDSP_IF_HD __host__ __device__ __forceinline__
#else
#define BDSP_IF_HD inline
#endif

namespace bdsp {

constexpr unsigned IF_WG = 256; // lanes per workgroup of every interpolatef kernel

// ------------------------------------------------------------------------------------------------ integer path
struct IfGeom {
    long long points, new_points; // of one row
    int conv_len, factor, ntaps;
    long long scalar_len;  // ntaps * factor: the reference's edge length
    long long q_lo, q_hi;  // input positions whose `factor` outputs are all inner outputs
    bool blocked;          // the blocked kernel takes [factor * q_lo, factor * q_hi), the table path the rest
    unsigned tile;         // input positions per tile of the blocked kernel
    unsigned inner_blocks; // tiles per row (0 unless blocked)
    unsigned edge_blocks;  // workgroups per row on the table path
};

// has_blocked: the factor has a blocked instantiation (2, 3, 4, 8); edge_cap: most workgroups per row on the table path
BDSP_IF_HD IfGeom if_geom(long long points, long long new_points, int conv_len, int factor, unsigned tile, bool has_blocked,
                          unsigned edge_cap)
{
    IfGeom g;
    g.points = points;
    g.new_points = new_points;
    g.conv_len = conv_len;
    g.factor = factor;
    g.ntaps = 2 * conv_len + 1;
    g.scalar_len = (long long)g.ntaps * factor;
    g.q_lo = (g.scalar_len + factor - 1) / factor;   // first q with f*q >= scalar_len
    g.q_hi = (new_points - g.scalar_len) / factor;   // f*q + f - 1 < new_points - scalar_len
    g.blocked = has_blocked && g.q_hi > g.q_lo && new_points >= 2 * g.scalar_len;
    g.tile = tile;
    g.inner_blocks = g.blocked ? (unsigned)((g.q_hi - g.q_lo + (long long)tile - 1) / (long long)tile) : 0u;
    const long long edge_outputs = g.blocked ? new_points - (g.q_hi - g.q_lo) * factor : new_points;
    long long eb = (edge_outputs + IF_WG - 1) / IF_WG;
    if (eb > (long long)edge_cap) eb = edge_cap;
    if (eb < 1) eb = 1;
    g.edge_blocks = (unsigned)eb;
    return g;
}

// virtual block -> (row, block of the row): one division per virtual block
BDSP_IF_HD void if_block(size_t vb, unsigned per_row, size_t* row, unsigned* k)
{
    const size_t r = vb / per_row;
    *row = r;
    *k = (unsigned)(vb - r * per_row);
}

// the table path walks the outputs outside [skip_lo, skip_hi) (all of them when that range is empty) as slots
// 0 .. new_points - nskip: slot -> output
BDSP_IF_HD long long if_skip_count(long long skip_lo, long long skip_hi) { return skip_hi > skip_lo ? skip_hi - skip_lo : 0; }
BDSP_IF_HD long long if_edge_output(long long slot, long long skip_lo, long long nskip)
{
    return (nskip && slot >= skip_lo) ? slot + nskip : slot;
}
// the reference's edge test (interpolate_priv_simd :191-290): the wrap-around form for these outputs
BDSP_IF_HD bool if_is_edge(long long i, long long scalar_len, long long new_points)
{
    return i < scalar_len || i + scalar_len >= new_points || new_points < 2 * scalar_len;
}
// edge output i reads x[(pos + 1 + m) mod points], m = 0 .. 2L, from pos = (i / f - L) mod points
BDSP_IF_HD long long if_edge_start(long long i, int factor, int conv_len, long long points)
{
    long long pos = (i / factor - conv_len) % points;
    if (pos < 0) pos += points;
    return pos;
}
BDSP_IF_HD long long if_wrap_next(long long pos, long long points) { return pos + 1 < points ? pos + 1 : 0; }
// inner output i reads x[end - 1 - m], m = 2L .. 0, with tap vector `shift`
BDSP_IF_HD long long if_inner_end(long long i, int factor, int conv_len) { return (i + factor - 1) / factor + conv_len; }
BDSP_IF_HD int if_inner_shift(long long i, int factor) { return (int)((factor - i % factor) % factor); }

// tile k of a row: positions [q0, q0 + nq), its x window x[xbase .. xbase + span) (read as 0 past the row's end)
BDSP_IF_HD long long if_tile_q0(const IfGeom& g, unsigned k) { return g.q_lo + (long long)k * g.tile; }
BDSP_IF_HD long long if_tile_nq(long long q0, long long q_hi, unsigned tile)
{
    const long long nq = q_hi - q0;
    return nq > (long long)tile ? (long long)tile : nq;
}
BDSP_IF_HD long long if_tile_xbase(long long q0, int conv_len) { return q0 - conv_len - 1; }
BDSP_IF_HD int if_tile_span(unsigned tile, int conv_len) { return (int)tile + 2 * conv_len + 2; }

// output staging of a tile in 16-byte packets: thread q hands over PP packets, `part` of them kept in slot
// PP * q + ((part + rot(q)) mod PP) for a power-of-two PP (eight consecutive lanes then cover eight different bank groups,
// see interp_inner_tile) and in PP * q + part otherwise
BDSP_IF_HD int if_rot(int q, int pp) { return pp >= 8 ? (q & (pp - 1)) : (pp > 1 ? ((q / (8 / (pp > 1 ? pp : 1))) & (pp - 1)) : 0); }
BDSP_IF_HD int if_lo_slot(int q, int part, int pp)
{
    const bool pow2 = (pp & (pp - 1)) == 0;
    return pp * q + (pow2 ? ((part + if_rot(q, pp)) & (pp - 1)) : part);
}

// ------------------------------------------------------------------------------------------------ scalar paths
template <typename IDX>
struct IfPos {
    IDX row, col;
};

template <typename IDX>
BDSP_IF_HD IfPos<IDX> if_pos(IDX flat, IDX width)
{
    const IDX row = flat / width;
    return IfPos<IDX>{row, flat - row * width};
}

template <typename IDX>
BDSP_IF_HD void if_advance(IfPos<IDX>* at, IfPos<IDX> step, IDX width)
{
    at->row += step.row;
    at->col += step.col; // < 2 * width: no wrap in IDX while 2 * width fits (if_fits_32 sees to it)
    if (at->col >= width) { at->col -= width; ++at->row; }
}

// 32-bit indices while every flat extent (scalars in, scalars out, and the walk's row + stride overshoot) is below 2^31
BDSP_IF_HD bool if_fits_32(size_t in_scalars, size_t out_scalars, size_t rows, size_t stride)
{
    const size_t lim = (size_t)1 << 31;
    return in_scalars < lim && out_scalars < lim && out_scalars + stride < lim && rows + stride < lim;
}

// wrap start of the scalar paths: output i of a row reads x[(p0 + 1 + k) mod points], k = 0 .. 2L
BDSP_IF_HD long long if_scalar_start(long long rounded, int conv_len, long long points)
{
    long long p0 = (rounded - conv_len - 1) % points;
    if (p0 < 0) p0 += points;
    return p0;
}
// the fast path of the packed kernel reads x[p0 + 1 .. p0 + ntaps] through one base pointer: only when that stays in the row
BDSP_IF_HD bool if_frac_wraps(long long p0, int ntaps, long long points) { return p0 + ntaps >= points; }

} // namespace bdsp
