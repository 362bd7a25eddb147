// mat_frame_core.h -- index maps and lane loops of mat_frame.hip, host + device: the shapes of from_frames and
// overlap_add, the flat walk every kernel shares (one divide per lane, then adds and one compare per element), the
// sources of the framing, overlap-add, zero-pad and rotate moves, and the loops themselves as functions of a lane's
// first flat index and the grid stride.  The kernels call the loops with raw pointers; tests/host_sim/sim_mat_frame.cpp
// calls the SAME functions with bounds-checking arrays and threads as loops.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define BDSP_MF_HD __host__ __device__ __forceinline__
#else
#define BDSP_MF_HD inline
#endif

namespace bdsp {

// ---------------------------------------------------------------------------------------------
// shapes (in points; a complex point is one element)
// ---------------------------------------------------------------------------------------------
// from_frames: frames of F points, H apart, of a signal of P points (F, H > 0).  Without pad_tail only whole frames;
// with it the tail gets a last, zero-extended frame, so every input point lies in a frame.
inline size_t mf_frame_rows(size_t P, size_t F, size_t H, bool pad_tail)
{
    if (!pad_tail) return P >= F ? (P - F) / H + 1 : 0;
    if (P == 0) return 0;
    return P > F ? (P - F) / H + ((P - F) % H ? 1 : 0) + 1 : 1; // ceil((P - F) / H) + 1
}

// overlap_add: rows of F points, H apart
inline size_t mf_ola_points(size_t rows, size_t F, size_t H) { return rows ? (rows - 1) * H + F : 0; }

// ---------------------------------------------------------------------------------------------
// the flat walk: a lane's place in a [.., width] layout.  Set once from the flat index (the one division a lane does),
// then moved by the grid stride -- split the same way, once -- with adds and one compare.
// ---------------------------------------------------------------------------------------------
template <typename IDX>
struct MfPos {
    IDX row, col;
};

template <typename IDX>
BDSP_MF_HD MfPos<IDX> mf_pos(IDX flat, IDX width)
{
    const IDX row = flat / width;
    return MfPos<IDX>{row, flat - row * width};
}

template <typename IDX>
BDSP_MF_HD void mf_advance(MfPos<IDX>* at, MfPos<IDX> step, IDX width)
{
    at->row += step.row;
    at->col += step.col; // < 2 * width: no wrap in IDX while 2 * width fits (the launchers see to it)
    if (at->col >= width) { at->col -= width; ++at->row; }
}

// ---------------------------------------------------------------------------------------------
// sources
// ---------------------------------------------------------------------------------------------
// from_frames: point j of frame r is x[r * H + j]; at or past P it reads as zero (the caller compares)
template <typename IDX>
BDSP_MF_HD IDX mf_frame_src(IDX r, IDX j, IDX H) { return r * H + j; }

// overlap_add: output i = q * H + rem (rem < H) sums m[r][i - r * H] over the rows r0 .. r1 (none if r0 > r1):
// r1 = min(q, rows - 1); below it every row whose offset rem + (q - r) * H is still < F.  rows > 0.
template <typename IDX>
BDSP_MF_HD void mf_ola_rows(IDX q, IDX rem, IDX rows, IDX F, IDX H, IDX* r0, IDX* r1)
{
    *r1 = q < rows ? q : rows - 1;
    if (rem >= F) { *r0 = *r1 + 1; return; } // a gap between frames (H > F)
    const IDX back = H >= F ? 0 : (F - 1 - rem) / H; // rows below q that still reach i
    *r0 = q > back ? q - back : 0;
}

// zero_pad of a row of pb points to `points` (data_reorganization.rs:343-358, 429-442): out = zeros; out[d0 .. d0 + n0) = in[0 ..);
// out[d1 .. d1 + n1) = in[s1 ..).  option 0 End, 1 Surround (right = diff / 2), else Center (the first ceil(pb / 2)
// points stay, the last floor(pb / 2) move to the end).
template <typename IDX>
struct MfPad {
    IDX d0, n0, d1, s1, n1;
};

inline void mf_pad_geom(size_t pb, size_t points, int option, size_t* d0, size_t* n0, size_t* d1, size_t* s1, size_t* n1)
{
    *d0 = 0; *n0 = pb; *d1 = 0; *s1 = 0; *n1 = 0;
    if (option == 1) {
        const size_t diff = points - pb, right = diff / 2;
        *d0 = diff - right;
    } else if (option != 0) {
        const size_t right = pb / 2, left = pb - pb / 2;
        *n0 = left;
        *d1 = points - right; *s1 = pb - right; *n1 = right;
    }
}

// position g of the padded row: true and *src = the position in the old row it copies, false: zero
template <typename IDX>
BDSP_MF_HD bool mf_pad_src(IDX g, const MfPad<IDX>& p, IDX* src)
{
    if (g >= p.d0 && g - p.d0 < p.n0) { *src = g - p.d0; return true; }
    if (g >= p.d1 && g - p.d1 < p.n1) { *src = p.s1 + (g - p.d1); return true; }
    return false;
}

// rotate: out[i] = in[(i + shift) mod points], shift < points.  fft_shift: shift = ceil(points / 2); ifft_shift: shift =
// floor(points / 2) -- for odd lengths exactly what the reference's cycle walk produces (KATs vector_types/mod.rs:700-712)
template <typename IDX>
BDSP_MF_HD IDX mf_rotate_src(IDX i, IDX points, IDX shift)
{
    IDX src = i + shift;
    if (src >= points) src -= points;
    return src;
}

// 32-bit indices while every flat extent (and so every flat index plus one grid stride, and 2 * width) stays below 2^32
inline bool mf_fits_32(size_t a, size_t b) { return a < (size_t(1) << 31) && b < (size_t(1) << 31); }

// ---------------------------------------------------------------------------------------------
// the lane loops.  `first` = blockIdx.x * blockDim.x + threadIdx.x, `stride` = gridDim.x * blockDim.x.  In / Out are
// anything with operator[] (device pointers in the kernels), P the element packet (a real scalar or a complex pair;
// P() is zero, a + b adds the components).
// ---------------------------------------------------------------------------------------------
// out[r][j] = x[r * H + j], zero at or past P; total = rows * F
template <typename P, typename IDX, class In, class Out>
BDSP_MF_HD void mf_lane_from_frames(In x, Out out, IDX total, IDX Pn, IDX F, IDX H, IDX first, IDX stride)
{
    IDX o = first;
    if (o >= total) return;
    MfPos<IDX> at = mf_pos<IDX>(o, F);
    const MfPos<IDX> step = mf_pos<IDX>(stride, F);
    for (; o < total; o += stride) {
        const IDX src = mf_frame_src<IDX>(at.row, at.col, H);
        P v = P();
        if (src < Pn) v = x[src];
        out[o] = v;
        mf_advance<IDX>(&at, step, F);
    }
}

// y[i] = sum over r0 .. r1, ascending, of m[r][i - r * H], from +0; total = (rows - 1) * H + F
template <typename P, typename IDX, class In, class Out>
BDSP_MF_HD void mf_lane_overlap_add(In m, Out y, IDX total, IDX rows, IDX F, IDX H, IDX first, IDX stride)
{
    IDX i = first;
    if (i >= total) return;
    MfPos<IDX> at = mf_pos<IDX>(i, H); // i = at.row * H + at.col
    const MfPos<IDX> step = mf_pos<IDX>(stride, H);
    for (; i < total; i += stride) {
        IDX r0, r1;
        mf_ola_rows<IDX>(at.row, at.col, rows, F, H, &r0, &r1);
        P acc = P();
        IDX src = r0 * F + (i - r0 * H); // m[r0][i - r0 * H]; the next row's is F - H further (modulo 2^bits while H > F)
        for (IDX r = r0; r <= r1; ++r) {
            acc = acc + m[src];
            src += F;
            src -= H;
        }
        y[i] = acc;
        mf_advance<IDX>(&at, step, H);
    }
}

// out[r][c] = vectors[r][c]; total = rows * points.  Tab: vectors[r] is anything with operator[]
template <typename P, typename IDX, class Tab, class Out>
BDSP_MF_HD void mf_lane_from_vectors(Tab vectors, Out out, IDX total, IDX points, IDX first, IDX stride)
{
    IDX o = first;
    if (o >= total) return;
    MfPos<IDX> at = mf_pos<IDX>(o, points);
    const MfPos<IDX> step = mf_pos<IDX>(stride, points);
    for (; o < total; o += stride) {
        out[o] = vectors[at.row][at.col];
        mf_advance<IDX>(&at, step, points);
    }
}

// out[r][g] = the zero-padded row r of `in` (rows of pb points); total = rows * points
template <typename P, typename IDX, class In, class Out>
BDSP_MF_HD void mf_lane_zero_pad(In in, Out out, IDX total, IDX pb, IDX points, MfPad<IDX> pad, IDX first, IDX stride)
{
    IDX o = first;
    if (o >= total) return;
    MfPos<IDX> at = mf_pos<IDX>(o, points);
    const MfPos<IDX> step = mf_pos<IDX>(stride, points);
    for (; o < total; o += stride) {
        IDX src;
        P v = P();
        if (mf_pad_src<IDX>(at.col, pad, &src)) v = in[at.row * pb + src];
        out[o] = v;
        mf_advance<IDX>(&at, step, points);
    }
}

// out[r][i] = in[r][(i + shift) mod points]; total = rows * points
template <typename P, typename IDX, class In, class Out>
BDSP_MF_HD void mf_lane_rotate(In in, Out out, IDX total, IDX points, IDX shift, IDX first, IDX stride)
{
    IDX o = first;
    if (o >= total) return;
    MfPos<IDX> at = mf_pos<IDX>(o, points);
    const MfPos<IDX> step = mf_pos<IDX>(stride, points);
    for (; o < total; o += stride) {
        out[o] = in[(o - at.col) + mf_rotate_src<IDX>(at.col, points, shift)];
        mf_advance<IDX>(&at, step, points);
    }
}

} // namespace bdsp
