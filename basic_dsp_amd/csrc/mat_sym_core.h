// mat_sym_core.h -- index maps of the symmetric real-signal transforms of a matrix (mat_sym.hip, k_sy_crop_rows and
// k_sy_mirror_rows), host + device: where a lane's flat output index lies in its row, how that position moves by one
// grid stride, which source bin an output position reads, and the "first bin must be real" rule of plain_sifft.
// tests/host_sim/sim_mat_sym.cpp drives exactly these functions with threads as loops.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define BDSP_SY_HD __host__ __device__ __forceinline__
#else
#define BDSP_SY_HD inline
#endif

namespace bdsp {

// A lane's place in the flat output: row `row`, position `col` of `width`.  Set once from the flat index (the one
// division a lane does), then moved by the grid stride with adds and one compare per element.
template <typename IDX>
struct SyPos {
    IDX row, col;
};

template <typename IDX>
BDSP_SY_HD SyPos<IDX> sy_pos(IDX flat, IDX width)
{
    const IDX row = flat / width;
    return SyPos<IDX>{row, flat - row * width};
}

// the stride as whole rows + leftover columns (leftover < width), computed once per lane
template <typename IDX>
BDSP_SY_HD SyPos<IDX> sy_stride(IDX stride, IDX width) { return sy_pos<IDX>(stride, width); }

template <typename IDX>
BDSP_SY_HD void sy_advance(SyPos<IDX>* at, SyPos<IDX> step, IDX width)
{
    at->row += step.row;
    at->col += step.col; // < 2 * width: no wrap in IDX while 2 * width fits (the launchers see to it)
    if (at->col >= width) { at->col -= width; ++at->row; }
}

// crop (unmirror!, time_to_freq.rs:178-186): bin j < p of row `row` of the full spectrum of n = 2p - 1 bins
template <typename IDX>
BDSP_SY_HD IDX sy_crop_src(IDX row, IDX j, IDX n) { return row * n + j; }

// mirror (freq.rs:52-83) of the half spectrum h(j) = in[(j + rot) mod p], rot < p: output position g < 2p - 1 reads bin
// sy_mirror_bin of its row, conjugated if *conj.  rot = 0: the plain mirror; rot = p / 2: ifft_shift of the half
// spectrum first (out[i] = in[(i + p/2) mod p], mat_frame_core.h mf_rotate_src).
template <typename IDX>
BDSP_SY_HD IDX sy_mirror_bin(IDX g, IDX p, IDX rot, bool* conj)
{
    *conj = g >= p;
    IDX j = *conj ? 2 * p - 1 - g : g; // g = p-1+k  ->  h(p-k)
    j += rot;
    if (j >= p) j -= p;
    return j;
}

// The first bin of a half spectrum must be real (freq_to_time.rs:203-211 tests |im| > 1e-10).  A spectrum that was
// COMPUTED carries rounding noise of a few eps * |X| there, so the absolute test is paired with a relative one against
// the first bins -- op_sifft's rule, in double as there.  re1 = im1 = 0 for a spectrum of one bin.
BDSP_SY_HD bool sy_first_bin_fails(double re0, double im0, double re1, double im1)
{
    const double a = im0 < 0 ? -im0 : im0;
    const double scale = (re0 < 0 ? -re0 : re0) + (re1 < 0 ? -re1 : re1) + (im1 < 0 ? -im1 : im1);
    return a > 1e-10 && a > 1e-3 * scale;
}

} // namespace bdsp
