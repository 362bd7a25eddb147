// mat_transpose_core.h -- tile geometry, lane maps and lane loops of mat_transpose.hip, host + device: the side of a
// tile and its LDS pitch, where flat tile t starts, which element of a tile a thread loads and which it stores in step
// k, the load loop (global -> LDS along a source row), the store loop (LDS -> global along a destination row) and the
// flat element-wise map of the thin path.  The kernels call the loops with raw pointers; tests/host_sim/
// sim_mat_transpose.cpp calls the SAME functions with bounds-checking, write-counting arrays and threads as loops, and
// derives the LDS bank conflicts of both sides of the tile from the same slot map.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define BDSP_TP_HD __host__ __device__ __forceinline__
#define BDSP_TP_UNROLL _Pragma("unroll")
#else
#define BDSP_TP_HD inline
#define BDSP_TP_UNROLL
#endif

namespace bdsp {

// ---------------------------------------------------------------------------------------------
// geometry.  An ELEMENT is one packet of 4, 8 or 16 bytes (f32; c32 or f64; c64).  A workgroup of 256 threads moves
// one square tile of S x S elements: S = 64 for 4- and 8-byte elements (256- and 512-byte runs along a row on both
// sides), S = 32 for 16-byte elements (512-byte runs).  LDS: S rows of S + 1 elements.
// ---------------------------------------------------------------------------------------------
constexpr int TP_THREADS = 256;
constexpr int TP_LANES = 64;
// a matrix whose shorter side is below this goes down the flat element-wise path (tp_lane_flat): a square tile would
// leave more than three quarters of its lanes idle on one side
constexpr int TP_THIN = 16;

constexpr int tp_tile_side(size_t elem_bytes) { return elem_bytes <= 8 ? 64 : 32; }
constexpr int tp_pitch(int S) { return S + 1; }                      // LDS row pitch in ELEMENTS
constexpr int tp_lds_elems(int S) { return S * tp_pitch(S); }
constexpr int tp_steps(int S) { return S * S / TP_THREADS; }         // elements per thread and tile: 16 or 4
BDSP_TP_HD int tp_lds_slot(int r, int c, int S) { return r * tp_pitch(S) + c; } // tile[r][c], r the SOURCE row

// step k of thread tid handles tile element i = k * 256 + tid.  Load side: consecutive lanes take consecutive source
// columns of one tile row (a wave: one row of 64, or two rows of 32); store side: consecutive lanes take consecutive
// source ROWS of one tile column, which are consecutive elements of a destination row.
BDSP_TP_HD void tp_load_rc(int k, int tid, int S, int* r, int* c)
{
    const int i = k * TP_THREADS + tid;
    *r = i / S;
    *c = i % S;
}
BDSP_TP_HD void tp_store_rc(int k, int tid, int S, int* r, int* c)
{
    const int i = k * TP_THREADS + tid;
    *c = i / S;
    *r = i % S;
}

// tiles per source row of tiles / per source column of tiles, and the flat tile t = tr * tiles_c + tc
inline size_t tp_tiles_along(size_t n, int S) { return (n + (size_t)S - 1) / (size_t)S; }

template <typename IDX>
BDSP_TP_HD void tp_tile_origin(IDX t, IDX tiles_c, int S, IDX* r0, IDX* c0)
{
    const IDX tr = t / tiles_c;
    *r0 = tr * (IDX)S;
    *c0 = (t - tr * tiles_c) * (IDX)S;
}

// 32-bit indices while every flat index, plus one grid stride, stays below 2^32
inline bool tp_fits_32(size_t total) { return total < (size_t(1) << 31); }

// the thin path applies (the launcher's choice; both paths are correct for every shape)
inline bool tp_is_thin(size_t R, size_t C) { return (R < C ? R : C) < (size_t)TP_THIN; }

// ---------------------------------------------------------------------------------------------
// the lane loops of the tiled path.  src is [R][C], dst is [C][R]; (r0, c0) is the tile's first source row and column.
// In / Out / Lds are anything with operator[] (device and LDS pointers in the kernels), P the element packet.
// ---------------------------------------------------------------------------------------------
// tile[r][c] = src[r0 + r][c0 + c] where that exists: all the loads first, so they are in flight together
template <typename P, typename IDX, int S, class In, class Lds>
BDSP_TP_HD void tp_lane_load(In src, Lds tile, IDX R, IDX C, IDX r0, IDX c0, int tid)
{
    P v[tp_steps(S)];
    BDSP_TP_UNROLL
    for (int k = 0; k < tp_steps(S); ++k) {
        int r, c;
        tp_load_rc(k, tid, S, &r, &c);
        v[k] = P();
        if (r0 + (IDX)r < R && c0 + (IDX)c < C) v[k] = src[(r0 + (IDX)r) * C + (c0 + (IDX)c)];
    }
    BDSP_TP_UNROLL
    for (int k = 0; k < tp_steps(S); ++k) {
        int r, c;
        tp_load_rc(k, tid, S, &r, &c);
        tile[tp_lds_slot(r, c, S)] = v[k];
    }
}

// dst[c0 + c][r0 + r] = tile[r][c] where that exists
template <typename P, typename IDX, int S, class Lds, class Out>
BDSP_TP_HD void tp_lane_store(Lds tile, Out dst, IDX R, IDX C, IDX r0, IDX c0, int tid)
{
    P v[tp_steps(S)];
    BDSP_TP_UNROLL
    for (int k = 0; k < tp_steps(S); ++k) {
        int r, c;
        tp_store_rc(k, tid, S, &r, &c);
        v[k] = tile[tp_lds_slot(r, c, S)];
    }
    BDSP_TP_UNROLL
    for (int k = 0; k < tp_steps(S); ++k) {
        int r, c;
        tp_store_rc(k, tid, S, &r, &c);
        if (r0 + (IDX)r < R && c0 + (IDX)c < C) dst[(c0 + (IDX)c) * R + (r0 + (IDX)r)] = v[k];
    }
}

// ---------------------------------------------------------------------------------------------
// the thin path: one lane per element along the flat [N][K] side, K the short dimension, in a grid-stride loop; the
// other side, [K][N], is reached at k * N + j.  near_is_src: src is [N][K] (a matrix of few COLUMNS: dst[k * N + j] =
// src[f]), else dst is [N][K] (few ROWS: dst[f] = src[k * N + j]).  A wave touches 64 consecutive elements on the near
// side and K runs of 64 / K consecutive elements on the far side, which the next waves continue.  One division per
// lane, then adds and one compare.  `first` = blockIdx.x * blockDim.x + threadIdx.x, `stride` = gridDim.x * blockDim.x.
// ---------------------------------------------------------------------------------------------
template <typename P, typename IDX, class In, class Out>
BDSP_TP_HD void tp_lane_flat(In src, Out dst, IDX total, IDX N, IDX K, bool near_is_src, IDX first, IDX stride)
{
    IDX f = first;
    if (f >= total) return;
    IDX j = f / K, k = f - j * K;
    const IDX sj = stride / K, sk = stride - sj * K;
    for (; f < total; f += stride) {
        const IDX far = k * N + j;
        if (near_is_src) dst[far] = src[f];
        else dst[f] = src[far];
        j += sj;
        k += sk; // < 2 K
        if (k >= K) { k -= K; ++j; }
    }
}

} // namespace bdsp
