// mat_scan_core.h -- the scan chunk size, the exact remainder of unwrap's serial chain and the index math of the per-row
// unwrap (mat_scan.hip, k_ms_unwrap), host + device: which lane loads which element of a tile, where it lands in LDS,
// which lane walks which row, and the recurrence step.  tests/host_sim/sim_mat_scan.cpp drives exactly these functions
// with threads as loops, where the device qualifiers fall away.
#pragma once

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define BDSP_MS_HD __host__ __device__ __forceinline__
#define BDSP_SCAN_FN __device__ __forceinline__
#else
#define BDSP_MS_HD inline
#define BDSP_SCAN_FN inline
#endif

namespace bdsp {

constexpr int SCAN_PER_THREAD = 16;
constexpr int SCAN_CHUNK = 256 * SCAN_PER_THREAD; // elements per workgroup

// fmod on the serial critical path: the remainder a - trunc(a/b)*b is exactly representable, so one fma returns it
// exactly when the quotient is right; a quotient off by one (a/b rounded across an integer) shows as a remainder
// outside [0, |b|) and is redone.  Huge quotients, infinities and NaNs go to the library function.
template <typename T>
BDSP_SCAN_FN T fmod_exact(T a, T b, T inv_abs_b)
{
    const T A = fabs(a), Bv = fabs(b);
    T q = trunc(A * inv_abs_b); // a guess within one of trunc(A / Bv): the checks below settle it
    if (!(q < (T)(sizeof(T) == 4 ? 4194304.0 : 2251799813685248.0))) return fmod(a, b);
    T r = fma(-q, Bv, A);
    if (r < T(0)) r = fma(-(q - T(1)), Bv, A);
    else if (r >= Bv) r = fma(-(q + T(1)), Bv, A);
    return copysign(r, a);
}

// One wavefront per workgroup.  A workgroup owns R consecutive rows and moves them through LDS in tiles of
// R rows x W columns, R * W = MS_TILE_BYTES / sizeof(T) elements whatever R is: every one of the 64 lanes loads and
// stores MS_TILE_BYTES / 64 / sizeof(T) elements per tile, lanes 0 .. R-1 walk one row each.
constexpr int MS_LANES = 64;
constexpr int MS_TILE_BYTES = 16384;
// R = 64: W = 64 f32 / 32 f64 = 256-byte runs per row.  Fewer rows x more columns (16, 4, 1) for matrices of few rows.
BDSP_MS_HD int ms_tile_elems(size_t elem_bytes) { return (int)(MS_TILE_BYTES / elem_bytes); }
BDSP_MS_HD int ms_tile_width(size_t elem_bytes, int R) { return ms_tile_elems(elem_bytes) / R; }

// LDS row stride in ELEMENTS: W + 1, an odd number.
//   f32: walker lane l reads / writes dword l * (W + 1) + j.  The bank is (a / 4) % 32 for ds_read_b32 (and ds_read2_b32
//        per dword) and ds_write_b32, counted per 32-lane half: l * odd mod 32 takes 32 distinct values over any 32
//        consecutive lanes -- conflict-free.
//   f64: the element is two dwords, lane l reads dwords l * 2 (W + 1) + 2 j, + 1 with ds_read_b64, bank (a / 4) % 64 per
//        32-lane half: 2 l (W + 1) mod 64 = 2 * (l * odd mod 32), 32 distinct even banks, each lane its pair --
//        conflict-free.  ds_write_b64 is served in groups of 16 contiguous lanes at (a / 4) % 32: 16 lanes x 2 dwords on
//        2 * (l * odd mod 16) -- conflict-free.
BDSP_MS_HD int ms_lds_stride(int W) { return W + 1; }
BDSP_MS_HD int ms_lds_slot(int r, int c, int W) { return r * ms_lds_stride(W) + c; }
BDSP_MS_HD int ms_lds_elems(int R, int W) { return R * ms_lds_stride(W); }

// Element k (0 .. tile elements / 64) of lane `lane` in the global <-> LDS passes: consecutive lanes take consecutive
// columns of one row (W >= 64), or two rows of 32 columns (f64, R = 64): 256 contiguous bytes per row and instruction.
BDSP_MS_HD void ms_tile_rc(int k, int lane, int W, int* r, int* c)
{
    const int i = k * MS_LANES + lane;
    *r = i / W;
    *c = i % W;
}

// rows per workgroup: the fewest of 1, 4, 16, 64 that keeps the grid within 4 workgroups (one wave per SIMD) per CU
BDSP_MS_HD int ms_rows_per_group(size_t rows, int cus)
{
    const int shapes[3] = {1, 4, 16};
    for (int i = 0; i < 3; ++i)
        if ((rows + shapes[i] - 1) / shapes[i] <= (size_t)4 * (size_t)cus) return shapes[i];
    return 64;
}

// columns of tile t that exist (row_len > t * W)
BDSP_MS_HD int ms_tile_cols(size_t row_len, size_t t, int W)
{
    const size_t left = row_len - t * (size_t)W;
    return left < (size_t)W ? (int)left : W;
}

// one step of unwrap (real_ops.rs:262-284): `prev` is the ALREADY unwrapped neighbour
template <typename T>
BDSP_SCAN_FN T ms_unwrap_step(T cur, T prev, T half, T divisor, T inv)
{
    T diff = cur - prev;
    if (diff > half) { diff = fmod_exact(diff, divisor, inv); diff = diff - divisor; cur = prev + diff; }
    else if (diff < -half) { diff = fmod_exact(diff, divisor, inv); diff = diff + divisor; cur = prev + diff; }
    return cur;
}

} // namespace bdsp
