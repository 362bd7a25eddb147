// mat_mul_core.h -- the dispatch rule, tile geometry, index maps and per-lane arithmetic of mat_mul.hip, host + device.
// The kernels call these functions with raw pointers and the matrix instruction; tests/host_sim/sim_mat_mul.cpp calls
// the SAME functions with threads as loops, the matrix instruction modelled as the k-ordered fmaf chain it is
// documented to be, and bounds-checking, write-counting arrays.
//
// C (M x N) = A (M x K) . op(B); every matrix is dense and row-major, an ELEMENT is one real scalar or one interleaved
// (re, im) pair.  Plain form: B is K x N.  Transposed form: B is N x K and enters conjugated, C[i][j] = sum_k A[i][k]
// conj(B[j][k]).
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define BDSP_MM_HD __host__ __device__ __forceinline__
#else
#define BDSP_MM_HD inline
#endif

namespace bdsp {

constexpr int MM_THREADS = 256;
constexpr int MM_LANES = 64;

// ---------------------------------------------------------------------------------------------
// the three paths and the one rule that picks among them: a function of (M, N, K, form) only -- never of the device's
// CU count, of timing, or of the data.  Number kind and precision change the tile depth (mm_tk), not the path.
// ---------------------------------------------------------------------------------------------
enum MmPath { MM_PATH_STREAM = 0, MM_PATH_TILED = 1, MM_PATH_SPLIT = 2 };

// Streaming path (plain form): A sits in LDS, one thread owns one column of B and keeps all M sums in registers, so
// MM_STREAM_MAX_M bounds the accumulator registers (16 complex f64 sums = 64 VGPRs) and MM_STREAM_MAX_M *
// MM_STREAM_MAX_K elements bound the LDS image (16 KB in complex f64).  Both limits: not measured -- they are what the
// register file and a quarter of the LDS of a workgroup allow, not a crossover found on the device.  profiles/mat_mul.txt
// has one shape on either side: (a) 8 x 8 (streaming) and (b) 64 x 64 (tiled).
constexpr size_t MM_STREAM_MAX_M = 16;
constexpr size_t MM_STREAM_MAX_K = 64;
constexpr int MM_STREAM_COLS = MM_THREADS; // columns of B per workgroup and trip: one per thread

// Tiled path: a workgroup computes one MM_TM x MM_TN tile of C in steps of mm_tk(precision) along K.
constexpr int MM_TM = 64;
constexpr int MM_TN = 64;
constexpr int mm_tk(bool is_double) { return is_double ? 16 : 32; } // 64 x TK elements per operand plane and step
constexpr int MM_PITCH = MM_TM + 1;                                 // LDS plane: [k][row or column], pitch 65 elements
constexpr int mm_plane_elems(int tk) { return tk * MM_PITCH; }

// Split path: with at most MM_SPLIT_MAX_TILES tiles of C (a quarter of the 256 CUs of the part would have work) and K
// from MM_SPLIT_MIN_K on, K is cut into chunks and every (chunk, tile) pair is one workgroup.  Chunks are
// MM_SPLIT_MIN_CHUNK long unless that would make more than MM_SPLIT_TARGET_BLOCKS workgroups; then they grow.  All
// four constants: not measured.  profiles/mat_mul.txt has the shapes (d) and (e) on this path and none on the other
// side of either threshold.
constexpr size_t MM_SPLIT_MAX_TILES = 64;
constexpr size_t MM_SPLIT_MIN_K = 256;
constexpr size_t MM_SPLIT_MIN_CHUNK = 512;
constexpr size_t MM_SPLIT_TARGET_BLOCKS = 1024;

inline size_t mm_tiles_along(size_t n, int t) { return (n + (size_t)t - 1) / (size_t)t; }
inline size_t mm_tiles(size_t M, size_t N) { return mm_tiles_along(M, MM_TM) * mm_tiles_along(N, MM_TN); }

// M, N, K all > 0 (the empty shapes never reach a kernel)
inline MmPath mm_dispatch(size_t M, size_t N, size_t K, bool transposed)
{
    if (!transposed && M <= MM_STREAM_MAX_M && K <= MM_STREAM_MAX_K) return MM_PATH_STREAM;
    if (K >= MM_SPLIT_MIN_K && mm_tiles(M, N) <= MM_SPLIT_MAX_TILES) return MM_PATH_SPLIT;
    return MM_PATH_TILED;
}

// accumulator rows of the streaming kernel: the smallest of 4, 8, 16 that holds M
inline int mm_stream_mb(size_t M) { return M <= 4 ? 4 : (M <= 8 ? 8 : 16); }

// chunk length of the split path (a multiple of 32, so of either tile depth) and the number of chunks
inline size_t mm_split_chunk(size_t M, size_t N, size_t K)
{
    size_t max_chunks = MM_SPLIT_TARGET_BLOCKS / mm_tiles(M, N);
    if (max_chunks == 0) max_chunks = 1;
    size_t c = (K + max_chunks - 1) / max_chunks;
    c = (c + 31) / 32 * 32;
    return c < MM_SPLIT_MIN_CHUNK ? MM_SPLIT_MIN_CHUNK : c;
}
inline size_t mm_split_chunks(size_t M, size_t N, size_t K)
{
    const size_t c = mm_split_chunk(M, N, K);
    return (K + c - 1) / c;
}

// ---------------------------------------------------------------------------------------------
// work item w of the tiled kernel -> (chunk, tile row origin, tile column origin); w = chunk * ntiles + tile, tile =
// tile row * tiles_n + tile column.  The tiled path is the split path with one chunk of K.
// ---------------------------------------------------------------------------------------------
BDSP_MM_HD void mm_work_item(size_t w, size_t ntiles, size_t tiles_n, size_t* chunk, size_t* i0, size_t* j0)
{
    *chunk = w / ntiles;
    const size_t t = w % ntiles;
    *i0 = (t / tiles_n) * (size_t)MM_TM;
    *j0 = (t % tiles_n) * (size_t)MM_TN;
}

// ---------------------------------------------------------------------------------------------
// staging, global -> LDS.  A plane is [k][x], x the row of A or the column of C, pitch 65.  Every thread moves
// TK / 4 elements per operand and step.
//   k-contiguous source (A always; B in the transposed form): consecutive lanes take consecutive k of one row, a run of
//     TK elements (128 B in real f32, 256 B in complex f32 and real f64), and write down a column of the plane;
//   x-contiguous source (B in the plain form): consecutive lanes take 64 consecutive columns of one k.
// Bank rules as in mat_transpose.hip (bank = dword address mod 32 inside a group of 32 lanes for 4-byte accesses, of 16
// lanes for 8-byte writes).  f32, k-contiguous: the 32 lanes of a group hold k = 0 .. 31 of one x and write dwords
// 65 k + x -- 65 is odd, 32 distinct banks.  f64, k-contiguous: 16 lanes hold k = 0 .. 15 and write dword pairs from
// 130 k + 2 x -- 130 = 128 + 2, 16 distinct even banks.  x-contiguous writes and all fragment reads of the f32 kernel
// touch consecutive elements of one plane row.  Conflicts: 0 (sim_mat_mul.cpp counts them from these maps).
// ---------------------------------------------------------------------------------------------
BDSP_MM_HD int mm_stage_steps(int tk) { return tk / 4; }
BDSP_MM_HD void mm_stage_kc(int tid, int r, int tk, int* x, int* k)
{
    *k = tid % tk;
    *x = tid / tk + r * (MM_THREADS / tk);
}
BDSP_MM_HD void mm_stage_xc(int tid, int r, int* x, int* k)
{
    *x = tid % MM_TN;
    *k = tid / MM_TN + r * (MM_THREADS / MM_TN);
}
BDSP_MM_HD int mm_lds_slot(int k, int x) { return k * MM_PITCH + x; }

// ---------------------------------------------------------------------------------------------
// f32: v_mfma_f32_32x32x2_f32.  Wave w of the four owns the 32 x 32 quadrant (w >> 1, w & 1) of the tile.  Operands: lane
// l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; result register g of lane l is C[row = (g & 3) +
// 8 (g >> 2) + 4 (l >> 5)][column = l & 31].  One instruction adds k = 0 then k = 1 to the accumulator, each product
// rounded once into it: a k-ordered fmaf chain.
// ---------------------------------------------------------------------------------------------
BDSP_MM_HD int mm_wave_row0(int wave) { return (wave >> 1) * 32; }
BDSP_MM_HD int mm_wave_col0(int wave) { return (wave & 1) * 32; }
BDSP_MM_HD int mm_mfma_ab_x(int lane) { return lane & 31; }
BDSP_MM_HD int mm_mfma_ab_k(int lane) { return lane >> 5; }
BDSP_MM_HD int mm_mfma_c_row(int lane, int g) { return (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5); }
BDSP_MM_HD int mm_mfma_c_col(int lane) { return lane & 31; }

// f64 (vector ALU): thread t owns the 4 x 4 elements (row (t >> 4) + 16 r, column (t & 15) + 16 c), r, c < 4
BDSP_MM_HD int mm_valu_row(int tid, int r) { return (tid >> 4) + 16 * r; }
BDSP_MM_HD int mm_valu_col(int tid, int c) { return (tid & 15) + 16 * c; }

// ---------------------------------------------------------------------------------------------
// One complex step on three real sums.  With b' = B (plain form) or conj(B) (transposed form; the sign of B's imaginary
// part is flipped when B is staged), a . b' = (ar br - ai bi') + i (ar bi' + ai br): four real products, no
// three-multiplication trick.  The two imaginary terms keep sums of their own, im = ia + ib at the very end: then
// C[j][i] of a Gram matrix goes through the same products with ia and ib exchanged and negated, so it is conj(C[i][j])
// to the bit, and the diagonal's imaginary part is x + (-x) = +0.
// fma3 is fmaf / fma on the host, on the f64 path and in the streaming kernel; in the f32 tiled kernel the matrix
// instruction takes its place with the same operands in the same order.  One instruction takes TWO k, so there the real
// sum goes ar br (k), ar br (k + 1), -ai bi (k), -ai bi (k + 1), then on to k + 2, with k counted from the start of the
// chunk; ia and ib stay plain chains over ascending k.  Still a function of the shape alone, and still symmetric under
// the exchange of i and j.
// ---------------------------------------------------------------------------------------------
template <typename S, typename A, typename F> // S: an operand scalar; A: a sum (a scalar, or the 16 registers of a lane)
BDSP_MM_HD void mm_cplx_step(S ar, S ai, S br, S bi, A* re, A* ia, A* ib, F fma3)
{
    *re = fma3(ar, br, *re);
    *re = fma3(-ai, bi, *re);
    *ia = fma3(ar, bi, *ia);
    *ib = fma3(ai, br, *ib);
}

// streaming kernel: LDS slot of A[m][k] (component c of e per element): [k][MB][e], so one thread's reads of consecutive
// m are consecutive; all lanes read the same address (a broadcast, no conflict)
BDSP_MM_HD int mm_stream_slot(int m, int k, int c, int mb, int e) { return (k * mb + m) * e + c; }

} // namespace bdsp
