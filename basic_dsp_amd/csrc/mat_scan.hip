// mat_scan.hip -- cum_sum (diff_sum.rs:110-122) and unwrap (real_ops.rs:262-284) of a vector or of every row of a matrix
// (a vector is a matrix of one row), and diff / diff_with_start of every row of a matrix (matrix/src/general/
// elementary.rs:206-225 DiffSumOps, matrix/src/real.rs:69-83 ModuloOps).  The launch counts do not depend on the number
// of rows.
//   * k_ms_diff: one launch over the flat output; every row as vecmath.hip's k_diff on it (the vector keeps that kernel:
//     at 2^20 points it measured faster than this one with one row).
//   * k_ms_scan_*: per-row prefix sums, the running sum carried in double whatever T is and rounded once per element
//     (the reference adds sequentially in T; compared with tolerance).  Rows of at most SCAN_CHUNK points in ONE pass
//     without scratch (a lane group per row, or a workgroup per row), longer rows in three steps with the row as a grid
//     dimension: chunk sums -> scan of the chunk sums -> rescan of every chunk with its offset.
//   * k_ms_unwrap: y[j] = F(x[j], y[j-1]) with a data-dependent branch on the ALREADY UNWRAPPED neighbour is a
//     genuinely sequential recurrence (its state does not reduce to an associative operator), the rows are
//     independent: one lane per row, the tiles travel global <-> LDS with coalesced runs (mat_scan_core.h).  Exact, not
//     fast for one long row (see DESIGN.md for the rate).
#include "bdsp_internal.h"
#include "mat_scan_core.h"

namespace bdsp {

// ---- diff -------------------------------------------------------------------------------------------------------
// Output element idx = r * n_out + j of the flat result; per row exactly k_diff:
// out[j] = in[j + step] - in[j] (diff, n_out = row_len - step) or j < step ? in[j] : in[j] - in[j - step] (n_out = row_len).
// A thread takes MS_DIFF_PER outputs 256 apart: one division, then (r, j) advance by (256 / n_out, 256 % n_out).
constexpr int MS_DIFF_PER = 8;
template <typename T>
__global__ __launch_bounds__(256) void k_ms_diff(const T* __restrict__ in, T* __restrict__ out, size_t total, size_t n_out,
                                                 size_t row_len, size_t step, bool with_start)
{
    size_t idx = (size_t)blockIdx.x * (256 * MS_DIFF_PER) + threadIdx.x;
    if (idx >= total) return;
    size_t r = idx / n_out, j = idx - r * n_out;
    const size_t dq = 256 / n_out, dr = 256 % n_out;
    for (int k = 0; k < MS_DIFF_PER && idx < total; ++k, idx += 256) {
        const T* row = in + r * row_len;
        if (with_start) out[idx] = j < step ? row[j] : row[j] - row[j - step];
        else out[idx] = row[j + step] - row[j];
        r += dq;
        j += dr;
        if (j >= n_out) { j -= n_out; ++r; }
    }
}

template <typename T>
int ms_diff(const T* in, T* out, size_t rows, size_t row_len, size_t step, bool with_start, hipStream_t s)
{
    if (row_len < step) return BDSP_OK;
    const size_t n_out = with_start ? row_len : row_len - step, total = rows * n_out;
    if (total == 0) return BDSP_OK;
    const size_t per = 256 * MS_DIFF_PER;
    hipLaunchKernelGGL(k_ms_diff<T>, dim3((unsigned)((total + per - 1) / per)), dim3(256), 0, s, in, out, total, n_out,
                       row_len, step, with_start);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// ---- cum_sum ----------------------------------------------------------------------------------------------------
// Short rows (at most MS_SCAN_SHORT points): a group of G lanes per row, 256 / G rows per workgroup.  The row goes
// through the group in strips of G points: coalesced load, inclusive scan across the group by shuffles in double, plus
// the carry of the strips before; the carry is the last lane's result.  No LDS, no scratch buffer.
constexpr int MS_SCAN_SHORT = 512;
template <typename T, int E, int G>
__global__ __launch_bounds__(256) void k_ms_scan_short(T* __restrict__ x, size_t rows, size_t points)
{
    const size_t row = (size_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int gl = threadIdx.x % G;
    const bool active = row < rows; // a whole group at a time: G divides the wavefront
    T* xr = x + (active ? row : 0) * points * E;
    double carry[E];
#pragma unroll
    for (int c = 0; c < E; ++c) carry[c] = 0.0;
    for (size_t s0 = 0; s0 < points; s0 += G) {
        const size_t i = s0 + gl;
        const bool ok = active && i < points;
        double v[E];
#pragma unroll
        for (int c = 0; c < E; ++c) v[c] = ok ? (double)xr[i * E + c] : 0.0;
#pragma unroll
        for (int d = 1; d < G; d <<= 1) {
#pragma unroll
            for (int c = 0; c < E; ++c) {
                const double t = __shfl_up(v[c], d, G);
                if (gl >= d) v[c] += t;
            }
        }
#pragma unroll
        for (int c = 0; c < E; ++c) v[c] += carry[c];
        if (ok) {
#pragma unroll
            for (int c = 0; c < E; ++c) xr[i * E + c] = (T)v[c];
        }
#pragma unroll
        for (int c = 0; c < E; ++c) carry[c] = __shfl(v[c], G - 1, G);
    }
}

// One chunk of SCAN_CHUNK points of a row by one workgroup: a thread scans 16 CONSECUTIVE points, the chunk travels
// global <-> LDS with unit stride (point e at LDS slot e + e / 16, so that the per-thread runs start in different
// banks; reading the runs straight from global memory -- every lane its own cache line -- measured 511 us for 16M
// complex f32 points).  `offset`: the E sums of the row's points before the chunk, or null.
template <typename T, int E>
__device__ __forceinline__ void ms_scan_chunk(T* __restrict__ xrow, size_t n, size_t base, const double* __restrict__ offset)
{
    struct El { T c[E]; };
    __shared__ El tile[SCAN_CHUNK + SCAN_CHUNK / 16];
    __shared__ double sh[E][256];
    El* xe = reinterpret_cast<El*>(xrow);
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        const int e = k * 256 + threadIdx.x;
        El v;
        for (int c = 0; c < E; ++c) v.c[c] = T(0);
        if (base + e < n) v = xe[base + e];
        tile[e + (e >> 4)] = v;
    }
    __syncthreads();
    double v[SCAN_PER_THREAD][E];
    double acc[E] = {};
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        const El el = tile[threadIdx.x * 17 + k];
        for (int c = 0; c < E; ++c) { v[k][c] = (double)el.c[c]; acc[c] += v[k][c]; }
    }
    for (int c = 0; c < E; ++c) sh[c][threadIdx.x] = acc[c];
    __syncthreads();
    // Hillis-Steele inclusive scan of the 256 thread totals
    for (int d = 1; d < 256; d <<= 1) {
        double t[E];
        for (int c = 0; c < E; ++c) t[c] = (int)threadIdx.x >= d ? sh[c][threadIdx.x - d] : 0.0;
        __syncthreads();
        for (int c = 0; c < E; ++c) sh[c][threadIdx.x] += t[c];
        __syncthreads();
    }
    double run[E];
    for (int c = 0; c < E; ++c) run[c] = (offset ? offset[c] : 0.0) + (threadIdx.x ? sh[c][threadIdx.x - 1] : 0.0);
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        El el;
        for (int c = 0; c < E; ++c) { run[c] += v[k][c]; el.c[c] = (T)run[c]; }
        tile[threadIdx.x * 17 + k] = el;
    }
    __syncthreads();
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        const int e = k * 256 + threadIdx.x;
        if (base + e < n) xe[base + e] = tile[e + (e >> 4)];
    }
}

// mid rows (MS_SCAN_SHORT < points <= SCAN_CHUNK): one workgroup per row, one pass
template <typename T, int E>
__global__ __launch_bounds__(256) void k_ms_scan_row(T* __restrict__ x, size_t points)
{
    ms_scan_chunk<T, E>(x + (size_t)blockIdx.x * points * E, points, 0, nullptr);
}

// long rows, step 1: the sum of every chunk of every row; workgroup b = row * nchunks + chunk, sums[b][E]
template <typename T, int E>
__global__ __launch_bounds__(256) void k_ms_scan_sums(const T* __restrict__ x, size_t points, size_t nchunks,
                                                      double* __restrict__ sums)
{
    __shared__ double sh[E][256];
    const size_t row = blockIdx.x / nchunks, chunk = blockIdx.x - row * nchunks;
    const T* xr = x + row * points * E;
    const size_t base = chunk * SCAN_CHUNK;
    double acc[E] = {};
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        const size_t i = base + (size_t)k * 256 + threadIdx.x;
        if (i < points)
            for (int c = 0; c < E; ++c) acc[c] += (double)xr[i * E + c];
    }
    for (int c = 0; c < E; ++c) sh[c][threadIdx.x] = acc[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < E; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int c = 0; c < E; ++c) sums[(size_t)blockIdx.x * E + c] = sh[c][0];
}

// step 2: exclusive scan of ONE row's chunk sums per workgroup (a thread owns a contiguous run): the offsets of row r
// are built from row r's sums alone
template <int E>
__global__ __launch_bounds__(256) void k_ms_scan_offsets(double* __restrict__ all_sums, size_t nchunks)
{
    __shared__ double sh[E][256];
    double* sums = all_sums + (size_t)blockIdx.x * nchunks * E;
    const size_t per = (nchunks + 255) / 256, b0 = threadIdx.x * per;
    const size_t b = b0 < nchunks ? b0 : nchunks, e = b + per < nchunks ? b + per : nchunks;
    double acc[E] = {};
    for (size_t i = b; i < e; ++i)
        for (int c = 0; c < E; ++c) acc[c] += sums[i * E + c];
    for (int c = 0; c < E; ++c) sh[c][threadIdx.x] = acc[c];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int c = 0; c < E; ++c) {
            double run = 0.0;
            for (int t = 0; t < 256; ++t) { const double v = sh[c][t]; sh[c][t] = run; run += v; }
        }
    __syncthreads();
    double run[E];
    for (int c = 0; c < E; ++c) run[c] = sh[c][threadIdx.x];
    for (size_t i = b; i < e; ++i)
        for (int c = 0; c < E; ++c) { const double v = sums[i * E + c]; sums[i * E + c] = run[c]; run[c] += v; }
}

// step 3: every chunk rescanned with its offset
template <typename T, int E>
__global__ __launch_bounds__(256) void k_ms_scan_apply(T* __restrict__ x, size_t points, size_t nchunks,
                                                       const double* __restrict__ offsets)
{
    const size_t row = blockIdx.x / nchunks, chunk = blockIdx.x - row * nchunks;
    ms_scan_chunk<T, E>(x + row * points * E, points, chunk * SCAN_CHUNK, offsets + (size_t)blockIdx.x * E);
}

// bytes of scratch ms_cum_sum needs: E doubles per chunk of every row, nothing for rows of one chunk
template <typename T> size_t ms_cum_sum_scratch(size_t rows, size_t row_points, bool is_complex)
{
    if (row_points <= (size_t)SCAN_CHUNK) return 0;
    return sizeof(double) * (is_complex ? 2 : 1) * rows * ((row_points + SCAN_CHUNK - 1) / SCAN_CHUNK);
}

template <typename T, int E>
static int ms_cum_sum_e(T* x, size_t rows, size_t points, void* scratch, hipStream_t s)
{
    if (points <= (size_t)MS_SCAN_SHORT) {
        if (points <= 8)
            hipLaunchKernelGGL((k_ms_scan_short<T, E, 4>), dim3((unsigned)((rows + 63) / 64)), dim3(256), 0, s, x, rows, points);
        else if (points <= 64)
            hipLaunchKernelGGL((k_ms_scan_short<T, E, 16>), dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, s, x, rows, points);
        else
            hipLaunchKernelGGL((k_ms_scan_short<T, E, 64>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, points);
    } else if (points <= (size_t)SCAN_CHUNK) {
        hipLaunchKernelGGL((k_ms_scan_row<T, E>), dim3((unsigned)rows), dim3(256), 0, s, x, points);
    } else {
        const size_t nchunks = (points + SCAN_CHUNK - 1) / SCAN_CHUNK;
        if (rows * nchunks > 0x7fffffffull) {
            set_last_error("mat_cum_sum: more than 2^31 chunks");
            return BDSP_ERR_UNSUPPORTED;
        }
        double* sums = static_cast<double*>(scratch);
        const unsigned grid = (unsigned)(rows * nchunks);
        hipLaunchKernelGGL((k_ms_scan_sums<T, E>), dim3(grid), dim3(256), 0, s, x, points, nchunks, sums);
        hipLaunchKernelGGL((k_ms_scan_offsets<E>), dim3((unsigned)rows), dim3(256), 0, s, sums, nchunks);
        hipLaunchKernelGGL((k_ms_scan_apply<T, E>), dim3(grid), dim3(256), 0, s, x, points, nchunks, sums);
    }
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T> int ms_cum_sum(T* x, size_t rows, size_t row_points, bool is_complex, void* scratch, hipStream_t s)
{
    if (rows == 0 || row_points == 0) return BDSP_OK;
    return is_complex ? ms_cum_sum_e<T, 2>(x, rows, row_points, scratch, s) : ms_cum_sum_e<T, 1>(x, rows, row_points, scratch, s);
}

// ---- unwrap -----------------------------------------------------------------------------------------------------
// One wavefront per workgroup, R rows per workgroup, tiles of R x W elements (mat_scan_core.h).  Per tile: all 64 lanes
// fetch tile t + 1 from global memory into registers, lanes 0 .. R-1 walk their row of tile t in LDS (eight elements
// at a time: read, recur, write back in place), all lanes store tile t and move tile t + 1 from the registers into
// the same LDS image.  The fetch is in flight during the walk, which is what the workgroup spends its time on: a
// serial chain of subtract, compare, (remainder,) add per element.  Every element is read and written once.
template <typename T, int R> struct MsShape {
    static constexpr int ELEMS = MS_TILE_BYTES / (int)sizeof(T), W = ELEMS / R, PER = ELEMS / MS_LANES;
};

template <typename T, int R>
__device__ __forceinline__ void ms_fetch(const T* __restrict__ x, size_t row0, int rv, size_t row_len, size_t t,
                                         T (&pre)[MsShape<T, R>::PER])
{
    constexpr int W = MsShape<T, R>::W;
    const size_t col0 = t * W;
    const int m = ms_tile_cols(row_len, t, W);
#pragma unroll
    for (int k = 0; k < MsShape<T, R>::PER; ++k) {
        int r, c;
        ms_tile_rc(k, (int)threadIdx.x, W, &r, &c);
        // slots past the matrix's edges read the edge element again (never stored): straight-line loads, no branches
        r = r < rv ? r : rv - 1;
        c = c < m ? c : m - 1;
        pre[k] = x[(row0 + r) * row_len + col0 + c];
    }
}

template <typename T, int R>
__device__ __forceinline__ void ms_to_lds(T* tile, const T (&pre)[MsShape<T, R>::PER])
{
    constexpr int W = MsShape<T, R>::W;
#pragma unroll
    for (int k = 0; k < MsShape<T, R>::PER; ++k) {
        int r, c;
        ms_tile_rc(k, (int)threadIdx.x, W, &r, &c);
        tile[ms_lds_slot(r, c, W)] = pre[k];
    }
}

template <typename T, int R>
__device__ __forceinline__ void ms_to_global(T* __restrict__ x, const T* tile, size_t row0, int rv, size_t row_len, size_t t)
{
    constexpr int W = MsShape<T, R>::W;
    const size_t col0 = t * W;
    const int m = ms_tile_cols(row_len, t, W);
    // sixteen LDS reads in flight, then their (predicated) stores
#pragma unroll
    for (int kb = 0; kb < MsShape<T, R>::PER; kb += 16) {
        T v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            int r, c;
            ms_tile_rc(kb + k, (int)threadIdx.x, W, &r, &c);
            v[k] = tile[ms_lds_slot(r, c, W)];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            int r, c;
            ms_tile_rc(kb + k, (int)threadIdx.x, W, &r, &c);
            if (r < rv && c < m) x[(row0 + r) * row_len + col0 + c] = v[k];
        }
    }
}

template <typename T, int R>
__global__ __launch_bounds__(MS_LANES) void k_ms_unwrap(T* __restrict__ x, size_t rows, size_t row_len, T divisor)
{
    using S = MsShape<T, R>;
    __shared__ T tile[R * (S::W + 1)]; // ms_lds_elems(R, W)
    const int lane = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * R;
    if (row0 >= rows || row_len == 0) return;
    const int rv = rows - row0 < (size_t)R ? (int)(rows - row0) : R;
    const size_t ntiles = (row_len + S::W - 1) / S::W;
    const T half = divisor / T(2);
    const T inv = T(1) / fabs(divisor);
    T pre[S::PER];
    ms_fetch<T, R>(x, row0, rv, row_len, 0, pre);
    ms_to_lds<T, R>(tile, pre);
    __syncthreads();
    T prev = T(0);
    T* row = tile + ms_lds_slot(lane < R ? lane : 0, 0, S::W);
    for (size_t t = 0; t < ntiles; ++t) {
        const bool more = t + 1 < ntiles;
        if (more) ms_fetch<T, R>(x, row0, rv, row_len, t + 1, pre);
        const int m = ms_tile_cols(row_len, t, S::W);
        if (lane < rv) {
            int j = 0;
            if (t == 0) { prev = row[0]; j = 1; } // the first element of a row stays
            for (; j + 8 <= m; j += 8) {
                T v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = row[j + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) { v[u] = ms_unwrap_step(v[u], prev, half, divisor, inv); prev = v[u]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) row[j + u] = v[u];
            }
            for (; j < m; ++j) {
                prev = ms_unwrap_step(row[j], prev, half, divisor, inv);
                row[j] = prev;
            }
        }
        __syncthreads();
        ms_to_global<T, R>(x, tile, row0, rv, row_len, t);
        __syncthreads();
        if (more) ms_to_lds<T, R>(tile, pre);
        __syncthreads();
    }
}

template <typename T> int ms_unwrap(T* x, size_t rows, size_t row_len, T divisor, hipStream_t s)
{
    if (rows == 0 || row_len < 2) return BDSP_OK;
    const int R = ms_rows_per_group(rows, num_cus());
    const size_t groups = (rows + R - 1) / R;
    if (groups > 0x7fffffffull) {
        set_last_error("mat_unwrap: more than 2^37 rows");
        return BDSP_ERR_UNSUPPORTED;
    }
    const dim3 grid((unsigned)groups), block(MS_LANES);
    switch (R) {
    case 1: hipLaunchKernelGGL((k_ms_unwrap<T, 1>), grid, block, 0, s, x, rows, row_len, divisor); break;
    case 4: hipLaunchKernelGGL((k_ms_unwrap<T, 4>), grid, block, 0, s, x, rows, row_len, divisor); break;
    case 16: hipLaunchKernelGGL((k_ms_unwrap<T, 16>), grid, block, 0, s, x, rows, row_len, divisor); break;
    default: hipLaunchKernelGGL((k_ms_unwrap<T, 64>), grid, block, 0, s, x, rows, row_len, divisor); break;
    }
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

#define BDSP_INST(T)                                                                                   \
    template int ms_diff<T>(const T*, T*, size_t, size_t, size_t, bool, hipStream_t);                  \
    template size_t ms_cum_sum_scratch<T>(size_t, size_t, bool);                                       \
    template int ms_cum_sum<T>(T*, size_t, size_t, bool, void*, hipStream_t);                          \
    template int ms_unwrap<T>(T*, size_t, size_t, T, hipStream_t);
BDSP_INST(float)
BDSP_INST(double)
#undef BDSP_INST

} // namespace bdsp
