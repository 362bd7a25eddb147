// detect.hip -- detect: the cells of every row of a real f32 / f64 matrix that stand above a threshold and are strict local
// maxima of a given order, compacted into one list in row-major order (detect_core.h has the predicate, the boundary rules,
// the LDS map and the prefix arithmetic).
//
// Four launches whatever the row count:
//   k_detect_count       rows x tiles of DETECT_TILE cells: the workgroup loads its tile and a halo of `order` cells on each
//                        side into LDS, applying the boundary rule; every lane tests its four cells; a wave's 64-bit ballot
//                        counts a (step, wave) segment of 64 consecutive cells; the tile's count is the sum of the 16
//   k_detect_scan_tiles  the exclusive prefix of the tile counts of every row and the row's total, 64-bit
//   k_detect_scan_rows   the exclusive prefix of the row totals, 64-bit, one workgroup
//   k_detect_write       the tile launch again: a detection's slot is row offset + tile offset + the counts of the segments
//                        before its own + the set bits of the ballot below its lane; index and value are stored where the
//                        slot is below the capacity
// Every slot is written by exactly one thread, once; plain loads and stores only, no workgroup waits for another: the list
// is a function of the data and the arguments.  Rows are read one value per lane and step: they need not start on a
// 16-byte boundary.  No register array, so there is no scratch.
// tests/host_sim/sim_detect.cpp runs the functions of detect_core.h with threads as loops.
#include "bdsp_internal.h"
#include "detect_core.h"

namespace bdsp {

extern __shared__ __align__(16) unsigned char detect_smem[];

template <typename T>
struct DetectIn {
    const T* x;           // rows x n
    size_t n;
    unsigned tiles;
    int order, boundary, kind;
    double t;             // DETECT_SCALAR
    const double* t_rows; // DETECT_PER_ROW: rows values
    const T* t_cells;     // DETECT_PROFILE: n values (t_stride 0); DETECT_PER_CELL: rows x n (t_stride n)
    size_t t_stride;
};

// loads the tile; bit k of the result: the lane's cell of step k is a detection
template <typename T>
__device__ __forceinline__ unsigned detect_tile_flags(const DetectIn<T>& a, size_t row, size_t tile, T* lds)
{
    const int tid = (int)threadIdx.x;
    const int points = detect_tile_points(a.n, tile), loaded = detect_loaded(points, a.order);
    const T* src = a.x + row * a.n;
    const int64_t first = detect_first_position(tile, a.order);
    for (int p = tid; p < loaded; p += DETECT_THREADS) {
        const int64_t g = rank_src_index(first + p, (int64_t)a.n, a.boundary);
        lds[p] = g < 0 ? (T)0 : src[g];
    }
    __syncthreads();
    const double t_row = a.kind == DETECT_PER_ROW ? a.t_rows[row] : a.t;
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < DETECT_PER_LANE; ++k) {
        const int o = detect_cell(tid, k);
        if (o < points) {
            const size_t j = tile * (size_t)DETECT_TILE + (size_t)o;
            const int slot = detect_slot(o, a.order);
            const T t_cell = a.kind >= DETECT_PROFILE ? a.t_cells[row * a.t_stride + j] : (T)0;
            if (detect_above<T>(lds[slot], a.kind, t_row, t_cell) &&
                detect_is_peak<T>(lds, slot, detect_reach(j, a.n, a.order, a.boundary, 0), detect_reach(j, a.n, a.order, a.boundary, 1)))
                mine |= 1u << k;
        }
    }
    return mine;
}

// the count of every (step, wave) segment into seg[]; all 256 lanes take part in every ballot
__device__ __forceinline__ void detect_segment_counts(unsigned mine, unsigned* seg)
{
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int k = 0; k < DETECT_PER_LANE; ++k) {
        const unsigned long long ballot = __ballot((mine >> k) & 1u);
        if (tid % DETECT_WAVE == 0) seg[detect_segment(tid, k)] = (unsigned)__popcll(ballot);
    }
    __syncthreads();
}

// blockIdx.x = row * tiles + tile
template <typename T>
__global__ __launch_bounds__(DETECT_THREADS) void k_detect_count(DetectIn<T> a, int64_t* __restrict__ tile_count)
{
    unsigned* seg = reinterpret_cast<unsigned*>(detect_smem);
    T* lds = reinterpret_cast<T*>(detect_smem + detect_data_offset());
    const size_t row = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const unsigned mine = detect_tile_flags<T>(a, row, tile, lds);
    detect_segment_counts(mine, seg);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = (int64_t)detect_tile_total(seg);
}

// blockIdx.x = row * tiles + tile; tile_off, row_off: the exclusive prefixes of the two scan launches
template <typename T>
__global__ __launch_bounds__(DETECT_THREADS) void k_detect_write(DetectIn<T> a, const int64_t* __restrict__ tile_off,
                                                                  const int64_t* __restrict__ row_off, uint64_t capacity,
                                                                  int64_t* __restrict__ index, T* __restrict__ value)
{
    unsigned* seg = reinterpret_cast<unsigned*>(detect_smem);
    T* lds = reinterpret_cast<T*>(detect_smem + detect_data_offset());
    const size_t row = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const uint64_t base = (uint64_t)(row_off[row] + tile_off[blockIdx.x]);
    if (base >= capacity) return; // the whole workgroup: nothing of this tile is listed
    const int tid = (int)threadIdx.x;
    const unsigned mine = detect_tile_flags<T>(a, row, tile, lds);
    detect_segment_counts(mine, seg);
#pragma unroll
    for (int k = 0; k < DETECT_PER_LANE; ++k) {
        const bool hit = (mine >> k) & 1u;
        const unsigned long long ballot = __ballot(hit);
        // the set bits below this lane's: detect_lane_rank(ballot, lane)
        const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
        const uint64_t pos = base + detect_segment_base(seg, detect_segment(tid, k)) + below;
        if (hit && pos < capacity) {
            const int o = detect_cell(tid, k);
            index[pos] = (int64_t)(tile * (size_t)DETECT_TILE + (size_t)o);
            value[pos] = lds[detect_slot(o, a.order)];
        }
    }
}

// one chunk of `entries` 64-bit values at e, from chunk_start on: every entry becomes carry + the sum of the entries before
// it; returns the chunk's sum.  All threads call; the buffers are free again on return.
__device__ __forceinline__ int64_t detect_scan_chunk(int64_t* e, size_t chunk_start, size_t entries, int64_t carry, int64_t* buf0, int64_t* buf1)
{
    const int tid = (int)threadIdx.x;
    const size_t first = detect_scan_first(chunk_start, tid);
    int64_t *src = buf0, *dst = buf1;
    const int64_t own = detect_scan_own(e, first, entries);
    src[tid] = own;
    __syncthreads();
    for (int step = 0; step < DETECT_SCAN_STEPS; ++step) {
        detect_scan_step(src, dst, tid, step);
        __syncthreads();
        int64_t* t = src; src = dst; dst = t;
    }
    const int64_t inclusive = src[tid], total = src[DETECT_THREADS - 1];
    __syncthreads();
    detect_scan_write(e, first, entries, carry + inclusive - own);
    return total;
}

// tile: rows x tiles counts in, the exclusive prefix within the row out; row_count[row] and row_off[row]: the row's total
// (one for the caller, one for k_detect_scan_rows to scan in place).  Workgroup b takes the rows b, b + gridDim.x, ...
__global__ __launch_bounds__(DETECT_THREADS) void k_detect_scan_tiles(int64_t* __restrict__ tile, int64_t* __restrict__ row_count,
                                                                       int64_t* __restrict__ row_off, size_t rows, size_t tiles)
{
    __shared__ int64_t buf[2][DETECT_THREADS];
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
        int64_t carry = 0;
        for (size_t c0 = 0; c0 < tiles; c0 += DETECT_SCAN_CHUNK) carry += detect_scan_chunk(tile + row * tiles, c0, tiles, carry, buf[0], buf[1]);
        if (threadIdx.x == 0) row_count[row] = row_off[row] = carry;
    }
}

// row_off: the row totals in, the detections of the rows before each row out; one workgroup
__global__ __launch_bounds__(DETECT_THREADS) void k_detect_scan_rows(int64_t* __restrict__ row_off, size_t rows)
{
    __shared__ int64_t buf[2][DETECT_THREADS];
    int64_t carry = 0;
    for (size_t c0 = 0; c0 < rows; c0 += DETECT_SCAN_CHUNK) carry += detect_scan_chunk(row_off, c0, rows, carry, buf[0], buf[1]);
}

// x: rows x n values, rows, n > 0, order <= DETECT_MAX_ORDER, detect_args_valid(kind, boundary); the threshold of the kind:
// t (DETECT_SCALAR), t_rows (DETECT_PER_ROW: rows values on the device), t_cells with t_stride 0 (DETECT_PROFILE: n values)
// or n (DETECT_PER_CELL).  tile_ws: rows x tiles, row_count and row_off: rows values (device); row_count receives the
// detections of every row.  capacity > 0: index and value (device, capacity entries) receive the first detections.
template <typename T>
int detect_rows(const T* x, size_t rows, size_t n, int kind, double t, const double* t_rows, const T* t_cells, size_t t_stride,
                size_t order, int boundary, size_t capacity, int64_t* tile_ws, int64_t* row_count, int64_t* row_off,
                int64_t* index, T* value, hipStream_t s)
{
    const size_t tiles = detect_tiles(n), lds = detect_lds_bytes((int)order, sizeof(T));
    if (rows > 0x7fffffffu / tiles) { set_last_error("detect: rows x tiles above 2^31"); return BDSP_ERR_UNSUPPORTED; }
    const DetectIn<T> a{x, n, (unsigned)tiles, (int)order, boundary, kind, t, t_rows, t_cells, t_stride};
    const dim3 grid((unsigned)(rows * tiles)), block(DETECT_THREADS);
    auto count = k_detect_count<T>;
    BDSP_TRY(kernel_lds(count, lds));
    hipLaunchKernelGGL(count, grid, block, lds, s, a, tile_ws);
    BDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_detect_scan_tiles, dim3(detect_scan_blocks(rows)), block, 0, s, tile_ws, row_count, row_off, rows, tiles);
    BDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_detect_scan_rows, dim3(1), block, 0, s, row_off, rows);
    BDSP_LAUNCH_CHECK();
    if (capacity == 0) return BDSP_OK;
    auto write = k_detect_write<T>;
    BDSP_TRY(kernel_lds(write, lds));
    hipLaunchKernelGGL(write, grid, block, lds, s, a, tile_ws, row_off, (uint64_t)capacity, index, value);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template int detect_rows<float>(const float*, size_t, size_t, int, double, const double*, const float*, size_t, size_t, int, size_t,
                                int64_t*, int64_t*, int64_t*, int64_t*, float*, hipStream_t);
template int detect_rows<double>(const double*, size_t, size_t, int, double, const double*, const double*, size_t, size_t, int, size_t,
                                 int64_t*, int64_t*, int64_t*, int64_t*, double*, hipStream_t);

} // namespace bdsp
