// detect_core.h -- the plan, the index maps, the predicate, the boundary index, the LDS map and the prefix arithmetic of
// detect.hip, host + device: detect, the cells of every row of a real matrix that stand above a threshold and are strict
// local maxima, as one compact list in row-major order.  The kernels call these functions on their LDS;
// tests/host_sim/sim_detect.cpp calls the SAME functions with threads as loops.
//
// Cell j of a row of n points is a detection iff
//   threshold  DETECT_NONE: always; DETECT_SCALAR / DETECT_PER_ROW: double(x[j]) > t (t of the call / of the row);
//              DETECT_PROFILE / DETECT_PER_CELL: x[j] > t[j] / t[row][j] in the data's precision.  IEEE >: a NaN on either
//              side is no detection, -0 is not above +0, denormals compare by value;
//   peak       for every 0 < |d| <= order: x[j] > x[j + d].  Positions outside the row: DETECT_OPEN skips the comparison
//              (the loops stop at the row's ends: detect_reach), DETECT_WRAP reads index mod n, DETECT_NEAREST the end point;
//              the two are rank_filter's rules and rank_src_index serves them.  order >= n under wrap, and an end point
//              under nearest, compare a cell with itself: x > x is false, nothing is detected.
//
// A row is cut into tiles of DETECT_TILE cells; the grid of the two tile launches is rows x tiles.  LDS map of a tile
// launch: DETECT_SEGMENTS unsigned counts first (detect_data_offset() bytes), then slot p = the value of row position
// tile * DETECT_TILE - order + p, p < points + 2 order, so cell o of the tile is slot order + o and its neighbours are the
// slots around it; DETECT_TILE + 2 order values are allocated (24 KB for f64 at DETECT_MAX_ORDER).  At step k lane t owns
// cell k * 256 + t: the 64 lanes of a wave own 64 CONSECUTIVE cells, the segment (k, wave) = cell / 64, so the wave's 64-bit
// ballot lists its detections in index order, a lane's place inside the segment is the number of set bits below its own
// (detect_lane_rank) and the segment's place inside the tile is the sum of the counts of the segments before it
// (detect_segment_base).  Consecutive lanes read consecutive slots at every step of the peak loops: conflict-free.
//
// Four launches whatever the row count:
//   count       rows x tiles workgroups: the number of detections of every tile
//   scan tiles  at most DETECT_SCAN_CHUNK workgroups, each taking the rows blockIdx.x, + gridDim.x, ...: the exclusive
//               prefix of a row's tile counts, DETECT_SCAN_CHUNK tiles at a time with a 64-bit carry, and the row's total
//   scan rows   one workgroup: the exclusive prefix of the row totals, DETECT_SCAN_CHUNK rows at a time with a 64-bit carry
//   write       rows x tiles workgroups evaluate the predicate again and store index and value of every detection whose
//               slot (row offset + tile offset + segment base + lane rank) is below the capacity
// A chunk is DETECT_SCAN_ITEMS consecutive entries per thread; the 256 thread sums are scanned in LDS by doubling steps
// between two buffers (detect_scan_step).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rank_filter_core.h"

#if defined(__HIPCC__)
#define BDSP_DETECT_HD __host__ __device__ __forceinline__
#else
#define BDSP_DETECT_HD inline
#endif

namespace bdsp {

constexpr int DETECT_THREADS = 256;
constexpr int DETECT_WAVE = 64;
constexpr int DETECT_PER_LANE = 4; // cells per lane; with DETECT_THREADS it makes the tile
// cells per tile
constexpr int DETECT_TILE = 1024; // not measured: no other tile was built
// (step, wave) segments of a tile, 64 consecutive cells each
constexpr int DETECT_SEGMENTS = 16;
// the longest order: the halo is then twice the tile
constexpr int DETECT_MAX_ORDER = 1024; // not measured (24 KB of LDS for f64; the cost per cell grows with the order, not with this)
// entries per step of the two prefix launches: DETECT_SCAN_ITEMS consecutive entries per thread; also the most workgroups
// of the tile-prefix launch
constexpr int DETECT_SCAN_ITEMS = 16; // not measured: one entry per thread took 242 us for the counts of 16384 x 2048, no third value was built
constexpr int DETECT_SCAN_CHUNK = 4096; // not measured: DETECT_THREADS x DETECT_SCAN_ITEMS
constexpr int DETECT_SCAN_STEPS = 8;

static_assert(DETECT_TILE == DETECT_THREADS * DETECT_PER_LANE, "DETECT_PER_LANE cells per lane");
static_assert(DETECT_SEGMENTS * DETECT_WAVE == DETECT_TILE, "a segment is the cells of one wave at one step");
static_assert(DETECT_SCAN_CHUNK == DETECT_THREADS * DETECT_SCAN_ITEMS && (1 << DETECT_SCAN_STEPS) == DETECT_THREADS, "DETECT_SCAN_ITEMS entries per thread");

enum { DETECT_OPEN = 0, DETECT_WRAP = 1, DETECT_NEAREST = 2 };
enum { DETECT_NONE = 0, DETECT_SCALAR = 1, DETECT_PER_ROW = 2, DETECT_PROFILE = 3, DETECT_PER_CELL = 4 };

static_assert((int)DETECT_WRAP == (int)RANK_WRAP && (int)DETECT_NEAREST == (int)RANK_NEAREST && (int)DETECT_OPEN == (int)RANK_ZERO,
              "rank_src_index serves the boundary codes (open: the slots it marks -1 are filled with zero and never read)");

// ---------------------------------------------------------------------------------------------
// the plan: a function of (n, order) alone
// ---------------------------------------------------------------------------------------------
BDSP_DETECT_HD bool detect_args_valid(int kind, int boundary)
{
    return kind >= DETECT_NONE && kind <= DETECT_PER_CELL && boundary >= DETECT_OPEN && boundary <= DETECT_NEAREST;
}
BDSP_DETECT_HD size_t detect_tiles(size_t n) { return (n + DETECT_TILE - 1) / DETECT_TILE; }
BDSP_DETECT_HD int detect_tile_points(size_t n, size_t tile)
{
    const size_t left = n - tile * (size_t)DETECT_TILE;
    return left < (size_t)DETECT_TILE ? (int)left : DETECT_TILE;
}
// workgroups of the tile-prefix launch; workgroup b takes the rows b, b + blocks, ...
BDSP_DETECT_HD unsigned detect_scan_blocks(size_t rows) { return rows < (size_t)DETECT_SCAN_CHUNK ? (unsigned)rows : (unsigned)DETECT_SCAN_CHUNK; }

// ---------------------------------------------------------------------------------------------
// LDS map of the tile launches
// ---------------------------------------------------------------------------------------------
BDSP_DETECT_HD size_t detect_data_offset() { return sizeof(unsigned) * DETECT_SEGMENTS; } // bytes; a multiple of 16
BDSP_DETECT_HD int detect_lds_values(int order) { return DETECT_TILE + 2 * order; }       // allocated
BDSP_DETECT_HD size_t detect_lds_bytes(int order, size_t value_bytes) { return detect_data_offset() + value_bytes * (size_t)detect_lds_values(order); }
BDSP_DETECT_HD int detect_loaded(int points, int order) { return points + 2 * order; }    // filled
BDSP_DETECT_HD int64_t detect_first_position(size_t tile, int order) { return (int64_t)(tile * (size_t)DETECT_TILE) - (int64_t)order; }
BDSP_DETECT_HD int detect_cell(int tid, int k) { return k * DETECT_THREADS + tid; }       // the tile's cell of lane tid at step k
BDSP_DETECT_HD int detect_segment(int tid, int k) { return k * (DETECT_THREADS / DETECT_WAVE) + tid / DETECT_WAVE; }
BDSP_DETECT_HD int detect_slot(int o, int order) { return order + o; }

// how far the peak test of row index j looks to the left (side 0) and to the right (side 1)
BDSP_DETECT_HD int detect_reach(size_t j, size_t n, int order, int boundary, int side)
{
    if (boundary != DETECT_OPEN) return order;
    const size_t room = side ? n - 1 - j : j;
    return room < (size_t)order ? (int)room : order;
}

// ---------------------------------------------------------------------------------------------
// the predicate
// ---------------------------------------------------------------------------------------------
// t_row: the threshold of kinds 1 and 2; t_cell: that of kinds 3 and 4
template <typename T>
BDSP_DETECT_HD bool detect_above(T x, int kind, double t_row, T t_cell)
{
    if (kind == DETECT_NONE) return true;
    if (kind <= DETECT_PER_ROW) return (double)x > t_row;
    return x > t_cell;
}

// lds[slot] gives a value (a pointer in the kernel, a checking view in the simulation)
template <typename T, typename L>
BDSP_DETECT_HD bool detect_is_peak(const L& lds, int slot, int left, int right)
{
    const T c = lds[slot];
    bool peak = true;
    for (int d = 1; d <= left && peak; ++d) peak = c > lds[slot - d];
    for (int d = 1; d <= right && peak; ++d) peak = c > lds[slot + d];
    return peak;
}

// ---------------------------------------------------------------------------------------------
// places inside a tile
// ---------------------------------------------------------------------------------------------
BDSP_DETECT_HD int detect_popcount(uint64_t m)
{
    m = m - ((m >> 1) & 0x5555555555555555ull);
    m = (m & 0x3333333333333333ull) + ((m >> 2) & 0x3333333333333333ull);
    m = (m + (m >> 4)) & 0x0f0f0f0f0f0f0f0full;
    return (int)((m * 0x0101010101010101ull) >> 56);
}
// the set bits of a wave's ballot below the lane's own (the kernel takes it from the mbcnt pair, the same number)
BDSP_DETECT_HD int detect_lane_rank(uint64_t ballot, int lane) { return detect_popcount(ballot & (((uint64_t)1 << lane) - 1)); }
// the detections of the tile before segment s; seg[i]: the count of segment i
template <typename L>
BDSP_DETECT_HD unsigned detect_segment_base(const L& seg, int s)
{
    unsigned base = 0;
    for (int i = 0; i < s; ++i) base += seg[i];
    return base;
}
template <typename L>
BDSP_DETECT_HD unsigned detect_tile_total(const L& seg) { return detect_segment_base(seg, DETECT_SEGMENTS); }

// ---------------------------------------------------------------------------------------------
// the prefix launches: DETECT_SCAN_CHUNK entries at a time, 64-bit sums.  Thread t of a chunk owns the entries
// t * DETECT_SCAN_ITEMS ... + DETECT_SCAN_ITEMS - 1: it adds them up (detect_scan_own), the 256 sums are scanned in LDS by
// DETECT_SCAN_STEPS doubling steps between two buffers (detect_scan_step), and it walks its entries again from
// carry + the sums of the threads before it (detect_scan_write).
// ---------------------------------------------------------------------------------------------
BDSP_DETECT_HD size_t detect_scan_first(size_t chunk_start, int tid) { return chunk_start + (size_t)tid * DETECT_SCAN_ITEMS; }
// the sum of the thread's entries; e[i]: entry i, `entries` of them
template <typename E>
BDSP_DETECT_HD int64_t detect_scan_own(const E& e, size_t first, size_t entries)
{
    int64_t sum = 0;
    for (int k = 0; k < DETECT_SCAN_ITEMS; ++k)
        if (first + (size_t)k < entries) sum += (int64_t)e[first + (size_t)k];
    return sum;
}
// one doubling step of the inclusive scan of the 256 sums, thread tid, from one buffer to the other
template <typename L>
BDSP_DETECT_HD void detect_scan_step(const L& src, L& dst, int tid, int step)
{
    const int stride = 1 << step;
    const int64_t own = src[tid];
    const int64_t before = tid >= stride ? (int64_t)src[tid - stride] : 0;
    dst[tid] = own + before;
}
// every entry of the thread becomes the sum of the entries before it; `before`: that of the thread's first entry
template <typename E>
BDSP_DETECT_HD void detect_scan_write(E& e, size_t first, size_t entries, int64_t before)
{
    for (int k = 0; k < DETECT_SCAN_ITEMS; ++k)
        if (first + (size_t)k < entries) {
            const int64_t v = e[first + (size_t)k];
            e[first + (size_t)k] = before;
            before += v;
        }
}
// the buffer (0 or 1) that holds the inclusive scan after DETECT_SCAN_STEPS steps that started in buffer 0
BDSP_DETECT_HD int detect_scan_result_buffer() { return DETECT_SCAN_STEPS & 1; }
BDSP_DETECT_HD size_t detect_scan_chunks(size_t entries) { return (entries + DETECT_SCAN_CHUNK - 1) / DETECT_SCAN_CHUNK; }

} // namespace bdsp
