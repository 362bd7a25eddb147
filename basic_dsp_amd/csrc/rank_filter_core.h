// rank_filter_core.h -- the key map, the boundary index, the window, the LDS map and the two selectors of rank_filter.hip,
// host + device: rank_filter, a sliding order statistic along every row of a real matrix.  The kernel calls these functions
// on its LDS; tests/host_sim/sim_rank_filter.cpp calls the SAME functions with threads as loops.
//
// Point i of a row of n points: the window is the multiset x[i + d], guard < |d| <= half (no guard: |d| <= half, the centre
// included), W = 2 half + 1 or 2 (half - guard) values; the result is its element of rank `rank` (0 the smallest).
// Positions outside the row are read by the boundary rule: +0.0 (RANK_ZERO), index mod n (RANK_WRAP, any number of turns),
// the row's first / last point (RANK_NEAREST).
//
// Order: IEEE totalOrder on the bit patterns, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  A value enters LDS as the
// unsigned key k(bits) = bits ^ (sign ? all ones : sign bit), a strictly monotone bijection, and the selected key goes back
// through the inverse: the output carries exactly the bits of the selected input, NaN payloads and denormals included.
// The data are loaded and stored as integers; no floating-point instruction touches a value, nothing is flushed.
//
// A row is cut into tiles of RANK_TILE outputs; the grid is rows x tiles, one launch.  LDS map (keys of K): slot p of a
// tile holds the key of row position tile * RANK_TILE - half + p, p < points + 2 half (points: the tile's outputs), so
// the window of output o is the slots o .. o + 2 half, less the guard's 2 guard + 1 slots in the middle: two segments
// (RankWindow).  RANK_TILE + 2 half keys are allocated: (1024 + 2048) x 8 B = 24 KB for f64 at RANK_MAX_HALF.  Lane t
// owns the outputs t, t + 256, t + 512, t + 768: at every step of a selector the lanes of a wave read CONSECUTIVE slots,
// 32 consecutive dwords per 32-lane half for ds_read_b32 (bank (a / 4) % 32) and 64 consecutive dwords for ds_read_b64
// (bank (a / 4) % 64): conflict-free, and the global store is coalesced.  sim_rank_filter.cpp counts exactly this.
//
// Two selectors, chosen by W and the key width alone (rank_uses_count):
//   count   for every candidate c of the window, #< = the window keys below c and #<= = those at or below c; the
//           candidate with #< <= rank < #<= is the answer.  All such candidates carry the same key, so there is no
//           tie-break.  W^2 LDS reads, 2 W^2 compares per output.
//   bisect  the answer key bit by bit from the top: with the bits above b settled in `ans`, the trial is ans with bit b
//           clear and all lower bits set; #<= trial <= rank means the answer lies above it, so bit b is set.  32 (f32) or 64
//           (f64) passes over the window, bits x W reads and compares per output.
// Neither leaves a loop early: the path and the time depend on (W, key width) only, never on the data.  By operation
// count (2 W^2 against bits x W compares) the selectors meet at W = 16 (f32) and 32 (f64), by LDS reads at 32 and 64;
// measured on an MI355X they meet at W = 17 and W = 49 (profiles/rank_filter.txt, the sweep of tools/rank_filter_bench.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BDSP_RANK_HD __host__ __device__ __forceinline__
#else
#define BDSP_RANK_HD inline
#endif

namespace bdsp {

constexpr int RANK_THREADS = 256;
constexpr int RANK_PER_LANE = 4; // outputs per lane; with RANK_THREADS it makes the tile
// outputs per tile
constexpr int RANK_TILE = 1024; // not measured: no other tile was built
// the longest half window: the halo is then twice the tile
constexpr int RANK_MAX_HALF = 1024; // not measured (24 KB of LDS for f64; the cost per output grows with W, not with this)
// the count selector is taken for W at or below the crossover of the key width, the bisect selector above it
constexpr int RANK_CROSS_F32 = 17; // measured: profiles/rank_filter.txt (count 314 us = bisect 314 us at W = 17; 195 / 313 at 13, 462 / 393 at 21)
constexpr int RANK_CROSS_F64 = 49; // measured: profiles/rank_filter.txt (count 2708 us, bisect 2747 us at W = 49; 1906 / 2301 at 41, 3633 / 3184 at 57)

static_assert(RANK_TILE == RANK_THREADS * RANK_PER_LANE, "RANK_PER_LANE outputs per lane");

enum { RANK_ZERO = 0, RANK_WRAP = 1, RANK_NEAREST = 2 };

// ---------------------------------------------------------------------------------------------
// the key map: unsigned keys in IEEE totalOrder, and back
// ---------------------------------------------------------------------------------------------
template <typename K>
BDSP_RANK_HD K rank_key(K bits)
{
    constexpr K top = (K)1 << (8 * sizeof(K) - 1);
    return bits ^ ((bits & top) ? (K)~(K)0 : top);
}
template <typename K>
BDSP_RANK_HD K rank_bits(K key)
{
    constexpr K top = (K)1 << (8 * sizeof(K) - 1);
    return key ^ ((key & top) ? top : (K)~(K)0);
}

// ---------------------------------------------------------------------------------------------
// the plan: a function of (n, half, guard) alone
// ---------------------------------------------------------------------------------------------
BDSP_RANK_HD size_t rank_tiles(size_t n) { return (n + RANK_TILE - 1) / RANK_TILE; }
BDSP_RANK_HD int rank_tile_points(size_t n, size_t tile)
{
    const size_t left = n - tile * (size_t)RANK_TILE;
    return left < (size_t)RANK_TILE ? (int)left : RANK_TILE;
}
// W; guard < 0: none.  SIZE_MAX where 2 half + 1 does not fit (every rank is then below it)
BDSP_RANK_HD size_t rank_window_size(size_t half, int64_t guard)
{
    if (guard >= 0) {
        if ((uint64_t)guard >= half) return 0;
        const size_t side = half - (size_t)guard;
        return side > SIZE_MAX / 2 ? SIZE_MAX : 2 * side;
    }
    return half > (SIZE_MAX - 1) / 2 ? SIZE_MAX : 2 * half + 1;
}
// the argument rule of the call: a known boundary, guard none or below half, rank below W
BDSP_RANK_HD bool rank_args_valid(size_t half, size_t rank, int64_t guard, int boundary)
{
    if (boundary != RANK_ZERO && boundary != RANK_WRAP && boundary != RANK_NEAREST) return false;
    if (guard < -1 || (guard >= 0 && (uint64_t)guard >= half)) return false;
    return rank < rank_window_size(half, guard);
}
BDSP_RANK_HD bool rank_uses_count(size_t W, int key_bytes) { return W <= (size_t)(key_bytes == 4 ? RANK_CROSS_F32 : RANK_CROSS_F64); }

// the row index that position q (any sign) reads, or -1 where it reads +0.0; n > 0
BDSP_RANK_HD int64_t rank_src_index(int64_t q, int64_t n, int boundary)
{
    if (q >= 0 && q < n) return q;
    if (boundary == RANK_WRAP) {
        const int64_t r = q % n;
        return r < 0 ? r + n : r;
    }
    if (boundary == RANK_NEAREST) return q < 0 ? 0 : n - 1;
    return -1;
}

// ---------------------------------------------------------------------------------------------
// LDS map and the window's two segments, as slot offsets from the output's own slot o (the slot of x[i - half])
// ---------------------------------------------------------------------------------------------
BDSP_RANK_HD int rank_lds_keys(int half) { return RANK_TILE + 2 * half; }    // allocated
BDSP_RANK_HD int rank_loaded(int points, int half) { return points + 2 * half; } // filled and read
BDSP_RANK_HD int64_t rank_first_position(size_t tile, int half) { return (int64_t)(tile * (size_t)RANK_TILE) - (int64_t)half; }
BDSP_RANK_HD int rank_out_index(int tid, int k) { return k * RANK_THREADS + tid; }

struct RankWindow {
    int len_a;   // slots o .. o + len_a - 1
    int start_b; // slots o + start_b .. o + start_b + len_b - 1
    int len_b;
};
BDSP_RANK_HD RankWindow rank_window(int half, int guard)
{
    if (guard < 0) return RankWindow{2 * half + 1, 0, 0};
    return RankWindow{half - guard, half + guard + 1, half - guard};
}

// ---------------------------------------------------------------------------------------------
// the selectors; lds[slot] gives a key (a pointer in the kernel, a checking view in the simulation)
// ---------------------------------------------------------------------------------------------
template <typename K, typename L>
BDSP_RANK_HD void rank_count_segment(const L& lds, int from, int len, K c, int* lt, int* le)
{
    for (int i = 0; i < len; ++i) {
        const K k = lds[from + i];
        *lt += k < c ? 1 : 0;
        *le += k <= c ? 1 : 0;
    }
}

template <typename K, typename L>
BDSP_RANK_HD K rank_select_count(const L& lds, int o, const RankWindow& w, int rank)
{
    K ans = 0;
    for (int seg = 0; seg < 2; ++seg) {
        const int from = seg ? o + w.start_b : o, len = seg ? w.len_b : w.len_a;
        for (int j = 0; j < len; ++j) {
            const K c = lds[from + j];
            int lt = 0, le = 0;
            rank_count_segment<K>(lds, o, w.len_a, c, &lt, &le);
            rank_count_segment<K>(lds, o + w.start_b, w.len_b, c, &lt, &le);
            if (lt <= rank && rank < le) ans = c;
        }
    }
    return ans;
}

template <typename K, typename L>
BDSP_RANK_HD K rank_select_bisect(const L& lds, int o, const RankWindow& w, int rank)
{
    K ans = 0;
    for (int b = 8 * (int)sizeof(K) - 1; b >= 0; --b) {
        const K bit = (K)1 << b, trial = ans | (K)(bit - 1);
        int le = 0;
        for (int i = 0; i < w.len_a; ++i) le += lds[o + i] <= trial ? 1 : 0;
        for (int i = 0; i < w.len_b; ++i) le += lds[o + w.start_b + i] <= trial ? 1 : 0;
        if (le <= rank) ans |= bit;
    }
    return ans;
}

} // namespace bdsp
