// sort_core.h -- the plan, the lane-to-slot maps, the LDS swizzle, the compare-exchange network and the merge-path split of
// sort.hip, host + device: sort, argsort, top_k and quantile, the order statistics of every row of a real matrix.  The kernels
// call these functions on their registers and LDS; tests/host_sim/sim_sort.cpp calls the SAME functions with threads as loops.
//
// Order: IEEE totalOrder on the bit patterns through the key map of rank_filter_core.h, k = rank_key(bits), unsigned;
// descending is the ascending order of the complemented key ~k.  Keys travel as keys from launch to launch; only the last
// launch turns them back into the bits of the inputs, NaN payloads and denormals included.  With an index (INDEX, the
// launches of order_select) the compare is on the pair (key, index), a strict total order: the result is the stable sort.
// Without one equal keys are equal bits, and any order of them is the same output.
//
// Tile: SORT_THREADS = 256 lanes hold SORT_TILE = 4096 elements, SORT_PER_LANE = 16 each, in registers, and run a bitonic
// network over the 12 bits of the logical slot.  A lane's 16 registers span four slot bits B .. B + 3, the lane number
// fills the other eight (sort_slot<B>): B = 0 (slots 16 t + r), B = 4 and B = 8 (slots 256 r + t, the coalesced order of
// global memory).  The compare distances inside the four bits run in registers; a change of B goes through LDS (store in
// the old layout, barrier, load in the new, barrier).  A stage of run size 2^s takes the distances 2^(s-1) .. 1: B = 8 for
// the bits 11 .. 8, B = 4 for 7 .. 4, B = 0 for 3 .. 0; the stages up to 16 need no LDS at all.  A full tile is 22 changes
// of layout.  Register arrays are indexed by constants only (every loop over r or a bit is unrolled): no scratch.
//
// LDS swizzle: logical slot s lives at word s ^ ((s >> 4) & 31) of the key array (and of the index array behind it), a
// bijection of every aligned 512-slot block.  In all three layouts the 32 lanes of a half wave then touch 32 different
// low-5-bit words for 4-byte keys and indices (ds_read_b32 / ds_write_b32: bank (a / 4) % 32 per 32-lane half), 32
// different 8-byte words for ds_read_b64 (bank (a / 4) % 64), and the 16 lanes of a ds_write_b64 group 16 different ones:
// sim_sort.cpp counts the bank cycles of every store and load of every layout change and prints the extra ones.
//
// Short rows share a workgroup: with p the power of two >= n, p <= SORT_TILE / 2, a workgroup takes SORT_TILE / p rows,
// row q in the slots q p .. q p + p - 1, and stops the network at stage size p.  The tail of a segment or a tile is padded
// with the all-ones key and the index 0xFFFFFFFF, which sort last whatever the data.
//
// Merge: one pass merges neighbouring sorted runs of `run` elements into 2 run (the last pair ragged, a lone last run
// copied); a workgroup produces SORT_TILE consecutive outputs.  Its piece is cut by the merge path: of the first d outputs
// of the pair, a(d) come from the left run, found by bisection on the diagonal with ties going to the left run -- the left
// run's indices are all below the right run's, so keys alone decide.  The bisection takes bit_length(min(la, lb)) steps,
// a function of the lengths.  The piece of A ascending, pads, and the piece of B reversed form a bitonic sequence; the 12
// half-cleaner steps sort it.  Nothing here leaves a loop early; path and time depend on (rows, n, key width, INDEX) only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rank_filter_core.h"

#if defined(__HIPCC__)
#define BDSP_SORT_HD __host__ __device__ __forceinline__
#define BDSP_SORT_UNROLL _Pragma("unroll")
#else
#define BDSP_SORT_HD inline
#define BDSP_SORT_UNROLL
#endif

namespace bdsp {

constexpr int SORT_THREADS = 256;
// elements per lane: four slot bits in registers
constexpr int SORT_PER_LANE = 16; // not measured: no other count was built
// elements per workgroup, of the tile launch and of a merge pass
constexpr int SORT_TILE = 4096; // not measured: no other tile was built
constexpr int SORT_TILE_LOG2 = 12;
constexpr int SORT_LANE_LOG2 = 4;
constexpr uint32_t SORT_PAD_INDEX = 0xFFFFFFFFu;
// the stage number that makes every compare-exchange ascending (no slot has that bit)
constexpr int SORT_ASCENDING = 30;

static_assert(SORT_TILE == SORT_THREADS * SORT_PER_LANE, "SORT_PER_LANE elements per lane");
static_assert(SORT_TILE == 1 << SORT_TILE_LOG2 && SORT_PER_LANE == 1 << SORT_LANE_LOG2, "powers of two");

// ---------------------------------------------------------------------------------------------
// keys
// ---------------------------------------------------------------------------------------------
template <typename K>
BDSP_SORT_HD K sort_to_key(K bits, bool descending)
{
    const K k = rank_key<K>(bits);
    return descending ? (K)~k : k;
}
template <typename K>
BDSP_SORT_HD K sort_to_bits(K key, bool descending)
{
    return rank_bits<K>(descending ? (K)~key : key);
}

// ---------------------------------------------------------------------------------------------
// the plan: a function of (rows, n) alone; n > 0
// ---------------------------------------------------------------------------------------------
struct SortPlan {
    int seg_log2;         // the network stops at run size 2^seg_log2: a row's segment, or the whole tile
    unsigned rows_per_wg; // rows that share a workgroup of the tile launch (1 for n > SORT_TILE / 2)
    size_t tiles;         // tiles of a row (1 where rows share)
    size_t groups;        // workgroups of the tile launch
    int passes;           // merge passes, ceil(log2(tiles))
};
BDSP_SORT_HD int sort_ceil_log2(size_t v)
{
    int s = 0;
    while (((size_t)1 << s) < v) ++s;
    return s;
}
BDSP_SORT_HD SortPlan sort_plan(size_t rows, size_t n)
{
    SortPlan p;
    if (n <= (size_t)SORT_TILE / 2) {
        p.seg_log2 = sort_ceil_log2(n);
        p.rows_per_wg = (unsigned)(SORT_TILE >> p.seg_log2);
        p.tiles = 1;
        p.groups = (rows + p.rows_per_wg - 1) / p.rows_per_wg;
    } else {
        p.seg_log2 = SORT_TILE_LOG2;
        p.rows_per_wg = 1;
        p.tiles = (n + SORT_TILE - 1) / SORT_TILE;
        p.groups = rows * p.tiles;
    }
    p.passes = sort_ceil_log2(p.tiles);
    return p;
}
// what the launches can address: 32-bit indices within a row, 31-bit grids
BDSP_SORT_HD bool sort_supported(size_t rows, size_t n)
{
    if (n > 0xffffffffu) return false;
    const size_t tiles = (n + SORT_TILE - 1) / SORT_TILE;
    return rows <= 0x7fffffffu / tiles;
}
BDSP_SORT_HD size_t sort_lds_bytes(size_t key_bytes, bool index) { return (size_t)SORT_TILE * (key_bytes + (index ? 4 : 0)); }

// the cell that logical slot `slot` of workgroup `group` of the tile launch holds
struct SortCell {
    size_t row, col;
    bool valid; // else a pad
};
BDSP_SORT_HD SortCell sort_tile_cell(const SortPlan& p, size_t rows, size_t n, size_t group, int slot)
{
    const size_t seg = (size_t)(slot >> p.seg_log2), off = (size_t)(slot & ((1 << p.seg_log2) - 1));
    SortCell c;
    if (p.tiles == 1) {
        c.row = group * p.rows_per_wg + seg;
        c.col = off;
    } else {
        c.row = group / p.tiles;
        c.col = (group % p.tiles) * (size_t)SORT_TILE + off;
    }
    c.valid = c.row < rows && c.col < n;
    return c;
}

// ---------------------------------------------------------------------------------------------
// the lane-to-slot maps and the LDS swizzle
// ---------------------------------------------------------------------------------------------
// register r of lane t holds this logical slot when the registers span the slot bits B .. B + 3
template <int B>
BDSP_SORT_HD int sort_slot(int t, int r)
{
    return ((t >> B) << (B + SORT_LANE_LOG2)) | (r << B) | (t & ((1 << B) - 1));
}
// the word of the LDS arrays that holds a logical slot
BDSP_SORT_HD int sort_phys(int slot) { return slot ^ ((slot >> 4) & 31); }

// an LDS array in the kernel; the simulation passes a checking view with the same two members
template <typename V>
struct SortLds {
    V* p;
    BDSP_SORT_HD V get(int i) const { return p[i]; }
    BDSP_SORT_HD void put(int i, V v) const { p[i] = v; }
};

template <typename K, bool INDEX>
struct SortRegs {
    K k[SORT_PER_LANE];
    uint32_t i[INDEX ? SORT_PER_LANE : 1];
};

template <int B, typename K, bool INDEX, typename LK, typename LI>
BDSP_SORT_HD void sort_lds_store(const LK& lk, const LI& li, int t, const SortRegs<K, INDEX>& g)
{
    BDSP_SORT_UNROLL
    for (int r = 0; r < SORT_PER_LANE; ++r) {
        const int w = sort_phys(sort_slot<B>(t, r));
        lk.put(w, g.k[r]);
        if constexpr (INDEX) li.put(w, g.i[r]);
    }
}
template <int B, typename K, bool INDEX, typename LK, typename LI>
BDSP_SORT_HD void sort_lds_load(const LK& lk, const LI& li, int t, SortRegs<K, INDEX>& g)
{
    BDSP_SORT_UNROLL
    for (int r = 0; r < SORT_PER_LANE; ++r) {
        const int w = sort_phys(sort_slot<B>(t, r));
        g.k[r] = lk.get(w);
        if constexpr (INDEX) g.i[r] = li.get(w);
    }
}

// ---------------------------------------------------------------------------------------------
// the network
// ---------------------------------------------------------------------------------------------
// registers a < b: afterwards a holds the smaller (down: the larger) of the two by (key, index)
template <typename K, bool INDEX>
BDSP_SORT_HD void sort_cmpx(SortRegs<K, INDEX>& g, int a, int b, bool down)
{
    const K ka = g.k[a], kb = g.k[b];
    bool gt = ka > kb;
    if constexpr (INDEX) gt = gt || (ka == kb && g.i[a] > g.i[b]);
    const bool swap = gt != down;
    g.k[a] = swap ? kb : ka;
    g.k[b] = swap ? ka : kb;
    if constexpr (INDEX) {
        const uint32_t ia = g.i[a], ib = g.i[b];
        g.i[a] = swap ? ib : ia;
        g.i[b] = swap ? ia : ib;
    }
}
// the compare-exchanges of the stage of run size 2^stage (SORT_ASCENDING: every pair ascending) at the distances
// 2^hi .. 2^lo, as far as they lie in this layout's bits B .. B + 3; a pair sorts downwards where its slots have bit `stage`
template <int B, typename K, bool INDEX>
BDSP_SORT_HD void sort_steps(SortRegs<K, INDEX>& g, int t, int stage, int hi, int lo)
{
    BDSP_SORT_UNROLL
    for (int b = SORT_LANE_LOG2 - 1; b >= 0; --b) {
        if (B + b <= hi && B + b >= lo) {
            BDSP_SORT_UNROLL
            for (int r = 0; r < SORT_PER_LANE; ++r) {
                if (!(r & (1 << b))) sort_cmpx<K, INDEX>(g, r, r | (1 << b), ((sort_slot<B>(t, r) >> stage) & 1) != 0);
            }
        }
    }
}
// the stages 1 .. min(seg_log2, 4) of the tile sort: all in the registers of layout 0
template <typename K, bool INDEX>
BDSP_SORT_HD void sort_first_stages(SortRegs<K, INDEX>& g, int t, int seg_log2)
{
    BDSP_SORT_UNROLL
    for (int s = 1; s <= SORT_LANE_LOG2; ++s)
        if (s <= seg_log2) sort_steps<0, K, INDEX>(g, t, s == seg_log2 ? SORT_ASCENDING : s, s - 1, 0);
}

// ---------------------------------------------------------------------------------------------
// the merge pass
// ---------------------------------------------------------------------------------------------
struct SortMerge {
    size_t start;    // the pair's first element within the row; run A starts here, run B at start + la
    uint32_t la, lb; // lengths of the two runs (lb == 0: a lone run, copied)
    uint32_t d0, d1; // the workgroup produces the outputs d0 .. d1 - 1 of the pair
};
BDSP_SORT_HD SortMerge sort_merge_geom(size_t n, size_t run, size_t tile)
{
    const size_t o0 = tile * (size_t)SORT_TILE, start = o0 / (2 * run) * (2 * run), left = n - start;
    SortMerge m;
    m.start = start;
    m.la = (uint32_t)(left < run ? left : run);
    m.lb = (uint32_t)(left - m.la < run ? left - m.la : run);
    m.d0 = (uint32_t)(o0 - start);
    const size_t total = (size_t)m.la + m.lb, end = (size_t)m.d0 + SORT_TILE;
    m.d1 = (uint32_t)(end < total ? end : total);
    return m;
}
BDSP_SORT_HD int sort_split_steps(uint32_t la, uint32_t lb)
{
    uint32_t v = la < lb ? la : lb;
    int s = 0;
    while (v) { ++s; v >>= 1; }
    return s;
}
// a(d) lies in [lo, hi]
BDSP_SORT_HD void sort_split_range(uint32_t d, uint32_t la, uint32_t lb, uint32_t* lo, uint32_t* hi)
{
    *lo = d > lb ? d - lb : 0;
    *hi = d < la ? d : la;
}
// one bisection step; a[i], b[i] give the keys of the two runs.  Ties go to the left run: a[mid] <= b[d - 1 - mid] means
// that a[mid] is among the first d outputs
template <typename A>
BDSP_SORT_HD void sort_split_step(const A& a, const A& b, uint32_t d, uint32_t* lo, uint32_t* hi)
{
    if (*lo < *hi) {
        const uint32_t mid = *lo + (*hi - *lo) / 2;
        if (a[mid] <= b[d - 1 - mid]) *lo = mid + 1;
        else *hi = mid;
    }
}
// logical slot e of a merge workgroup that takes na elements of A from a0 and nb of B from b0: the offset of its source
// from the pair's start (A ascending from slot 0, B reversed down from the last slot), or -1 for a pad between them
BDSP_SORT_HD int64_t sort_merge_source(int e, uint32_t a0, uint32_t na, uint32_t b0, uint32_t nb, uint32_t la)
{
    if ((uint32_t)e < na) return (int64_t)a0 + e;
    if ((uint32_t)e >= (uint32_t)SORT_TILE - nb) return (int64_t)la + b0 + (SORT_TILE - 1 - e);
    return -1;
}

} // namespace bdsp
