// sort.hip -- sort and order_select: every row of a real f32 / f64 matrix in IEEE totalOrder on the bit patterns, in place,
// or the (index, value) pairs of requested ranks of every row (sort_core.h has the order, the plan, the lane-to-slot maps, the
// LDS swizzle, the network and the merge-path split).
//
// 1 + P launches for sort and 2 + P for order_select, P = ceil(log2(ceil(n / SORT_TILE))), whatever the row count:
//   k_sort_tile    a workgroup loads SORT_TILE elements -- one tile of a long row, or SORT_TILE / p short rows, p the power of
//                  two >= n -- as keys (complemented for descending, the tail padded with all ones), 16 per lane in
//                  registers, and runs the bitonic network up to run size p or SORT_TILE; compare distances below 16 run in
//                  registers, a change of the four register bits goes through LDS
//   k_sort_merge   one pass: neighbouring runs of `run` elements become runs of 2 run; a workgroup finds its piece of the two
//                  runs by the merge path, loads A ascending and B reversed and runs the 12 bitonic-merge steps
//   k_sort_gather  order_select only: index and value bits of the requested ranks of every row
// Keys travel as keys; the last launch of sort turns them back into bits.  With INDEX the compare is on (key, u32 index): the
// stable sort.  Rows are read and written as integers, one value per lane and step: they need not start on a 16-byte
// boundary.  Plain loads and stores only, every output is written by exactly one thread, once; no workgroup waits for
// another; no loop leaves early.  Register arrays are indexed by constants only, so there is no scratch.
// tests/host_sim/sim_sort.cpp runs the functions of sort_core.h with threads as loops.
#include <type_traits>

#include "bdsp_internal.h"
#include "sort_core.h"

namespace bdsp {

extern __shared__ __align__(16) unsigned char sort_smem[];

// the registers from layout FROM to layout TO through LDS
template <int FROM, int TO, typename K, bool INDEX>
__device__ __forceinline__ void sort_relayout(const SortLds<K>& lk, const SortLds<uint32_t>& li, int t, SortRegs<K, INDEX>& g)
{
    sort_lds_store<FROM, K, INDEX>(lk, li, t, g);
    __syncthreads();
    sort_lds_load<TO, K, INDEX>(lk, li, t, g);
    __syncthreads();
}

// in -> out_k (and out_i): may be the same buffer, a workgroup reads all of its cells before it writes any
template <typename K, bool INDEX>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_tile(const K* in, K* out_k, uint32_t* out_i, size_t rows, size_t n, SortPlan plan,
                                                             int descending, int to_bits)
{
    const SortLds<K> lk{reinterpret_cast<K*>(sort_smem)};
    const SortLds<uint32_t> li{reinterpret_cast<uint32_t*>(sort_smem + sizeof(K) * SORT_TILE)};
    const int t = (int)threadIdx.x, sp = plan.seg_log2;
    SortRegs<K, INDEX> g;
#pragma unroll
    for (int r = 0; r < SORT_PER_LANE; ++r) {
        const SortCell c = sort_tile_cell(plan, rows, n, blockIdx.x, sort_slot<8>(t, r));
        g.k[r] = c.valid ? sort_to_key<K>(in[c.row * n + c.col], descending != 0) : (K)~(K)0;
        if constexpr (INDEX) g.i[r] = c.valid ? (uint32_t)c.col : SORT_PAD_INDEX;
    }
    sort_relayout<8, 0, K, INDEX>(lk, li, t, g);
    sort_first_stages<K, INDEX>(g, t, sp);
    for (int s = SORT_LANE_LOG2 + 1; s <= sp; ++s) {
        const int stage = s == sp ? SORT_ASCENDING : s;
        if (s > 8) {
            sort_relayout<0, 8, K, INDEX>(lk, li, t, g);
            sort_steps<8, K, INDEX>(g, t, stage, s - 1, 8);
            sort_relayout<8, 4, K, INDEX>(lk, li, t, g);
        } else {
            sort_relayout<0, 4, K, INDEX>(lk, li, t, g);
        }
        sort_steps<4, K, INDEX>(g, t, stage, s - 1 < 7 ? s - 1 : 7, 4);
        sort_relayout<4, 0, K, INDEX>(lk, li, t, g);
        sort_steps<0, K, INDEX>(g, t, stage, 3, 0);
    }
    sort_relayout<0, 8, K, INDEX>(lk, li, t, g);
#pragma unroll
    for (int r = 0; r < SORT_PER_LANE; ++r) {
        const SortCell c = sort_tile_cell(plan, rows, n, blockIdx.x, sort_slot<8>(t, r));
        if (c.valid) {
            out_k[c.row * n + c.col] = to_bits ? sort_to_bits<K>(g.k[r], descending != 0) : g.k[r];
            if constexpr (INDEX) out_i[c.row * n + c.col] = g.i[r];
        }
    }
}

// blockIdx.x = row * tiles + tile; src and dst are two buffers
template <typename K, bool INDEX>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_merge(const K* __restrict__ src_k, const uint32_t* __restrict__ src_i, K* __restrict__ dst_k,
                                                              uint32_t* __restrict__ dst_i, size_t n, unsigned tiles, size_t run, int descending,
                                                              int to_bits)
{
    const SortLds<K> lk{reinterpret_cast<K*>(sort_smem)};
    const SortLds<uint32_t> li{reinterpret_cast<uint32_t*>(sort_smem + sizeof(K) * SORT_TILE)};
    const int t = (int)threadIdx.x;
    const size_t row = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const SortMerge m = sort_merge_geom(n, run, tile);
    const size_t base = row * n + m.start;
    const K *a = src_k + base, *b = a + m.la;
    uint32_t lo0, hi0, lo1, hi1;
    sort_split_range(m.d0, m.la, m.lb, &lo0, &hi0);
    sort_split_range(m.d1, m.la, m.lb, &lo1, &hi1);
    for (int step = sort_split_steps(m.la, m.lb); step > 0; --step) {
        sort_split_step(a, b, m.d0, &lo0, &hi0);
        sort_split_step(a, b, m.d1, &lo1, &hi1);
    }
    const uint32_t a0 = lo0, na = lo1 - lo0, b0 = m.d0 - lo0, nb = (m.d1 - m.d0) - na;
    SortRegs<K, INDEX> g;
#pragma unroll
    for (int r = 0; r < SORT_PER_LANE; ++r) {
        const int64_t src = sort_merge_source(sort_slot<8>(t, r), a0, na, b0, nb, m.la);
        g.k[r] = src >= 0 ? src_k[base + (size_t)src] : (K)~(K)0;
        if constexpr (INDEX) g.i[r] = src >= 0 ? src_i[base + (size_t)src] : SORT_PAD_INDEX;
    }
    sort_steps<8, K, INDEX>(g, t, SORT_ASCENDING, 11, 8);
    sort_relayout<8, 4, K, INDEX>(lk, li, t, g);
    sort_steps<4, K, INDEX>(g, t, SORT_ASCENDING, 7, 4);
    sort_relayout<4, 0, K, INDEX>(lk, li, t, g);
    sort_steps<0, K, INDEX>(g, t, SORT_ASCENDING, 3, 0);
    sort_relayout<0, 8, K, INDEX>(lk, li, t, g);
    const uint32_t produced = m.d1 - m.d0;
#pragma unroll
    for (int r = 0; r < SORT_PER_LANE; ++r) {
        const uint32_t e = (uint32_t)sort_slot<8>(t, r);
        if (e < produced) {
            dst_k[base + m.d0 + e] = to_bits ? sort_to_bits<K>(g.k[r], descending != 0) : g.k[r];
            if constexpr (INDEX) dst_i[base + m.d0 + e] = g.i[r];
        }
    }
}

// entry e = row * count + j: the element of rank ranks[j] (ranks null: j) of the sorted row
template <typename K>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_gather(const K* __restrict__ keys, const uint32_t* __restrict__ idx, size_t n, size_t count,
                                                               size_t entries, const uint64_t* __restrict__ ranks, int descending,
                                                               int64_t* __restrict__ index, K* __restrict__ value)
{
    const size_t e = (size_t)blockIdx.x * SORT_THREADS + threadIdx.x;
    if (e >= entries) return;
    const size_t row = e / count, j = e % count, at = row * n + (ranks ? (size_t)ranks[j] : j);
    if (index) index[e] = (int64_t)idx[at];
    if (value) value[e] = sort_to_bits<K>(keys[at], descending != 0);
}

template <typename K, bool INDEX>
static int sort_launch_tile(const K* in, K* out_k, uint32_t* out_i, size_t rows, size_t n, const SortPlan& plan, bool descending, bool to_bits,
                            hipStream_t s)
{
    const size_t lds = sort_lds_bytes(sizeof(K), INDEX);
    auto kern = k_sort_tile<K, INDEX>;
    BDSP_TRY(kernel_lds(kern, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)plan.groups), dim3(SORT_THREADS), lds, s, in, out_k, out_i, rows, n, plan, (int)descending, (int)to_bits);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename K, bool INDEX>
static int sort_launch_merge(const K* src_k, const uint32_t* src_i, K* dst_k, uint32_t* dst_i, size_t rows, size_t n, const SortPlan& plan,
                             size_t run, bool descending, bool to_bits, hipStream_t s)
{
    const size_t lds = sort_lds_bytes(sizeof(K), INDEX);
    auto kern = k_sort_merge<K, INDEX>;
    BDSP_TRY(kernel_lds(kern, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(rows * plan.tiles)), dim3(SORT_THREADS), lds, s, src_k, src_i, dst_k, dst_i, n, (unsigned)plan.tiles, run, (int)descending, (int)to_bits);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// data, buf: rows x n values of T as their bit patterns, two buffers; rows, n > 0 and sort_supported(rows, n).  The sorted rows
// end in buf iff *in_buf.  1 + P launches
template <typename T>
int sort_rows(T* data, T* buf, size_t rows, size_t n, bool descending, bool* in_buf, hipStream_t s)
{
    using K = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
    const SortPlan plan = sort_plan(rows, n);
    K *cur = reinterpret_cast<K*>(data), *other = reinterpret_cast<K*>(buf);
    BDSP_TRY((sort_launch_tile<K, false>(cur, cur, nullptr, rows, n, plan, descending, plan.passes == 0, s)));
    size_t run = SORT_TILE;
    for (int pass = 0; pass < plan.passes; ++pass, run *= 2) {
        BDSP_TRY((sort_launch_merge<K, false>(cur, nullptr, other, nullptr, rows, n, plan, run, descending, pass + 1 == plan.passes, s)));
        K* x = cur; cur = other; other = x;
    }
    *in_buf = plan.passes % 2 != 0;
    return BDSP_OK;
}

// x: rows x n values (not modified); ws_a, ws_b: sort_select_ws_bytes each (ws_b only for rows of more than one tile); ranks:
// null (0 .. count - 1) or count ranks below n on the device; index, value: rows x count entries on the device, each may be
// null.  rows, n, count > 0 and sort_supported(rows, n).  2 + P launches
size_t sort_select_ws_bytes(size_t rows, size_t n, size_t key_bytes) { return rows * n * (key_bytes + 4); }
template <typename T>
int sort_select_rows(const T* x, size_t rows, size_t n, bool descending, size_t count, const uint64_t* ranks, void* ws_a, void* ws_b,
                     int64_t* index, T* value, hipStream_t s)
{
    using K = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
    const SortPlan plan = sort_plan(rows, n);
    const size_t entries = rows * count, blocks = (entries + SORT_THREADS - 1) / SORT_THREADS;
    if (blocks > 0x7fffffffu) { set_last_error("order_select: rows x count above 2^39"); return BDSP_ERR_UNSUPPORTED; }
    K *cur_k = reinterpret_cast<K*>(ws_a), *other_k = reinterpret_cast<K*>(ws_b);
    uint32_t *cur_i = reinterpret_cast<uint32_t*>(cur_k + rows * n), *other_i = reinterpret_cast<uint32_t*>(other_k + rows * n);
    BDSP_TRY((sort_launch_tile<K, true>(reinterpret_cast<const K*>(x), cur_k, cur_i, rows, n, plan, descending, false, s)));
    size_t run = SORT_TILE;
    for (int pass = 0; pass < plan.passes; ++pass, run *= 2) {
        BDSP_TRY((sort_launch_merge<K, true>(cur_k, cur_i, other_k, other_i, rows, n, plan, run, descending, false, s)));
        K* xk = cur_k; cur_k = other_k; other_k = xk;
        uint32_t* xi = cur_i; cur_i = other_i; other_i = xi;
    }
    hipLaunchKernelGGL(k_sort_gather<K>, dim3((unsigned)blocks), dim3(SORT_THREADS), 0, s, cur_k, cur_i, n, count, entries, ranks, (int)descending,
                       index, reinterpret_cast<K*>(value));
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template int sort_rows<float>(float*, float*, size_t, size_t, bool, bool*, hipStream_t);
template int sort_rows<double>(double*, double*, size_t, size_t, bool, bool*, hipStream_t);
template int sort_select_rows<float>(const float*, size_t, size_t, bool, size_t, const uint64_t*, void*, void*, int64_t*, float*, hipStream_t);
template int sort_select_rows<double>(const double*, size_t, size_t, bool, size_t, const uint64_t*, void*, void*, int64_t*, double*, hipStream_t);

} // namespace bdsp
