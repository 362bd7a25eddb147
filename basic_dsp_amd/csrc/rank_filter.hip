// rank_filter.hip -- rank_filter: the element of a given rank of a sliding window along every row of a real f32 / f64
// matrix (rank_filter_core.h has the order, the boundary rules, the LDS map and both selectors).
//
// One launch whatever the row count; the grid is rows x tiles of RANK_TILE outputs:
//   k_rank_tile  the workgroup loads its tile and a halo of `half` positions on each side into LDS, applying the boundary
//                rule and turning every value into its integer key once; every lane then selects its four outputs with
//                the count selector (COUNT) or the bisect selector, turns the key back into the value's bits and stores.
// A tile reads its neighbours' input, so the rows go from `in` to `out`, two buffers; the caller trades them.  Rows are
// read and written as integers, one value per lane and step: rows need not start on a 16-byte boundary.  Plain loads and
// stores only; every output is written by exactly one thread, once; no register array, so there is no scratch.
// tests/host_sim/sim_rank_filter.cpp runs the functions of rank_filter_core.h with threads as loops.
#include <type_traits>

#include "bdsp_internal.h"
#include "rank_filter_core.h"

namespace bdsp {

extern __shared__ __align__(16) unsigned char rank_smem[];

// blockIdx.x = row * tiles + tile
template <typename K, bool COUNT>
__global__ __launch_bounds__(RANK_THREADS) void k_rank_tile(const K* __restrict__ in, K* __restrict__ out, size_t n, unsigned tiles,
                                                             int half, int guard, int rank, int boundary)
{
    K* lds = reinterpret_cast<K*>(rank_smem);
    const int tid = (int)threadIdx.x;
    const size_t row = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int points = rank_tile_points(n, tile), loaded = rank_loaded(points, half);
    const K* src = in + row * n;
    const int64_t first = rank_first_position(tile, half);
    for (int p = tid; p < loaded; p += RANK_THREADS) {
        const int64_t g = rank_src_index(first + p, (int64_t)n, boundary);
        lds[p] = rank_key<K>(g < 0 ? (K)0 : src[g]);
    }
    __syncthreads();
    const RankWindow w = rank_window(half, guard);
    K* dst = out + row * n + tile * (size_t)RANK_TILE;
    for (int k = 0; k < RANK_PER_LANE; ++k) {
        const int o = rank_out_index(tid, k);
        if (o < points) dst[o] = rank_bits<K>(COUNT ? rank_select_count<K>(lds, o, w, rank) : rank_select_bisect<K>(lds, o, w, rank));
    }
}

template <typename K, bool COUNT>
static int rank_launch(const K* in, K* out, size_t rows, size_t n, int half, int guard, int rank, int boundary, hipStream_t s)
{
    const size_t tiles = rank_tiles(n), lds = sizeof(K) * (size_t)rank_lds_keys(half);
    auto kern = k_rank_tile<K, COUNT>;
    BDSP_TRY(kernel_lds(kern, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(rows * tiles)), dim3(RANK_THREADS), lds, s, in, out, n, (unsigned)tiles, half, guard, rank, boundary);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// in, out: rows x n values of T as their bit patterns, two buffers; rows, n > 0, half <= RANK_MAX_HALF and
// rank_args_valid(half, rank, guard, boundary)
template <typename T>
int rank_filter_rows(const T* in, T* out, size_t rows, size_t n, size_t half, size_t rank, int64_t guard, int boundary, hipStream_t s)
{
    using K = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
    if (rows > 0x7fffffffu / rank_tiles(n)) { set_last_error("rank_filter: rows x tiles above 2^31"); return BDSP_ERR_UNSUPPORTED; }
    const K* a = reinterpret_cast<const K*>(in);
    K* b = reinterpret_cast<K*>(out);
    if (rank_uses_count(rank_window_size(half, guard), (int)sizeof(K)))
        return rank_launch<K, true>(a, b, rows, n, (int)half, (int)guard, (int)rank, boundary, s);
    return rank_launch<K, false>(a, b, rows, n, (int)half, (int)guard, (int)rank, boundary, s);
}

template int rank_filter_rows<float>(const float*, float*, size_t, size_t, size_t, size_t, int64_t, int, hipStream_t);
template int rank_filter_rows<double>(const double*, double*, size_t, size_t, size_t, size_t, int64_t, int, hipStream_t);

} // namespace bdsp
