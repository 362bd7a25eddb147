// mat_transpose.hip -- the one move of the batch API that goes ACROSS the rows: an out-of-place transpose of an [R][C]
// array of elements into [C][R].  It serves
//   transpose          the rows of a matrix become its columns, so every row operation works down the columns
//   from_interleaved   a vector of interleaved channels -> channels x samples (the reference's split_into,
//                      vector/src/vector_types/general/data_reorganization.rs, with the rows of one matrix as targets)
//   to_interleaved     the inverse (the reference's merge)
// One launch each.  An element is a real scalar or an interleaved complex pair and moves as ONE packet of 4, 8 or 16
// bytes (f32; c32 or f64; c64); the kernels are instantiated per packet SIZE, so f64 and c32 share theirs.  Copies
// only, bit-exact.
//
// Alignment: a row may start at any element (an f32 row of odd length puts row 1 on a 4-byte boundary), so every global
// load and store is one element wide and assumes the element's own alignment, nothing more.
//
// Tiled path (k_tp_tiled): a workgroup of 256 threads moves one square tile of S x S elements through LDS, S = 64 for
// 4- and 8-byte elements and 32 for 16-byte ones.  It loads along source rows (a wave instruction reads one run of
// 256 or 512 bytes, or two of 512 for S = 32) and stores along destination rows (the same runs); partial tiles mask
// the lanes past the edge.  The grid is flat over the tiles, t = tile row * tiles per row + tile column, decomposed in
// the kernel, so no row count reaches the y / z limit of a launch.
//
// LDS pitch: S + 1 elements (65 / 130 / 132 dwords for 4 / 8 / 16 bytes), written row-wise, read column-wise.  From
// the bank rules of the LDS (bank = (byte address / 4) mod 32 for every ds_write and for ds_read_b32, mod 64 for
// ds_read_b64 and ds_read_b128; lanes conflict only inside one lane group):
//   row-wise ds_write_b32 / b64 / b128 (groups of 32 / 16 / 8 contiguous lanes): a group writes 32 consecutive dwords
//                       of one tile row -- 32 distinct banks, 0 conflicts;
//   column-wise ds_read_b32  (2 groups of 32 lanes): lane l reads dword 65 l + c; 65 is odd, so 32 consecutive l give
//                       32 distinct banks mod 32 -- 0 conflicts;
//   column-wise ds_read_b64  (2 groups of 32 lanes): lane l reads dwords 130 l + 2 c, + 1; 130 = 2 * 65, so the pairs
//                       start on 2 * (65 l mod 32): 32 distinct even banks mod 64 -- 0 conflicts;
//   column-wise ds_read_b128 (4 groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32): lane l
//                       reads dwords 132 l' + 4 c .. + 3 with l' = l mod 32 the tile row; 132 = 4 * 33, so the quads
//                       start on 4 * (33 l' mod 16), and the l' of every group are distinct mod 16 -- 0 conflicts.
// Conflict count of both sides of the tile, every element size: 0.  (Where the compiler pairs two of a thread's reads
// into one ds_read2_b32 / ds_read2_b64, each half is served as an access of its own at mod 32, in groups of 32 / 16
// contiguous lanes: 65 l and 2 * (65 l mod 16) are distinct there too.)  tests/host_sim/sim_mat_transpose.cpp computes
// the same numbers from tp_lds_slot and the lane groups, and 16- to 32-way for a pitch of S, to show the rule bites.
//
// Thin matrices (k_tp_flat): when the shorter side is below TP_THIN = 16 (70000 x 3, 8 x 1000000, N x 1) a square tile
// would idle most of its lanes, so the flat element-wise map has a path of its own: one lane per element along the
// flat side whose INNER dimension is the short one, grid-stride; the other side is reached in K runs of 64 / K
// consecutive elements per wave, which the next waves continue.  The launcher picks the path from (R, C) alone.
//
// No scratch, no atomics, no stream or device synchronisation; the launcher holds no loop.  Indices are 32-bit
// whenever R * C allows.  The geometry, the lane maps and the load and store loops are in mat_transpose_core.h;
// tests/host_sim/sim_mat_transpose.cpp runs the same functions with threads as loops.
#include "bdsp_internal.h"
#include "mat_transpose_core.h"

namespace bdsp {

// the element packets by size
template <int BYTES> struct tp_packet_of;
template <> struct tp_packet_of<4> { using type = unsigned; };
template <> struct tp_packet_of<8> { using type = unsigned long long; };
template <> struct tp_packet_of<16> { typedef unsigned type __attribute__((ext_vector_type(4))); };

template <typename P, typename IDX>
__global__ __launch_bounds__(TP_THREADS) void k_tp_tiled(const P* __restrict__ src, P* __restrict__ dst, IDX R, IDX C,
                                                          IDX tiles_c, IDX ntiles)
{
    constexpr int S = tp_tile_side(sizeof(P));
    __shared__ P tile[tp_lds_elems(S)];
    // one trip unless there are more tiles than a grid may have blocks
    for (IDX t = blockIdx.x; t < ntiles; t += gridDim.x) {
        IDX r0, c0;
        tp_tile_origin<IDX>(t, tiles_c, S, &r0, &c0);
        tp_lane_load<P, IDX, S>(src, tile, R, C, r0, c0, (int)threadIdx.x);
        __syncthreads();
        tp_lane_store<P, IDX, S>(tile, dst, R, C, r0, c0, (int)threadIdx.x);
        __syncthreads();
    }
}

template <typename P, typename IDX>
__global__ __launch_bounds__(TP_THREADS) void k_tp_flat(const P* __restrict__ src, P* __restrict__ dst, IDX total, IDX N,
                                                         IDX K, bool near_is_src)
{
    tp_lane_flat<P, IDX>(src, dst, total, N, K, near_is_src, (IDX)blockIdx.x * blockDim.x + threadIdx.x,
                         (IDX)gridDim.x * blockDim.x);
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
template <typename P, typename IDX>
static int tp_launch(const void* src, void* dst, size_t R, size_t C, hipStream_t s)
{
    const P* in = reinterpret_cast<const P*>(src);
    P* out = reinterpret_cast<P*>(dst);
    const size_t total = R * C;
    if (tp_is_thin(R, C)) {
        const bool near_is_src = C <= R; // few columns: the source is the [N][K] side
        const size_t N = near_is_src ? R : C, K = near_is_src ? C : R;
        size_t blocks = (total + TP_THREADS - 1) / TP_THREADS;
        const size_t cap = (size_t)num_cus() * 8;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL((k_tp_flat<P, IDX>), dim3((unsigned)blocks), dim3(TP_THREADS), 0, s, in, out, (IDX)total, (IDX)N,
                           (IDX)K, near_is_src);
    } else {
        constexpr int S = tp_tile_side(sizeof(P));
        const size_t tiles_c = tp_tiles_along(C, S), ntiles = tp_tiles_along(R, S) * tiles_c;
        const size_t blocks = ntiles < 0x7fffffffu ? ntiles : 0x7fffffffu;
        hipLaunchKernelGGL((k_tp_tiled<P, IDX>), dim3((unsigned)blocks), dim3(TP_THREADS), 0, s, in, out, (IDX)R, (IDX)C,
                           (IDX)tiles_c, (IDX)ntiles);
    }
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <int BYTES>
static int tp_launch_bytes(const void* src, void* dst, size_t R, size_t C, hipStream_t s)
{
    using P = typename tp_packet_of<BYTES>::type;
    if (tp_fits_32(R * C)) return tp_launch<P, unsigned>(src, dst, R, C, s);
    return tp_launch<P, size_t>(src, dst, R, C, s);
}

// src: R rows of C elements (complex pairs if is_complex) -> dst: C rows of R elements; src and dst must not overlap
template <typename T>
int tp_transpose(const T* src, T* dst, size_t R, size_t C, bool is_complex, hipStream_t s)
{
    if (R == 0 || C == 0) return BDSP_OK;
    if (src == dst) return BDSP_ERR_UNSUPPORTED;
    constexpr int E = (int)sizeof(T);
    if (is_complex) return tp_launch_bytes<2 * E>(src, dst, R, C, s);
    return tp_launch_bytes<E>(src, dst, R, C, s);
}

template int tp_transpose<float>(const float*, float*, size_t, size_t, bool, hipStream_t);
template int tp_transpose<double>(const double*, double*, size_t, size_t, bool, hipStream_t);

} // namespace bdsp
