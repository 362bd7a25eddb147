// mat_frame.hip -- the entrance and the exit of the batch API, and the index moves of a matrix's rows:
//   from_frames   a vector in HBM -> the matrix of its overlapping frames (the analysis step of an STFT)
//   overlap_add   the rows of a matrix summed back into one vector, `hop` apart (the synthesis step)
//   from_vectors  equally long vectors -> the rows of a matrix (the reference's to_mat,
//                 matrix/src/to_from_mat_conversions.rs)
//   zero_pad, swap_halves / fft_shift / ifft_shift of a vector (data_reorganization.rs:343-442, vector_types/mod.rs:
//                 171-191) or of every row of a matrix (matrix/src/time_freq.rs forwards them row by row)
// One launch each, whatever the row count.
//
// Every kernel moves whole ELEMENTS (a real scalar or an interleaved complex pair) as one packet of 4 .. 16 bytes, one
// lane per OUTPUT element along the flat output in a grid-stride loop, so stores are contiguous, neither the row count
// nor where a row or a frame starts needs a special case, and nothing assumes more alignment than the packet's own (a
// frame may start at any element).  A lane divides once and carries (row, position) from one grid stride to the next;
// indices are 32-bit whenever every flat extent allows it.  overlap_add is a gather: the lane of output i adds the
// rows that reach i in ascending order from +0 -- no atomics, so the sum is deterministic and bit-equal to the row
// loop y[r * H : r * H + F] += m[r].  The loops and maps are in mat_frame_core.h; tests/host_sim/sim_mat_frame.cpp
// runs the same functions with threads as loops.  Copies and additions only: nothing here can contract into an FMA.
#include "bdsp_internal.h"
#include "mat_frame_core.h"

namespace bdsp {

static inline unsigned mf_grid(size_t n)
{
    size_t blocks = (n + 255) / 256;
    size_t cap = (size_t)num_cus() * 8;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks ? blocks : 1);
}

template <typename T> struct mf_vec2 { typedef T type __attribute__((ext_vector_type(2))); };
// a whole element as one packet
template <typename T, int ELEM> struct mf_packet_of { using type = T; };
template <typename T> struct mf_packet_of<T, 2> { using type = typename mf_vec2<T>::type; };

#define BDSP_MF_LANE (IDX)blockIdx.x * blockDim.x + threadIdx.x, (IDX)gridDim.x * blockDim.x

template <typename P, typename IDX>
__global__ __launch_bounds__(256) void k_mf_from_frames(const P* __restrict__ x, P* __restrict__ out, IDX total, IDX Pn,
                                                         IDX F, IDX H)
{
    mf_lane_from_frames<P, IDX>(x, out, total, Pn, F, H, BDSP_MF_LANE);
}

template <typename P, typename IDX>
__global__ __launch_bounds__(256) void k_mf_overlap_add(const P* __restrict__ m, P* __restrict__ y, IDX total, IDX rows,
                                                         IDX F, IDX H)
{
    mf_lane_overlap_add<P, IDX>(m, y, total, rows, F, H, BDSP_MF_LANE);
}

template <typename P, typename IDX>
__global__ __launch_bounds__(256) void k_mf_from_vectors(const P* const* __restrict__ vectors, P* __restrict__ out,
                                                          IDX total, IDX points)
{
    mf_lane_from_vectors<P, IDX>(vectors, out, total, points, BDSP_MF_LANE);
}

template <typename P, typename IDX>
__global__ __launch_bounds__(256) void k_mf_zero_pad(const P* __restrict__ in, P* __restrict__ out, IDX total, IDX pb,
                                                      IDX points, const MfPad<IDX> pad)
{
    mf_lane_zero_pad<P, IDX>(in, out, total, pb, points, pad, BDSP_MF_LANE);
}

template <typename P, typename IDX>
__global__ __launch_bounds__(256) void k_mf_rotate(const P* __restrict__ in, P* __restrict__ out, IDX total, IDX points,
                                                    IDX shift)
{
    mf_lane_rotate<P, IDX>(in, out, total, points, shift, BDSP_MF_LANE);
}

#undef BDSP_MF_LANE

// ---------------------------------------------------------------------------------------------
// launchers: KERNEL<P, IDX>(BDSP_MF_ARGS(P, IDX)) over `total` output elements, P = the element packet, IDX = 32-bit
// indices when `total` and `other` (the largest extent read) allow
// ---------------------------------------------------------------------------------------------
#define BDSP_MF_LAUNCH(KERNEL, total, other)                                                                  \
    do {                                                                                                      \
        const dim3 grid_(mf_grid(total)), block_(256);                                                        \
        if (is_complex) {                                                                                     \
            using P = typename mf_packet_of<T, 2>::type;                                                      \
            if (mf_fits_32(total, other)) hipLaunchKernelGGL((KERNEL<P, unsigned>), grid_, block_, 0, s, BDSP_MF_ARGS(P, unsigned)); \
            else hipLaunchKernelGGL((KERNEL<P, size_t>), grid_, block_, 0, s, BDSP_MF_ARGS(P, size_t));       \
        } else {                                                                                              \
            using P = T;                                                                                      \
            if (mf_fits_32(total, other)) hipLaunchKernelGGL((KERNEL<P, unsigned>), grid_, block_, 0, s, BDSP_MF_ARGS(P, unsigned)); \
            else hipLaunchKernelGGL((KERNEL<P, size_t>), grid_, block_, 0, s, BDSP_MF_ARGS(P, size_t));       \
        }                                                                                                     \
        BDSP_LAUNCH_CHECK();                                                                                  \
    } while (0)

template <typename T>
int mf_from_frames(const T* x, T* out, size_t points, size_t rows, size_t frame_points, size_t hop, bool is_complex,
                   hipStream_t s)
{
    if (rows == 0 || frame_points == 0 || hop == 0) return BDSP_OK;
    const size_t total = rows * frame_points;
    // a hop past the end reads nothing but zeros from the second frame on, as a hop of exactly `points` does: r * hop
    // stays below 2 * points + frame_points
    const size_t h = hop < points ? hop : points;
#define BDSP_MF_ARGS(P, I) reinterpret_cast<const P*>(x), reinterpret_cast<P*>(out), (I)total, (I)points, (I)frame_points, (I)h
    BDSP_MF_LAUNCH(k_mf_from_frames, total, points);
#undef BDSP_MF_ARGS
    return BDSP_OK;
}

template <typename T>
int mf_overlap_add(const T* m, T* y, size_t rows, size_t frame_points, size_t hop, bool is_complex, hipStream_t s)
{
    if (rows == 0 || hop == 0) return BDSP_OK;
    if (m == y) return BDSP_ERR_UNSUPPORTED;
    const size_t h = rows == 1 ? (frame_points ? frame_points : 1) : hop; // one row: the hop moves nothing
    const size_t total = mf_ola_points(rows, frame_points, h); // empty rows: (rows - 1) * hop zeros
    if (total == 0) return BDSP_OK;
#define BDSP_MF_ARGS(P, I) reinterpret_cast<const P*>(m), reinterpret_cast<P*>(y), (I)total, (I)rows, (I)frame_points, (I)h
    BDSP_MF_LAUNCH(k_mf_overlap_add, total, rows * frame_points);
#undef BDSP_MF_ARGS
    return BDSP_OK;
}

template <typename T>
int mf_from_vectors(const T* const* vectors, T* out, size_t rows, size_t points, bool is_complex, hipStream_t s)
{
    if (rows == 0 || points == 0) return BDSP_OK;
    const size_t total = rows * points;
#define BDSP_MF_ARGS(P, I) reinterpret_cast<const P* const*>(vectors), reinterpret_cast<P*>(out), (I)total, (I)points
    BDSP_MF_LAUNCH(k_mf_from_vectors, total, 0);
#undef BDSP_MF_ARGS
    return BDSP_OK;
}

template <typename T>
int mf_zero_pad(const T* in, T* out, size_t rows, size_t points_before, size_t points, bool is_complex, int option,
                hipStream_t s)
{
    if (points <= points_before) return BDSP_ERR_ARG_LENGTH;
    if (rows == 0) return BDSP_OK;
    if (in == out) return BDSP_ERR_UNSUPPORTED;
    const size_t total = rows * points;
    size_t d0, n0, d1, s1, n1;
    mf_pad_geom(points_before, points, option, &d0, &n0, &d1, &s1, &n1);
#define BDSP_MF_ARGS(P, I) reinterpret_cast<const P*>(in), reinterpret_cast<P*>(out), (I)total, (I)points_before, (I)points, MfPad<I>{(I)d0, (I)n0, (I)d1, (I)s1, (I)n1}
    BDSP_MF_LAUNCH(k_mf_zero_pad, total, 0);
#undef BDSP_MF_ARGS
    return BDSP_OK;
}

template <typename T>
int mf_rotate(const T* in, T* out, size_t rows, size_t points, size_t shift, bool is_complex, hipStream_t s)
{
    if (rows == 0 || points == 0) return BDSP_OK;
    if (in == out) return BDSP_ERR_UNSUPPORTED;
    const size_t total = rows * points, sh = shift % points;
#define BDSP_MF_ARGS(P, I) reinterpret_cast<const P*>(in), reinterpret_cast<P*>(out), (I)total, (I)points, (I)sh
    BDSP_MF_LAUNCH(k_mf_rotate, total, 0);
#undef BDSP_MF_ARGS
    return BDSP_OK;
}

#undef BDSP_MF_LAUNCH

#define BDSP_INST(T)                                                                                          \
    template int mf_from_frames<T>(const T*, T*, size_t, size_t, size_t, size_t, bool, hipStream_t);          \
    template int mf_overlap_add<T>(const T*, T*, size_t, size_t, size_t, bool, hipStream_t);                  \
    template int mf_from_vectors<T>(const T* const*, T*, size_t, size_t, bool, hipStream_t);                  \
    template int mf_zero_pad<T>(const T*, T*, size_t, size_t, size_t, bool, int, hipStream_t);                \
    template int mf_rotate<T>(const T*, T*, size_t, size_t, size_t, bool, hipStream_t);
BDSP_INST(float)
BDSP_INST(double)
#undef BDSP_INST

} // namespace bdsp
