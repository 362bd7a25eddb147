// mat_ew.hip -- the row-aware elementwise operations of a matrix: multiply_complex_exponential, reverse and the
// wrap-around binary operations add_smaller / sub_smaller / mul_smaller / div_smaller with a matrix or one vector as
// operand (DspMat methods of the same names).  A vector is a matrix of one row: DspVec's reverse and *_smaller
// launch these kernels too (its mixer keeps elementwise.hip's packet map, which measured faster for one long row).
//
// Replaces the row loop of the reference's matrix crate (matrix/src/complex.rs:203-211, general/elementary.rs:117-198
// forward the traits to the rows one after the other); each row computes what complex_ops.rs:81-105,
// data_reorganization.rs:237-262 and elementary.rs:591-640 compute.  One launch each, whatever the row count.  The
// flat vector kernels do not fit: the phase index restarts in every row, a flat reversal also reverses the order of
// the rows, and the operand's period belongs to the row, not to the allocation.
//
//   k_mw_cexp     z[r][k] *= exp(j (a k + b)).  A workgroup owns 256 consecutive points of the row (rows shorter than
//                 that share it, floor(256 / points) side by side) and walks down the rows: the phasor depends on the
//                 position alone, so a lane forms it ONCE -- a double-precision sincos -- and then only loads one
//                 interleaved pair (8 or 16 bytes, naturally aligned), multiplies and stores, four rows in flight.
//   k_mw_reverse  out[r][i] = in[r][points - 1 - i]: whole elements as packets, lanes along the flat output.
//   k_mw_smaller  x[r][i] (.)= y[r * ystride + i mod ypoints] (ystride 0: one vector for every row), lanes along the
//                 flat matrix.
// The last two divide once per lane and carry the position, the row and the period position from one grid stride to
// the next.  The per-element arithmetic and the maps are in mat_ew_core.h (the mixer's expressions are shared with
// elementwise.hip, so a row is bit-equal to the vector call on it), tests/host_sim/sim_mat_ew.cpp runs the maps with
// threads as loops.  Built without FMA contraction, as elementwise.hip.
#include "bdsp_internal.h"
#include "mat_ew_core.h"

namespace bdsp {

static inline unsigned mw_grid(size_t blocks)
{
    size_t cap = (size_t)num_cus() * 8;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks ? blocks : 1);
}

template <typename T> struct mw_vec2 { typedef T type __attribute__((ext_vector_type(2))); };
// a whole element (a real scalar or an interleaved complex pair) as one packet
template <typename T, int ELEM> struct mw_packet_of { using type = T; };
template <typename T> struct mw_packet_of<T, 2> { using type = typename mw_vec2<T>::type; };

template <typename T>
__global__ __launch_bounds__(256) void k_mw_cexp(T* __restrict__ x, const MwCexpGeom g, double a, double b)
{
    typedef typename mw_vec2<T>::type V2;
    unsigned sub;
    unsigned long long k;
    if (!mw_cexp_lane(g, blockIdx.x, threadIdx.x, &sub, &k)) return;
    T wr, wi;
    cexp_phasor<T>(a, b, (double)k, &wr, &wi);
    V2* x2 = reinterpret_cast<V2*>(x);
    const unsigned long long gy = gridDim.y;
    for (unsigned long long rg = blockIdx.y; rg < g.row_groups; rg += 4 * gy) {
        unsigned long long at[4];
        V2 z[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned long long row = mw_cexp_row(g, rg + u * gy, sub);
            ok[u] = row < g.rows;
            at[u] = row * g.points + k;
            if (ok[u]) z[u] = x2[at[u]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!ok[u]) continue;
            T zr = z[u].x, zi = z[u].y;
            cexp_mul<T>(&zr, &zi, wr, wi);
            x2[at[u]] = V2{zr, zi};
        }
    }
}

template <typename P, typename IDX>
__global__ __launch_bounds__(256) void k_mw_reverse(const P* __restrict__ in, P* __restrict__ out, IDX total, IDX points,
                                                     IDX s_i)
{
    IDX o = (IDX)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    const IDX stride = (IDX)gridDim.x * blockDim.x;
    IDX r, i;
    mw_flat_start<IDX>(o, points, &r, &i);
    for (; o < total; o += stride) {
        out[o] = in[mw_reverse_src<IDX>(o, points, i)];
        mw_flat_step<IDX>(points, 0, s_i, &r, &i);
    }
}

// x and y may be the same matrix (ypoints == points): every lane reads its two elements before it writes
template <typename T, bool CPLX, typename IDX>
__global__ __launch_bounds__(256) void k_mw_smaller(T* x, const T* y, IDX total, IDX points, IDX ypoints, IDX ystride,
                                                     IDX s_r, IDX s_i, IDX s_j, int op)
{
    typedef typename mw_vec2<T>::type V2;
    IDX o = (IDX)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    const IDX stride = (IDX)gridDim.x * blockDim.x;
    IDX r, i;
    mw_flat_start<IDX>(o, points, &r, &i);
    IDX j = i % ypoints;
    for (; o < total; o += stride) {
        const IDX q = mw_operand_index<IDX>(r, ystride, j);
        if (CPLX) {
            V2* xp = reinterpret_cast<V2*>(x) + o;
            const V2 a = *xp, b = reinterpret_cast<const V2*>(y)[q];
            T re, im;
            smaller_complex<T>(a.x, a.y, b.x, b.y, op, &re, &im);
            *xp = V2{re, im};
        } else {
            x[o] = smaller_real<T>(x[o], y[q], op);
        }
        mw_flat_step<IDX>(points, s_r, s_i, &r, &i);
        j = mw_period_step<IDX>(j, s_j, ypoints);
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
template <typename T>
int mw_cexp(T* x, size_t rows, size_t points, double a, double b, hipStream_t s)
{
    if (rows == 0 || points == 0) return BDSP_OK;
    const MwCexpGeom g = mw_cexp_geom(rows, points);
    if (g.tiles_per_row >= (1ull << 23)) { // gridDim.x * 256 stays below 2^31
        set_last_error("multiply_complex_exponential: rows of 2^31 points or more are not supported");
        return BDSP_ERR_UNSUPPORTED;
    }
    // enough workgroups to fill the device, each walking as many rows as that leaves
    size_t gy = (size_t)num_cus() * 8 / (size_t)g.tiles_per_row;
    if (gy > g.row_groups) gy = (size_t)g.row_groups;
    if (gy > 65535) gy = 65535;
    if (gy == 0) gy = 1;
    hipLaunchKernelGGL((k_mw_cexp<T>), dim3((unsigned)g.tiles_per_row, (unsigned)gy), dim3(MW_WG), 0, s, x, g, a, b);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, int ELEM, typename IDX>
static int mw_reverse_launch(const T* in, T* out, size_t total, size_t points, hipStream_t s)
{
    typedef typename mw_packet_of<T, ELEM>::type P;
    const unsigned grid = mw_grid((total + 255) / 256);
    const size_t stride = (size_t)grid * 256;
    hipLaunchKernelGGL((k_mw_reverse<P, IDX>), dim3(grid), dim3(256), 0, s, reinterpret_cast<const P*>(in),
                       reinterpret_cast<P*>(out), (IDX)total, (IDX)points, (IDX)(stride % points));
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T>
int mw_reverse(const T* in, T* out, size_t rows, size_t points, bool is_complex, hipStream_t s)
{
    if (rows == 0 || points == 0) return BDSP_OK;
    if (in == out) return BDSP_ERR_UNSUPPORTED;
    const size_t total = rows * points;
    if (mw_fits_32(total, 0)) {
        if (is_complex) return mw_reverse_launch<T, 2, unsigned>(in, out, total, points, s);
        return mw_reverse_launch<T, 1, unsigned>(in, out, total, points, s);
    }
    if (is_complex) return mw_reverse_launch<T, 2, size_t>(in, out, total, points, s);
    return mw_reverse_launch<T, 1, size_t>(in, out, total, points, s);
}

template <typename T, bool CPLX, typename IDX>
static int mw_smaller_launch(T* x, const T* y, size_t total, size_t points, size_t ypoints, size_t ystride, int op,
                             hipStream_t s)
{
    const unsigned grid = mw_grid((total + 255) / 256);
    const size_t stride = (size_t)grid * 256;
    hipLaunchKernelGGL((k_mw_smaller<T, CPLX, IDX>), dim3(grid), dim3(256), 0, s, x, y, (IDX)total, (IDX)points,
                       (IDX)ypoints, (IDX)ystride, (IDX)(stride / points), (IDX)(stride % points), (IDX)(stride % ypoints),
                       op);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T>
int mw_smaller(T* x, const T* y, size_t rows, size_t points, size_t ypoints, size_t ystride, bool is_complex, int op,
               hipStream_t s)
{
    if (rows == 0 || points == 0) return BDSP_OK;
    if (ypoints == 0 || points % ypoints != 0) return BDSP_ERR_ARG_LENGTH;
    const size_t total = rows * points;
    if (mw_fits_32(total, ystride ? rows * ystride : ypoints)) {
        if (is_complex) return mw_smaller_launch<T, true, unsigned>(x, y, total, points, ypoints, ystride, op, s);
        return mw_smaller_launch<T, false, unsigned>(x, y, total, points, ypoints, ystride, op, s);
    }
    if (is_complex) return mw_smaller_launch<T, true, size_t>(x, y, total, points, ypoints, ystride, op, s);
    return mw_smaller_launch<T, false, size_t>(x, y, total, points, ypoints, ystride, op, s);
}

#define BDSP_INST(T)                                                                                 \
    template int mw_cexp<T>(T*, size_t, size_t, double, double, hipStream_t);                        \
    template int mw_reverse<T>(const T*, T*, size_t, size_t, bool, hipStream_t);                     \
    template int mw_smaller<T>(T*, const T*, size_t, size_t, size_t, size_t, bool, int, hipStream_t);
BDSP_INST(float)
BDSP_INST(double)
#undef BDSP_INST

} // namespace bdsp
