// mat_interp.hip -- time-domain smoothing and real-row resampling of a matrix (DspMat.convolve with an impulse-response
// function, convolve_complex, interpolate_lin, interpolate_hermite).
//
// Replaces the row loop of the reference's matrix crate (matrix/src/time_freq.rs:329-387 forwards the traits to the rows
// one after the other); each row computes what convolve_function_priv (time_freq/mod.rs:174-213) and
// real_interpolation.rs:33-176 compute.  One launch each, whatever the row count.
//
//   k_mt_interp_lin / k_mt_interp_hermite   one lane per element of the flat output [rows][dest_len], grid-stride; the
//                     arithmetic is interp.hip's (mat_interp_core.h), so a row is bit-equal to the vector call on it
//   k_mt_conv_direct  y[r][i] = sum_{k=0}^{2L} x[r][(i - L + k) mod N] * w[k], accumulated over ascending k in T.  A
//                     workgroup owns a tile of one row, or a whole number of rows shorter than the workgroup, and keeps
//                     the tile(s), their circular halos and the 2L + 1 weights in LDS:
//                         [ seg 0: tile + 2L elements | seg 1 | ... | pad to an even scalar | weights ]
//                     Global reads (staging) and writes walk consecutive scalars / elements; LDS reads of consecutive
//                     lanes are consecutive elements, the weight read is a broadcast.  STAGED = false is the same kernel
//                     reading global memory with the modular index, for windows that do not fit the LDS budget.
//
// The tiling and staging maps are in mat_interp_core.h; tests/host_sim/sim_mat_interp.cpp runs them with threads as
// loops.  Built without FMA contraction, as interp.hip.
#include "bdsp_internal.h"
#include "mat_interp_core.h"

namespace bdsp {

static inline unsigned mt_grid(size_t blocks, unsigned per_cu)
{
    size_t cap = (size_t)num_cus() * per_cu;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks ? blocks : 1);
}

// ---------------------------------------------------------------------------------------------
// interpolate_lin / interpolate_hermite of every row
// ---------------------------------------------------------------------------------------------
template <typename T, typename IDX>
__global__ __launch_bounds__(256) void k_mt_interp_lin(const T* __restrict__ in, T* __restrict__ out, IDX rows, IDX len,
                                                        IDX dest_len, T factor, T delay)
{
    const IDX total = rows * dest_len, stride = (IDX)gridDim.x * blockDim.x;
    for (IDX o = (IDX)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += stride) {
        IDX row, n;
        mt_flat_pos<IDX>(o, dest_len, &row, &n);
        out[o] = interp_lin_value<T>(in + row * len, (long long)len, (long long)dest_len, (long long)n, factor, delay);
    }
}

template <typename T, typename IDX>
__global__ __launch_bounds__(256) void k_mt_interp_hermite(const T* __restrict__ in, T* __restrict__ out, IDX rows,
                                                            IDX len, IDX dest_len, T factor, T delay, long long start,
                                                            long long tail)
{
    const IDX total = rows * dest_len, stride = (IDX)gridDim.x * blockDim.x;
    for (IDX o = (IDX)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += stride) {
        IDX row, n;
        mt_flat_pos<IDX>(o, dest_len, &row, &n);
        out[o] = interp_hermite_value<T>(in + row * len, (long long)len, (long long)n, factor, delay, start, tail);
    }
}

template <typename T>
int mt_interpolate_real(const T* in, T* out, size_t rows, size_t len, T factor, T delay, bool hermite, hipStream_t s)
{
    if (rows == 0 || len == 0) return BDSP_OK;
    if (in == out) return BDSP_ERR_UNSUPPORTED;
    const size_t dest_len = interpolate_real_len<T>(len, factor);
    const size_t total = rows * dest_len;
    if (total == 0) return BDSP_OK;
    const dim3 grid(mt_grid((total + 255) / 256, 16)), block(256);
    long long start = 0, tail = 0;
    if (hermite) interp_hermite_regions<T>(dest_len, factor, delay, &start, &tail);
    if (mt_fits_32(rows * len, total)) {
        if (hermite)
            hipLaunchKernelGGL((k_mt_interp_hermite<T, unsigned>), grid, block, 0, s, in, out, (unsigned)rows, (unsigned)len,
                               (unsigned)dest_len, factor, delay, start, tail);
        else
            hipLaunchKernelGGL((k_mt_interp_lin<T, unsigned>), grid, block, 0, s, in, out, (unsigned)rows, (unsigned)len,
                               (unsigned)dest_len, factor, delay);
    } else {
        if (hermite)
            hipLaunchKernelGGL((k_mt_interp_hermite<T, size_t>), grid, block, 0, s, in, out, rows, len, dest_len, factor,
                               delay, start, tail);
        else
            hipLaunchKernelGGL((k_mt_interp_lin<T, size_t>), grid, block, 0, s, in, out, rows, len, dest_len, factor, delay);
    }
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// ---------------------------------------------------------------------------------------------
// direct circular convolution of every row with one weight table
// ---------------------------------------------------------------------------------------------
template <typename T> struct mt_vec2 { typedef T type __attribute__((ext_vector_type(2))); };

// one multiply-add step of output (sre, sim) with element (xr, xi) and weight (w, wi): k_conv_function's expressions
template <typename T, bool CPLX, bool CW>
__device__ __forceinline__ void mt_mac(T& sre, T& sim, T xr, T xi, T w, T wi)
{
    if (CW) { // complex weights (convolve_complex): Complex * Complex, then the sum
        sre = sre + (xr * w - xi * wi);
        sim = sim + (xr * wi + xi * w);
    } else if (CPLX) {
        sre = sre + xr * w;
        sim = sim + xi * w;
    } else {
        sre = sre + xr * w;
    }
}

template <typename T, bool CPLX, bool CW, bool STAGED, int PER>
__global__ __launch_bounds__(256) void k_mt_conv_direct(const T* __restrict__ in, T* __restrict__ out,
                                                         const T* __restrict__ taps, const MtConvGeom g)
{
    static_assert(!CW || CPLX, "complex weights need complex rows");
    static_assert(STAGED || PER == 1, "the unstaged variant computes one output per lane");
    typedef typename mt_vec2<T>::type V2;
    constexpr unsigned E = CPLX ? 2 : 1, WE = CW ? 2 : 1;
    extern __shared__ __align__(16) unsigned char mt_smem[];
    T* xs = reinterpret_cast<T*>(mt_smem);
    T* ws = xs + g.x_scalars;
    const unsigned t = threadIdx.x;
    const unsigned n = (unsigned)g.n, ntaps = 2 * (unsigned)g.l + 1; // STAGED: both below 2^31
    const size_t row_len = (size_t)g.n * E;

    if (STAGED) {
        for (unsigned q = t; q < ntaps * WE; q += MT_WG) ws[q] = taps[q];
    }
    for (unsigned long long vb = blockIdx.x; vb < g.nblocks; vb += gridDim.x) {
        unsigned long long row0;
        unsigned start, cnt;
        mt_conv_block(g, vb, &row0, &start, &cnt);
        const unsigned nseg = mt_conv_segments(g, row0);
        if (STAGED) {
            const unsigned first = mt_conv_first_src(g, start);
            const unsigned span = (cnt + ntaps - 1) * E; // scalars staged per segment
            for (unsigned sg = 0; sg < nseg; ++sg) {
                const T* row = in + (size_t)(row0 + sg) * row_len;
                T* dst = xs + (size_t)sg * g.seg_stride * E;
                for (unsigned q = t; q < span; q += MT_WG) {
                    const unsigned j = CPLX ? q >> 1 : q;
                    dst[q] = row[(size_t)mt_conv_src(first, j, n) * E + (CPLX ? (q & 1) : 0)];
                }
            }
            __syncthreads();
            T sre[PER], sim[PER];
            unsigned at[PER], oi[PER], os[PER];
            bool ok[PER];
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                sre[u] = 0; sim[u] = 0;
                ok[u] = mt_conv_out(g, t + MT_WG * u, nseg, cnt, &os[u], &oi[u]);
                at[u] = ok[u] ? os[u] * g.seg_stride + oi[u] : 0;
            }
            for (unsigned k = 0; k < ntaps; ++k) {
                T w, wi = 0;
                if (CW) { const V2 wv = *reinterpret_cast<const V2*>(ws + 2 * k); w = wv.x; wi = wv.y; }
                else w = ws[k];
#pragma unroll
                for (int u = 0; u < PER; ++u) {
                    if (!ok[u]) continue;
                    if (CPLX) {
                        const V2 xv = *reinterpret_cast<const V2*>(xs + 2 * (size_t)(at[u] + k));
                        mt_mac<T, CPLX, CW>(sre[u], sim[u], xv.x, xv.y, w, wi);
                    } else {
                        mt_mac<T, CPLX, CW>(sre[u], sim[u], xs[at[u] + k], (T)0, w, wi);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                if (!ok[u]) continue;
                T* dst = out + (size_t)(row0 + os[u]) * row_len + (size_t)(start + oi[u]) * E;
                if (CPLX) *reinterpret_cast<V2*>(dst) = V2{sre[u], sim[u]}; // a complex row starts at an even scalar
                else *dst = sre[u];
            }
            __syncthreads(); // the next virtual block restages
        } else {
            unsigned sg, i;
            if (!mt_conv_out(g, t, nseg, cnt, &sg, &i)) continue;
            const long long points = (long long)g.n, L = (long long)g.l;
            const T* row = in + (size_t)(row0 + sg) * row_len;
            const long long o = (long long)start + i;
            long long p = (o - L) % points;
            if (p < 0) p += points;
            T sre = 0, sim = 0;
            for (long long k = 0; k <= 2 * L; ++k) {
                const T w = CW ? taps[2 * k] : taps[k], wi = CW ? taps[2 * k + 1] : (T)0;
                if (CPLX) mt_mac<T, CPLX, CW>(sre, sim, row[2 * p], row[2 * p + 1], w, wi);
                else mt_mac<T, CPLX, CW>(sre, sim, row[p], (T)0, w, wi);
                if (++p == points) p = 0;
            }
            T* dst = out + (size_t)(row0 + sg) * row_len + (size_t)o * E;
            if (CPLX) *reinterpret_cast<V2*>(dst) = V2{sre, sim};
            else *dst = sre;
        }
    }
}

// Staging budget: 64 KB keeps two workgroups resident on a compute unit's 160 KB and stays within what a kernel gets
// without a raised dynamic-LDS limit (kernel_lds); windows above it take the unstaged variant.
constexpr size_t MT_CONV_LDS_BUDGET = 64 * 1024;

template <typename T, bool CPLX, bool CW>
static int mt_conv_launch(const T* in, T* out, const T* taps, const MtConvGeom& g, hipStream_t s)
{
    const dim3 grid(mt_grid((size_t)(g.nblocks < (1ull << 31) ? g.nblocks : (1ull << 31)), 32)), block(MT_WG);
    if (!g.staged)
        hipLaunchKernelGGL((k_mt_conv_direct<T, CPLX, CW, false, 1>), grid, block, 0, s, in, out, taps, g);
    else if (g.per == 4)
        hipLaunchKernelGGL((k_mt_conv_direct<T, CPLX, CW, true, 4>), grid, block, g.lds_bytes, s, in, out, taps, g);
    else
        hipLaunchKernelGGL((k_mt_conv_direct<T, CPLX, CW, true, 1>), grid, block, g.lds_bytes, s, in, out, taps, g);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T>
int mt_conv_direct(const T* in, T* out, size_t rows, size_t points, bool is_complex, const T* taps, size_t conv_len,
                   bool complex_taps, hipStream_t s)
{
    if (rows == 0 || points == 0) return BDSP_OK;
    if (in == out || conv_len > points || (complex_taps && !is_complex)) return BDSP_ERR_UNSUPPORTED;
    const MtConvGeom g = mt_conv_geom(rows, points, conv_len, is_complex ? 2 : 1, complex_taps ? 2 : 1, sizeof(T),
                                      MT_CONV_LDS_BUDGET);
    if (complex_taps) return mt_conv_launch<T, true, true>(in, out, taps, g, s);
    if (is_complex) return mt_conv_launch<T, true, false>(in, out, taps, g, s);
    return mt_conv_launch<T, false, false>(in, out, taps, g, s);
}

#define BDSP_INST(T)                                                                                         \
    template int mt_interpolate_real<T>(const T*, T*, size_t, size_t, T, T, bool, hipStream_t);              \
    template int mt_conv_direct<T>(const T*, T*, size_t, size_t, bool, const T*, size_t, bool, hipStream_t);
BDSP_INST(float)
BDSP_INST(double)
#undef BDSP_INST

} // namespace bdsp
