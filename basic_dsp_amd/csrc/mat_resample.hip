// mat_resample.hip -- FFT-domain resampling and decimation of every row of a matrix (DspMat.interpolatei / interpolate /
// interpft / decimatei).
//
// Replaces the row loop of the reference's matrix crate (matrix/src/time_freq.rs:266-327 forwards InterpolationOps to
// the rows one after the other); each row computes what interpolation.rs:484-633 computes.  The launch counts do not
// depend on the row count.
//
//   k_rs_spectrum_rows  what k_spectrum_resample (elementwise.hip) does for one spectrum, for all rows in one launch:
//                       the general path's step between the batched forward and inverse transforms.  A thread keeps
//                       its destination bin and walks down the rows, so the response and the phase of a bin are
//                       evaluated once per thread, not once per element.
//   k_rs_decimate_rows  out[row][j] = in[row][delay + j * factor], all rows in one launch
//   k_rs_fused          p points -> N = f p points, N a power of two in [16, 4096]: the whole chain in ONE launch.  The
//                       geometry is k_mc_correlate's (mat_correlate.hip): NT = N/16 threads per row with 16 points
//                       each in registers, 256/NT rows per workgroup, data crosses threads through LDS only.  The
//                       zero interleave is a predicate on the load (so the forward N-point transform yields X[k mod p],
//                       the periodic repetition), the multiplier of destination bin k -- mask, response, ratio -- is
//                       applied in registers, the linear phase of a delay in LDS, 1/N rides on the store.  A row is
//                       read once (p points) and written once (N points); real rows are read and written as reals.
#include "bdsp_internal.h"
#include "dsp_funcs.h"

namespace bdsp {

// LDS elements between the regions of adjacent rows of one workgroup (mc_col_stride of mat_correlate.hip)
__host__ __device__ constexpr int rs_col_stride(int n)
{
    const int w = 256 / (n / 16);
    const int base = (n + (n >> 4) + 15) / 16 * 16;
    return base + (w >= 16 ? 1 : 16 / w);
}

// OpFreqResp (elementwise.hip) at bin k of an fft-shifted axis of 2 * maxv (+ 1) points: the same formula in the same
// order, every product rounded on its own
template <typename T>
__device__ __forceinline__ T rs_response(int fid, T rolloff, T ratio, T maxv, size_t k)
{
#pragma clang fp contract(off)
    T j = -maxv + (T)k;
    if (j > (T)0) j = -j;
    return ratio * conv_freq_value<T>(fid, rolloff, fft_swap_x<T>(true, j, maxv) * ratio);
}

// MODE as k_spectrum_resample: 0 periodic repetition, 1 zero_pad(Center) (also dst_points == src_points: a pure delay),
// 2 the crop of interpolate_downsample; fid >= 0 the response on the destination axis, -1 x ratio, -2 nothing.
// Rows: src_points complex apart in `in`, dst_points apart in `out`.  blockDim = (bx, 256 / bx).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_rs_spectrum_rows(const T* __restrict__ in, T* __restrict__ out, size_t rows,
                                                           size_t src_points, size_t dst_points, int fid, T rolloff,
                                                           T ratio, double phase_inc)
{
#pragma clang fp contract(off)
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= dst_points) return;
    const size_t offset = dst_points % 2;
    const T maxv = (T)(dst_points - offset) / (T)2;
    const size_t pos = src_points - src_points / 2, neg = src_points / 2; // bins that stay / move to the end
    const size_t ph_pos = src_points / 2;                                  // OpLinearPhase's positive bins
    size_t sk;
    bool zero = false;
    if (MODE == 0) sk = k % src_points;
    else if (MODE == 2) sk = k < dst_points - dst_points / 2 ? k : k + (src_points - dst_points);
    else {
        if (k < pos) sk = k;
        else if (k >= dst_points - neg) sk = k - (dst_points - src_points);
        else { sk = 0; zero = true; }
    }
    T wr = (T)1, wi = (T)0;
    const bool phase = MODE != 0 && phase_inc != 0.0 && !zero;
    if (phase) { // OpLinearPhase on the source bin
        const double kk = sk < ph_pos ? (double)sk : (double)sk - (double)src_points;
        double sn, cs;
        sincos(phase_inc * kk, &sn, &cs);
        wr = (T)cs;
        wi = (T)sn;
    }
    const T arg = fid >= 0 ? rs_response<T>(fid, rolloff, ratio, maxv, k) : ratio;
    typedef T vec2 __attribute__((ext_vector_type(2)));
    const vec2* in2 = reinterpret_cast<const vec2*>(in);
    vec2* out2 = reinterpret_cast<vec2*>(out);
    const size_t row_step = (size_t)gridDim.y * blockDim.y;
    for (size_t row = (size_t)blockIdx.y * blockDim.y + threadIdx.y; row < rows; row += row_step) {
        T re = (T)0, im = (T)0;
        if (!zero) {
            const vec2 z = in2[row * src_points + sk];
            re = z.x;
            im = z.y;
            if (phase) {
                const T zr = re, zi = im;
                re = zr * wr - zi * wi;
                im = zr * wi + zi * wr;
            }
        }
        if (fid >= 0) {
            const T r2 = re * arg - im * (T)0, i2 = re * (T)0 + im * arg;
            re = r2; im = i2;
        } else if (fid == -1) {
            re = re * ratio; im = im * ratio;
        }
        out2[row * dst_points + k] = vec2{re, im};
    }
}

template <typename P>
__global__ __launch_bounds__(256) void k_rs_decimate_rows(const P* __restrict__ in, P* __restrict__ out, size_t rows,
                                                           size_t points, size_t out_points, size_t factor, size_t delay)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= out_points) return;
    const size_t sj = delay + j * factor; // < points: out_points = ceil((points - delay) / factor)
    const size_t row_step = (size_t)gridDim.y * blockDim.y;
    for (size_t row = (size_t)blockIdx.y * blockDim.y + threadIdx.y; row < rows; row += row_step)
        out[row * out_points + j] = in[row * points + sj];
}

// one thread per column of `cols`, 256 / bx rows per workgroup, enough workgroups down the rows to fill the device
static void rs_row_geometry(size_t rows, size_t cols, dim3* grid, dim3* block)
{
    unsigned bx = 256;
    while (bx > 1 && bx / 2 >= cols) bx /= 2;
    const unsigned by = 256 / bx;
    const size_t gx = (cols + bx - 1) / bx;
    const size_t row_groups = (rows + by - 1) / by;
    size_t gy = ((size_t)num_cus() * 32 + gx - 1) / gx;
    if (gy > row_groups) gy = row_groups;
    if (gy > 65535) gy = 65535;
    if (gy == 0) gy = 1;
    *grid = dim3((unsigned)gx, (unsigned)gy);
    *block = dim3(bx, by);
}

template <typename T>
int rs_spectrum_rows(const T* in, T* out, size_t rows, size_t src_points, size_t dst_points, int mode, int fid, T rolloff,
                     T ratio, double phase_inc, hipStream_t s)
{
    if (rows == 0 || dst_points == 0) return BDSP_OK;
    if (in == out || src_points == 0) return BDSP_ERR_UNSUPPORTED;
    if (mode == 2 ? dst_points > src_points : (mode == 1 && dst_points < src_points)) return BDSP_ERR_ARG_LENGTH;
    if (dst_points > (size_t(1) << 39)) { set_last_error("resample: rows too long for one launch"); return BDSP_ERR_UNSUPPORTED; }
    dim3 grid, block;
    rs_row_geometry(rows, dst_points, &grid, &block);
#define BDSP_RS(M) hipLaunchKernelGGL((k_rs_spectrum_rows<T, M>), grid, block, 0, s, in, out, rows, src_points, dst_points, fid, rolloff, ratio, phase_inc)
    if (mode == 0) BDSP_RS(0);
    else if (mode == 2) BDSP_RS(2);
    else BDSP_RS(1);
#undef BDSP_RS
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T>
int rs_decimate_rows(const T* in, T* out, size_t rows, size_t points, size_t out_points, size_t elem, size_t factor,
                     size_t delay, hipStream_t s)
{
    if (rows == 0 || out_points == 0) return BDSP_OK;
    if (in == out || factor == 0 || delay >= points || delay + (out_points - 1) * factor >= points) return BDSP_ERR_ARG_LENGTH;
    if (out_points > (size_t(1) << 39)) { set_last_error("decimatei: rows too long for one launch"); return BDSP_ERR_UNSUPPORTED; }
    dim3 grid, block;
    rs_row_geometry(rows, out_points, &grid, &block);
    if (elem == 2)
        hipLaunchKernelGGL((k_rs_decimate_rows<cpx<T>>), grid, block, 0, s, reinterpret_cast<const cpx<T>*>(in),
                           reinterpret_cast<cpx<T>*>(out), rows, points, out_points, factor, delay);
    else
        hipLaunchKernelGGL((k_rs_decimate_rows<T>), grid, block, 0, s, in, out, rows, points, out_points, factor, delay);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// mode 0: interpolatei (response on every bin); mode 1: interpolate / interpft (brick-wall mask of the zero_pad(Center),
// response or ratio alone, linear phase on the source bin).  p = N >> lf points per input row, real scalars if is_real.
template <typename T, int N>
__global__ __launch_bounds__(256) void k_rs_fused(const T* __restrict__ in, T* __restrict__ out,
                                                  const cpx<T>* __restrict__ wtab, size_t rows, int lf, int is_real,
                                                  int mode, int fid, T rolloff, T ratio, double phase_inc, T scale)
{
    constexpr int NT = N / 16;
    constexpr int B = 256 / NT; // rows per workgroup
    using F = WgFft<T, N, NT>;
    using P = Radix16Plan<N>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cpx<T>* lds = reinterpret_cast<cpx<T>*>(smem_raw);

    const int tid = threadIdx.x;
    const int c = tid / NT, t = tid % NT;
    const size_t row = (size_t)blockIdx.x * B + c;
    const bool active = row < rows; // inactive threads of the last workgroup transform zeros and keep every barrier
    cpx<T>* l = lds + (size_t)c * rs_col_stride(N);
    auto tw = [&](int m) { return wtab[m]; };
    const int p = N >> lf, fmask = (1 << lf) - 1;

    // zero_interleave(f): point idx of the long row is src[idx / f] where f divides idx, else zero
    const size_t src0 = row * (size_t)p;
    const cpx<T>* srcc = reinterpret_cast<const cpx<T>*>(in);
    cpx<T> v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int idx = t + r * NT;
        const bool ld = active && (idx & fmask) == 0;
        const size_t j = src0 + (size_t)(idx >> lf);
        v[r] = ld ? (is_real ? cpx<T>{in[j], 0} : srcc[j]) : cpx<T>{0, 0};
    }

    constexpr int RL = P::R3 > 1 ? P::R3 : (P::R2 > 1 ? P::R2 : 16);
    constexpr int NSL = N / RL;
    // forward transform: the stages of k_fft_wg
    F::template compute<16, 1, -1>(v, t, tw);
    if constexpr (P::R2 > 1) {
        F::template scatter<16, 1>(v, t, l);
        __syncthreads();
        F::template gather<P::R2>(v, t, l);
        F::template compute<P::R2, 16, -1>(v, t, tw);
    }
    if constexpr (P::R3 > 1) {
        __syncthreads();
        F::template scatter<P::R2, 16>(v, t, l);
        __syncthreads();
        F::template gather<P::R3>(v, t, l);
        F::template compute<P::R3, 16 * P::R2, -1>(v, t, tw);
    }
    // x the multiplier of destination bin k (what k_spectrum_resample applies there), in natural order into LDS: the
    // inverse's input
    const T maxv = (T)(N / 2);
    const int pos = p - p / 2, neg = p / 2;
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int k = F::template out_index<RL, NSL>(t, b, r);
            const T m = fid >= 0 ? rs_response<T>(fid, rolloff, ratio, maxv, (size_t)k) : ratio;
            const bool keep = mode == 0 || k < pos || k >= N - neg;
            l[F::pad(k)] = cscale(keep ? v[b * RL + r] : cpx<T>{0, 0}, m);
        }
    if (mode != 0 && phase_inc != 0.0) {
        // OpLinearPhase on the source bin k mod p: each thread on the elements it has just written, in a loop that stays
        // rolled (one copy of the double-precision sincos)
#pragma unroll 1
        for (int j = 0; j < 16; ++j) {
            const int k = F::template out_index<RL, NSL>(t, j / RL, j % RL);
            const int sk = k & (p - 1);
            const double kk = sk < neg ? (double)sk : (double)sk - (double)p;
            double sn, cs;
            sincos(phase_inc * kk, &sn, &cs);
            l[F::pad(k)] = cmul(l[F::pad(k)], cpx<T>{(T)cs, (T)sn});
        }
    }
    __syncthreads();
    if constexpr (N >= 256) F::template gather<16>(v, t, l);
    else {
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = l[F::pad(F::template in_index<16>(t, 0, r))];
    }
    // inverse transform
    F::template compute<16, 1, 1>(v, t, tw);
    if constexpr (P::R2 > 1) {
        __syncthreads();
        F::template scatter<16, 1>(v, t, l);
        __syncthreads();
        F::template gather<P::R2>(v, t, l);
        F::template compute<P::R2, 16, 1>(v, t, tw);
    }
    if constexpr (P::R3 > 1) {
        __syncthreads();
        F::template scatter<P::R2, 16>(v, t, l);
        __syncthreads();
        F::template gather<P::R3>(v, t, l);
        F::template compute<P::R3, 16 * P::R2, 1>(v, t, tw);
    }
    if (!active) return;
    // 1/N; a real row keeps the real parts only
    const size_t dst0 = row * (size_t)N;
    cpx<T>* dstc = reinterpret_cast<cpx<T>*>(out);
#pragma unroll
    for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const size_t k = dst0 + (size_t)F::template out_index<RL, NSL>(t, b, r);
            if (is_real) out[k] = v[b * RL + r].x * scale;
            else dstc[k] = cscale(v[b * RL + r], scale);
        }
}

// an integer factor >= 2 into a power of two in [16, 4096] (so the factor and the row length are powers of two as well)
bool rs_fused_applies(size_t points, size_t new_points)
{
    return new_points >= 16 && new_points <= 4096 && (new_points & (new_points - 1)) == 0 && points >= 1 &&
           points < new_points && new_points % points == 0;
}

template <typename T, int N>
static int rs_launch(const T* in, T* out, size_t rows, size_t p, bool is_real, int mode, int fid, T rolloff, T ratio,
                     double phase_inc, hipStream_t s)
{
    const cpx<T>* wtab;
    BDSP_TRY(twiddle_table<T>(N, &wtab));
    constexpr int B = 256 / (N / 16);
    const size_t lds = (size_t)B * rs_col_stride(N) * sizeof(cpx<T>);
    const size_t groups = (rows + B - 1) / B;
    if (groups > 0x7fffffffu) { set_last_error("resample: too many rows for one launch"); return BDSP_ERR_UNSUPPORTED; }
    BDSP_TRY(kernel_lds(k_rs_fused<T, N>, lds));
    int lf = 0;
    while ((p << lf) < (size_t)N) ++lf;
    hipLaunchKernelGGL((k_rs_fused<T, N>), dim3((unsigned)groups), dim3(256), lds, s, in, out, wtab, rows, lf,
                       is_real ? 1 : 0, mode, fid, rolloff, ratio, phase_inc, (T)1 / (T)N);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T>
int rs_fused(const T* in, T* out, size_t rows, size_t points, size_t new_points, bool is_real, int mode, int fid,
             T rolloff, T ratio, double phase_inc, hipStream_t s)
{
    if (!rs_fused_applies(points, new_points) || in == out) { set_last_error("resample: no fused kernel for these lengths"); return BDSP_ERR_UNSUPPORTED; }
    if (rows == 0) return BDSP_OK;
    switch (new_points) {
#define BDSP_RS(NV) case NV: return rs_launch<T, NV>(in, out, rows, points, is_real, mode, fid, rolloff, ratio, phase_inc, s)
        BDSP_RS(16); BDSP_RS(32); BDSP_RS(64); BDSP_RS(128); BDSP_RS(256); BDSP_RS(512); BDSP_RS(1024); BDSP_RS(2048);
        BDSP_RS(4096);
#undef BDSP_RS
    }
    return BDSP_ERR_UNSUPPORTED;
}

#define BDSP_INST(T)                                                                                                    \
    template int rs_spectrum_rows<T>(const T*, T*, size_t, size_t, size_t, int, int, T, T, double, hipStream_t);        \
    template int rs_decimate_rows<T>(const T*, T*, size_t, size_t, size_t, size_t, size_t, size_t, hipStream_t);        \
    template int rs_fused<T>(const T*, T*, size_t, size_t, size_t, bool, int, int, T, T, double, hipStream_t);
BDSP_INST(float)
BDSP_INST(double)
#undef BDSP_INST

} // namespace bdsp
