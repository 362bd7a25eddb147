// mat_correlate.hip -- cross-correlation of every row of a matrix with a prepared argument (DspMat.correlate).
//
// Replaces the row loop of the reference's matrix crate (matrix/src/time_freq.rs:208-264 forwards
// CrossCorrelationArgumentOps / CrossCorrelationOps to the rows one after the other); each row computes what
// correlation.rs:96-160 computes: zero_pad(L, Surround) -> plain_fft -> x argument -> plain_ifft -> 1/L -> swap_halves.
//
//   k_mc_pad_rows   all rows of a matrix Surround-padded from p to L points in one launch (prepare_argument_padded and
//                   the general path; real or complex rows)
//   k_mc_correlate  L = N a power of two, 16 <= N <= 4096: the whole chain in ONE launch.  The geometry is k_fft_wg's
//                   (fft_impl.h): NT = N/16 threads per row with 16 points each in registers, 256/NT rows per
//                   workgroup, data crosses threads through LDS only.  A row is read once (p points) and written once
//                   (L points); the padding is a predicate on the load, the argument multiplies the spectrum in
//                   registers, 1/L and swap_halves ride on the store.
#include "bdsp_internal.h"

namespace bdsp {

// LDS elements between the regions of adjacent rows of one workgroup: col_stride(n) of fft_impl.h (the padded length
// rounded up to 16, plus an odd-ish offset that spreads the rows of a 16-lane group over all banks)
__host__ __device__ constexpr int mc_col_stride(int n)
{
    const int w = 256 / (n / 16);
    const int base = (n + (n >> 4) + 15) / 16 * 16;
    return base + (w >= 16 ? 1 : 16 / w);
}

template <typename E>
__global__ __launch_bounds__(256) void k_mc_pad_rows(const E* __restrict__ in, E* __restrict__ out, size_t rows, size_t p,
                                                     size_t l, size_t d0)
{
    const size_t total = rows * l, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const size_t row = i / l, idx = i - row * l;
        const bool inside = idx >= d0 && idx - d0 < p;
        out[i] = inside ? in[row * p + (idx - d0)] : E{};
    }
}

template <typename T, int N>
__global__ __launch_bounds__(256) void k_mc_correlate(const cpx<T>* __restrict__ in, cpx<T>* __restrict__ out,
                                                      const cpx<T>* __restrict__ arg, const cpx<T>* __restrict__ wtab,
                                                      size_t rows, int p, int d0, size_t arg_stride, T scale)
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
    cpx<T>* l = lds + (size_t)c * mc_col_stride(N);
    auto tw = [&](int m) { return wtab[m]; };

    // zero_pad(N, Surround): point idx of the padded row is in[idx - d0] for 0 <= idx - d0 < p
    const cpx<T>* src = in + row * (size_t)p;
    cpx<T> v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = t + r * NT - d0;
        v[r] = (active && k >= 0 && k < p) ? src[k] : cpx<T>{0, 0};
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
    // x argument (prepared = already conjugated), in natural order into LDS: the inverse's input
    const cpx<T>* a = arg + (active ? row * arg_stride : 0);
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int k = F::template out_index<RL, NSL>(t, b, r);
            l[F::pad(k)] = cmul(v[b * RL + r], a[k]);
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
    // 1/L, and swap_halves: the last stage's digit r is the top digit of the output index, (k + N/2) mod N flips its top bit
    cpx<T>* dst = out + row * (size_t)N;
#pragma unroll
    for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
        for (int r = 0; r < RL; ++r)
            dst[F::template out_index<RL, NSL>(t, b, r ^ (RL / 2))] = cscale(v[b * RL + r], scale);
}

template <typename T>
int mc_pad_rows(const T* in, T* out, size_t rows, size_t p, size_t l, bool is_complex, hipStream_t s)
{
    if (rows == 0 || l == 0) return BDSP_OK;
    if (l < p) return BDSP_ERR_ARG_LENGTH;
    const size_t d0 = (l - p) - (l - p) / 2; // zero_pad, option Surround (mat_frame_core.h, mf_pad_geom)
    const size_t total = rows * l, want = (total + 255) / 256, cap = (size_t)num_cus() * 32;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    if (is_complex)
        hipLaunchKernelGGL((k_mc_pad_rows<cpx<T>>), dim3(grid), dim3(256), 0, s, reinterpret_cast<const cpx<T>*>(in),
                           reinterpret_cast<cpx<T>*>(out), rows, p, l, d0);
    else
        hipLaunchKernelGGL((k_mc_pad_rows<T>), dim3(grid), dim3(256), 0, s, in, out, rows, p, l, d0);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

bool mc_fused_len(size_t l) { return l >= 16 && l <= 4096 && (l & (l - 1)) == 0; }

template <typename T, int N>
static int mc_launch(const T* in, T* out, const T* arg, size_t arg_stride, size_t rows, size_t p, hipStream_t s)
{
    const cpx<T>* wtab;
    BDSP_TRY(twiddle_table<T>(N, &wtab));
    constexpr int B = 256 / (N / 16);
    const size_t lds = (size_t)B * mc_col_stride(N) * sizeof(cpx<T>);
    const size_t groups = (rows + B - 1) / B;
    if (groups > 0x7fffffffu) { set_last_error("correlate: too many rows for one launch"); return BDSP_ERR_UNSUPPORTED; }
    BDSP_TRY(kernel_lds(k_mc_correlate<T, N>, lds));
    const int d0 = (int)((N - p) - (N - p) / 2);
    hipLaunchKernelGGL((k_mc_correlate<T, N>), dim3((unsigned)groups), dim3(256), lds, s,
                       reinterpret_cast<const cpx<T>*>(in), reinterpret_cast<cpx<T>*>(out),
                       reinterpret_cast<const cpx<T>*>(arg), wtab, rows, (int)p, d0, arg_stride, (T)1 / (T)N);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T>
int mc_correlate_fused(const T* in, T* out, const T* arg, size_t arg_stride, size_t rows, size_t p, size_t l, hipStream_t s)
{
    if (!mc_fused_len(l) || p >= l) { set_last_error("correlate: no fused kernel for this length"); return BDSP_ERR_UNSUPPORTED; }
    if (rows == 0) return BDSP_OK;
    switch (l) {
#define BDSP_MC(NV) case NV: return mc_launch<T, NV>(in, out, arg, arg_stride, rows, p, s)
        BDSP_MC(16); BDSP_MC(32); BDSP_MC(64); BDSP_MC(128); BDSP_MC(256); BDSP_MC(512); BDSP_MC(1024); BDSP_MC(2048);
        BDSP_MC(4096);
#undef BDSP_MC
    }
    return BDSP_ERR_UNSUPPORTED;
}

#define BDSP_INST(T)                                                                                                    \
    template int mc_pad_rows<T>(const T*, T*, size_t, size_t, size_t, bool, hipStream_t);                               \
    template int mc_correlate_fused<T>(const T*, T*, const T*, size_t, size_t, size_t, size_t, hipStream_t);
BDSP_INST(float)
BDSP_INST(double)
#undef BDSP_INST

} // namespace bdsp
