// zoom_fft.hip -- chirp-z transform of a frequency band of every row of a matrix (a vector is one row):
//     X[r][k] = sum_{n<N} x[r][n] exp(-2 pi i (start_r + k step) n),      k < bins
// with a free start (one for all rows, or one per row), step and output count; nothing of it is in the reference.  The
// algebra, the phase reduction and the per-thread maps are in zoom_fft_core.h.
//
//   k_zf_tables   the three chirp tables of a plan (pre, post, wrapped kernel) in one launch; every phase is reduced
//                 exactly and evaluated by sincospi in double (the kernel's spectrum is then one power-of-two transform)
//   k_zf_wg       L in {512, 1024, 2048, 4096}: the whole transform of every row in ONE launch, k_bluestein_wg's geometry
//                 (L/16 threads per row, 16 points in registers, 256/(L/16) rows per workgroup, persistent over the rows,
//                 the spectrum stays in registers between the two transforms); rows of N points in, rows of `bins`
//                 points out, real rows read as (x, 0), and with per-row starts the load applies the row's own phase ramp
//   k_zf_pre      larger L: chirp, zero fill to L, real input and the per-row start in one launch over all rows ...
//   k_zf_post     ... and post-chirp and crop to `bins` in another, around the batched transforms; both walk a flat index
//                 in a grid-stride loop, so the launch count does not depend on the row count
#include "bdsp_internal.h"
#include "zoom_fft_core.h"
#include <type_traits>

namespace bdsp {

template <typename T>
__global__ __launch_bounds__(256) void k_zf_tables(cpx<T>* __restrict__ pre, cpx<T>* __restrict__ post,
                                                   cpx<T>* __restrict__ kern, unsigned long long n,
                                                   unsigned long long bins, unsigned long long l, double start, double step)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) pre[i] = zf_pre_value<T>(start, step, i);
    if (i < bins) post[i] = zf_post_value<T>(step, i);
    if (i < l) kern[i] = zf_kern_value<T>(step, i, n, bins, l);
}

template <typename T, int L, bool IN_REAL, bool ROW_START>
__global__ __launch_bounds__(256) void k_zf_wg(const T* __restrict__ x, cpx<T>* __restrict__ y,
                                               const cpx<T>* __restrict__ pre, const cpx<T>* __restrict__ post,
                                               const cpx<T>* __restrict__ kspec, const cpx<T>* __restrict__ wtab,
                                               const double* __restrict__ starts, unsigned n, unsigned bins, size_t rows)
{
    using G = ZfGeom<L>;
    constexpr int NT = G::NT, B = G::B, R3 = G::R3;
    using F = WgFft<T, L, NT>;
    using XE = typename std::conditional<IN_REAL, T, cpx<T>>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, col = tid / NT, t = tid % NT;
    cpx<T>* l = reinterpret_cast<cpx<T>*>(smem_raw) + (size_t)col * (F::LDS_ELEMS + 1);
    cpx<T>* tw2l = reinterpret_cast<cpx<T>*>(smem_raw) + (size_t)B * (F::LDS_ELEMS + 1);
    auto tw = [&](int mm) { return wtab[mm]; };
    // persistent over the rows: last-stage twiddles in registers, second-stage twiddles in an LDS table
    cpx<T> tw3[G::NTW3];
    F::template load_twiddles<R3, 256>(tw3, t, tw);
    if (tid < 240) {
        int k = tid / 15, r = tid % 15 + 1;
        tw2l[k * 17 + r - 1] = wtab[r * k * (L / 256)];
    }
    __syncthreads();
    const cpx<T>* tw2p = tw2l + (t & 15) * 17;

    cpx<T> v[16];
    auto fft3 = [&](auto dir) {
        constexpr int DIR = decltype(dir)::value;
        F::template compute<16, 1, DIR>(v, t, tw);
        __syncthreads(); // the previous exchange's gather is done
        F::template scatter<16, 1>(v, t, l);
        __syncthreads();
        F::template gather<16>(v, t, l);
        F::template compute_pre<16, 16, DIR>(v, tw2p);
        __syncthreads();
        F::template scatter<16, 16>(v, t, l);
        __syncthreads();
        F::template gather<R3>(v, t, l);
        F::template compute_pre<R3, 256, DIR>(v, tw3);
    };
    const size_t groups = (rows + B - 1) / B;
    for (size_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        const size_t row = gi * B + col;
        const bool active = row < rows; // inactive columns of the last group transform zeros and keep every barrier
        const XE* xv = reinterpret_cast<const XE*>(x) + (active ? row * (size_t)n : 0);
        double start_r = 0.0;
        if (ROW_START && active) start_r = starts[row];
        zf_load<T, L, IN_REAL, ROW_START>(v, t, active, xv, pre, n, start_r);
        fft3(std::integral_constant<int, -1>{});
        zf_spectrum_mul<T, L>(v, t, kspec);
        fft3(std::integral_constant<int, 1>{});
        if (active) zf_store<T, L>(v, t, y + row * (size_t)bins, post, bins);
    }
}

template <typename T, bool IN_REAL, bool ROW_START>
__global__ __launch_bounds__(256) void k_zf_pre(const T* __restrict__ x, cpx<T>* __restrict__ a,
                                                const cpx<T>* __restrict__ pre, const double* __restrict__ starts,
                                                unsigned long long n, unsigned long long l, unsigned long long total)
{
    using XE = typename std::conditional<IN_REAL, T, cpx<T>>::type;
    const XE* xe = reinterpret_cast<const XE*>(x);
    const unsigned long long step = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step)
        a[i] = zf_pre_point<T, IN_REAL, ROW_START>(xe, pre, starts, i, n, l);
}

template <typename T>
__global__ __launch_bounds__(256) void k_zf_post(const cpx<T>* __restrict__ conv, cpx<T>* __restrict__ out,
                                                 const cpx<T>* __restrict__ post, unsigned long long bins,
                                                 unsigned long long l, unsigned long long total)
{
    const unsigned long long step = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step)
        out[i] = zf_post_point<T>(conv, post, i, bins, l);
}

static inline unsigned zf_grid(size_t items)
{
    size_t g = (items + 255) / 256, cap = (size_t)num_cus() * 16;
    return (unsigned)(g < cap ? (g ? g : 1) : cap);
}

template <typename T>
int zf_tables(T* pre, T* post, T* kern, size_t n, size_t bins, size_t l, double start, double step, hipStream_t s)
{
    hipLaunchKernelGGL((k_zf_tables<T>), dim3((unsigned)((l + 255) / 256)), dim3(256), 0, s, reinterpret_cast<cpx<T>*>(pre),
                       reinterpret_cast<cpx<T>*>(post), reinterpret_cast<cpx<T>*>(kern), (unsigned long long)n,
                       (unsigned long long)bins, (unsigned long long)l, start, step);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, int L, bool IN_REAL, bool ROW_START>
static int zf_launch_wg(const T* x, T* y, const T* pre, const T* post, const T* kspec, const double* starts, size_t n,
                        size_t bins, size_t rows, hipStream_t s)
{
    const cpx<T>* wtab;
    BDSP_TRY(twiddle_table<T>(L, &wtab));
    constexpr int B = ZfGeom<L>::B;
    using F = WgFft<T, L, L / 16>;
    const size_t lds = ((size_t)B * (F::LDS_ELEMS + 1) + 16 * 17) * sizeof(cpx<T>);
    auto k = k_zf_wg<T, L, IN_REAL, ROW_START>;
    BDSP_TRY(kernel_lds(k, lds));
    const size_t groups = (rows + B - 1) / B, slots = (size_t)num_cus() * 4;
    hipLaunchKernelGGL(k, dim3((unsigned)(groups < slots ? groups : slots)), dim3(256), lds, s, x, reinterpret_cast<cpx<T>*>(y),
                       reinterpret_cast<const cpx<T>*>(pre), reinterpret_cast<const cpx<T>*>(post),
                       reinterpret_cast<const cpx<T>*>(kspec), wtab, starts, (unsigned)n, (unsigned)bins, rows);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, int L>
static int zf_launch_wg_kind(const T* x, T* y, const T* pre, const T* post, const T* kspec, const double* starts, size_t n,
                             size_t bins, size_t rows, bool in_real, hipStream_t s)
{
    if (in_real)
        return starts ? zf_launch_wg<T, L, true, true>(x, y, pre, post, kspec, starts, n, bins, rows, s)
                      : zf_launch_wg<T, L, true, false>(x, y, pre, post, kspec, starts, n, bins, rows, s);
    return starts ? zf_launch_wg<T, L, false, true>(x, y, pre, post, kspec, starts, n, bins, rows, s)
                  : zf_launch_wg<T, L, false, false>(x, y, pre, post, kspec, starts, n, bins, rows, s);
}

// rows x n points (real scalars if in_real, else complex) at x -> rows x bins complex at y (must not overlap x), for
// l = zf_conv_len(n, bins) in {512, 1024, 2048, 4096}; starts: null, or one start per row (device, reduced modulo 1)
template <typename T>
int zf_fused(const T* x, T* y, const T* pre, const T* post, const T* kspec, const double* starts, size_t n, size_t bins,
             size_t l, size_t rows, bool in_real, hipStream_t s)
{
    if (rows == 0) return BDSP_OK;
    if (n + bins - 1 > l) return BDSP_ERR_ARG_LENGTH;
    switch (l) {
    case 512: return zf_launch_wg_kind<T, 512>(x, y, pre, post, kspec, starts, n, bins, rows, in_real, s);
    case 1024: return zf_launch_wg_kind<T, 1024>(x, y, pre, post, kspec, starts, n, bins, rows, in_real, s);
    case 2048: return zf_launch_wg_kind<T, 2048>(x, y, pre, post, kspec, starts, n, bins, rows, in_real, s);
    case 4096: return zf_launch_wg_kind<T, 4096>(x, y, pre, post, kspec, starts, n, bins, rows, in_real, s);
    default: return BDSP_ERR_UNSUPPORTED;
    }
}

// rows x n points at x -> rows x l complex at a: chirped, zero filled
template <typename T>
int zf_pre(const T* x, T* a, const T* pre, const double* starts, size_t n, size_t l, size_t rows, bool in_real, hipStream_t s)
{
    const size_t total = rows * l;
    if (total == 0) return BDSP_OK;
    const dim3 grid(zf_grid(total));
#define BDSP_ZF_PRE(R, S)                                                                                              \
    hipLaunchKernelGGL((k_zf_pre<T, R, S>), grid, dim3(256), 0, s, x, reinterpret_cast<cpx<T>*>(a),                    \
                       reinterpret_cast<const cpx<T>*>(pre), starts, (unsigned long long)n, (unsigned long long)l,     \
                       (unsigned long long)total)
    if (in_real) { if (starts) BDSP_ZF_PRE(true, true); else BDSP_ZF_PRE(true, false); }
    else { if (starts) BDSP_ZF_PRE(false, true); else BDSP_ZF_PRE(false, false); }
#undef BDSP_ZF_PRE
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// rows x l complex at conv -> rows x bins complex at out: post-chirp and crop
template <typename T>
int zf_post(const T* conv, T* out, const T* post, size_t bins, size_t l, size_t rows, hipStream_t s)
{
    const size_t total = rows * bins;
    if (total == 0) return BDSP_OK;
    hipLaunchKernelGGL((k_zf_post<T>), dim3(zf_grid(total)), dim3(256), 0, s, reinterpret_cast<const cpx<T>*>(conv),
                       reinterpret_cast<cpx<T>*>(out), reinterpret_cast<const cpx<T>*>(post), (unsigned long long)bins,
                       (unsigned long long)l, (unsigned long long)total);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

#define BDSP_INST(T)                                                                                                       \
    template int zf_tables<T>(T*, T*, T*, size_t, size_t, size_t, double, double, hipStream_t);                            \
    template int zf_fused<T>(const T*, T*, const T*, const T*, const T*, const double*, size_t, size_t, size_t, size_t,    \
                             bool, hipStream_t);                                                                           \
    template int zf_pre<T>(const T*, T*, const T*, const double*, size_t, size_t, size_t, bool, hipStream_t);              \
    template int zf_post<T>(const T*, T*, const T*, size_t, size_t, size_t, hipStream_t);
BDSP_INST(float)
BDSP_INST(double)
#undef BDSP_INST

} // namespace bdsp
