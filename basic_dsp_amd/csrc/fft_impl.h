// fft_impl.h -- (included by fft_f32.hip / fft_f64.hip with BDSP_FFT_T set) unnormalised complex FFT kernels for gfx950 (f32 and f64).
//
// Replaces, for the hot path: rustfft behind fft() (vector/src/vector_types/time_freq/mod.rs:32-63)
// and clFFT behind GpuSupport::fft (vector/src/gpu_support/ocl/mod.rs:301-357).
//
// Power-of-two lengths:
//   n <= 8            one thread per transform (k_fft_tiny)
//   16 <= n <= 4096   one workgroup-resident Stockham FFT, 16 points per thread, data crosses
//                     threads through LDS only (k_fft_wg); several small transforms per workgroup
//   n > 4096          2 or 3 global Stockham passes of super-radix RP in {64..1024} (k_fft_pass):
//                     each workgroup takes a tile of W = 4096/RP adjacent columns, so every global
//                     access is a run of W contiguous points (RP = 256: 128-byte segments), does the
//                     RP-point sub-FFT for all W columns in registers + LDS, applies the inter-pass
//                     twiddle on load and writes the autosorted result.  2^24 points = 3 passes.
// Every other length goes through Bluestein's chirp-z on the same kernels (fft_any).
// Window, 1/N scale, fft_shift / ifft_shift and magnitude are fused into the first / last pass
// (FftIo), so fft()/windowed_fft()/ifft() never take an extra trip through HBM
// (reference: time_to_freq.rs:158-175, freq_to_time.rs:160-177 run them as separate passes).
#include <cstdlib>
#include <type_traits>

#include "bdsp_internal.h"
#include "dsp_funcs.h"

// BDSP_FFT_PART (round 6).  A process's first transform loads the code object of the translation unit its first kernel lives
// in (HIP loads per unit: *measured*, tools/first_call_probe.py -- 4.2 ms for the 2.7 MB of all f32 kernels), and two thirds
// of that code serves fused options and generic I/O that a plain transform never launches.  So each precision is TWO units:
//   1  "plain" (fft_f32.hip / fft_f64.hip): plan selection, fft_pow2, and every kernel a plain transform can launch -- the
//      SIMPLE pass instantiations, k_fft_wg without generic I/O, k_fft_wg_batch, k_fft_wg4, k_fft_tiny;
//   2  "options" (fft_f32_opts.hip / fft_f64_opts.hip): the pass kernels with fused shift / scale / window / real input /
//      magnitude / real-part output and the generic-I/O (GEN) kernels, reached through launch_pass_opts_rp / launch_wg_gen.
//   0  everything in one unit.
#ifndef BDSP_FFT_PART
#define BDSP_FFT_PART 0
#endif

namespace bdsp {

template <typename T>
int launch_pass_opts_rp(const FftPassRoute& r, const FftIo<T>& io, const cpx<T>* src, cpx<T>* dst, size_t n, size_t nsg, size_t batch,
                        hipStream_t s);
template <typename T>
int launch_wg_gen(int n, const FftIo<T>& io, size_t batch, bool inverse, hipStream_t s);

// ------------------------------------------------------------------------------ fused I/O
template <typename T>
__device__ __forceinline__ T dev_hypot(T a, T b);
template <> __device__ __forceinline__ float dev_hypot<float>(float a, float b) { return hypotf(a, b); }
template <> __device__ __forceinline__ double dev_hypot<double>(double a, double b) { return hypot(a, b); }

template <typename T>
__device__ __forceinline__ cpx<T> io_load(const FftIo<T>& io, size_t vec, size_t i)
{
    size_t src = i;
    if (io.flags & BDSP_FFT_SHIFT_IN) { // ifft_shift: out[i] = in[(i + floor(n/2)) mod n]
        src = i + io.n / 2;
        if (src >= io.n) src -= io.n;
    }
    cpx<T> v;
    if (io.in_valid && src >= io.in_valid) return cpx<T>{0, 0};
    if (io.flags & FFT_IN_REAL) {
        v.x = reinterpret_cast<const T*>(io.in)[vec * io.in_stride + src];
        v.y = (T)0;
    } else {
        v = reinterpret_cast<const cpx<T>*>(io.in)[vec * io.in_stride + src];
    }
    if (io.window_id >= 0 && !(io.flags & FFT_WINDOW_OUT_DIV)) {
        T w = window_value_sym<T>(io.window_id, io.window_alpha, src, io.n);
        v.x = v.x * w;
        v.y = v.y * w;
    }
    if (io.in_scale != (T)1) {
        v.x = v.x * io.in_scale;
        v.y = v.y * io.in_scale;
    }
    return v;
}

template <typename T>
__device__ __forceinline__ void io_store(const FftIo<T>& io, size_t vec, size_t k, cpx<T> v)
{
    size_t dst = k;
    if (io.flags & BDSP_FFT_SHIFT_OUT) { // fft_shift: out[i] = in[(i + ceil(n/2)) mod n]
        dst = k + io.n / 2;
        if (dst >= io.n) dst -= io.n;
    }
    if (io.flags & FFT_WINDOW_OUT_DIV) {
        T w = (T)1 / window_value_sym<T>(io.window_id, io.window_alpha, dst, io.n);
        v.x = v.x * w;
        v.y = v.y * w;
    }
    if (io.flags & BDSP_FFT_MAGNITUDE)
        reinterpret_cast<T*>(io.out)[vec * io.out_stride + dst] = dev_hypot<T>(v.x, v.y);
    else if (io.flags & FFT_OUT_REAL)
        reinterpret_cast<T*>(io.out)[vec * io.out_stride + dst] = v.x;
    else
        reinterpret_cast<cpx<T>*>(io.out)[vec * io.out_stride + dst] = v;
}

// (col_stride, pass_split_exchange, pass_tile_lds_bytes, pass_min_waves, pass_lds_twiddles: fft_plan_core.h)

// ------------------------------------------------------------------------------ n <= 8
template <typename T, int N, int DIR>
__global__ __launch_bounds__(256) void k_fft_tiny(FftIo<T> io, size_t batch)
{
    size_t vec = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec >= batch) return;
    cpx<T> v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = io_load(io, vec, i);
    dft<N, DIR>(v);
#pragma unroll
    for (int i = 0; i < N; ++i) io_store(io, vec, i, v[i]);
}

// ------------------------------------------------------------------------------ 16 <= n <= 4096
// GEN = false: plain complex in/out, registers <-> global directly.
// GEN = true : any fused option (window, scale, shifts, real input, magnitude ...).  The option
// code runs in a ROLLED loop that stages through LDS, so the register array stays statically
// indexed and the option code is emitted once instead of 16 times per thread.
template <typename T, int N, int DIR, bool GEN>
__global__ __launch_bounds__(256) void k_fft_wg(FftIo<T> io, const cpx<T>* __restrict__ wtab,
                                                 size_t batch)
{
    constexpr int NT = N / 16;
    constexpr int B = 256 / NT; // transforms per workgroup
    using F = WgFft<T, N, NT>;
    using P = Radix16Plan<N>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cpx<T>* lds = reinterpret_cast<cpx<T>*>(smem_raw);

    const int tid = threadIdx.x;
    const int c = tid / NT, t = tid % NT;
    const size_t vec = (size_t)blockIdx.x * B + c;
    const bool active = vec < batch;
    cpx<T>* l = lds + (size_t)c * col_stride(N);
    auto tw = [&](int m) { return wtab[m]; };

    cpx<T> v[16];
    if constexpr (GEN) {
#pragma unroll 2
        for (int e = 0; e < 16; ++e) {
            int idx = t + e * NT;
            l[F::pad(idx)] = active ? io_load(io, vec, (size_t)idx) : cpx<T>{0, 0};
        }
        __syncthreads();
        if constexpr (N >= 256) F::template gather<16>(v, t, l);
        else {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = l[F::pad(F::template in_index<16>(t, 0, r))];
        }
        __syncthreads();
    } else {
        const cpx<T>* in = reinterpret_cast<const cpx<T>*>(io.in) + vec * io.in_stride;
        const int nvalid = io.in_valid ? (int)io.in_valid : N;
        // ifft_shift of the input (even n): in[(i + n/2) mod n] with i = t + r*NT is register r ^ 8's address
        const int rx = (io.flags & BDSP_FFT_SHIFT_IN) ? 8 : 0;
        if (io.flags & FFT_IN_REAL) {
            const T* inr = reinterpret_cast<const T*>(io.in) + vec * io.in_stride;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int idx = F::template in_index<16>(t, 0, r ^ rx);
                v[r] = cpx<T>{(active && idx < nvalid) ? inr[idx] : (T)0, (T)0};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int idx = F::template in_index<16>(t, 0, r ^ rx);
                v[r] = (active && idx < nvalid) ? in[idx] : cpx<T>{0, 0};
            }
        }
        if (io.in_scale != (T)1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = cpx<T>{v[r].x * io.in_scale, v[r].y * io.in_scale};
        }
    }
    F::template compute<16, 1, DIR>(v, t, tw);
    if constexpr (P::R2 > 1) {
        F::template scatter<16, 1>(v, t, l);
        __syncthreads();
        F::template gather<P::R2>(v, t, l);
        F::template compute<P::R2, 16, DIR>(v, t, tw);
    }
    if constexpr (P::R3 > 1) {
        __syncthreads();
        F::template scatter<P::R2, 16>(v, t, l);
        __syncthreads();
        F::template gather<P::R3>(v, t, l);
        F::template compute<P::R3, 16 * P::R2, DIR>(v, t, tw);
    }
    constexpr int RL = P::R3 > 1 ? P::R3 : (P::R2 > 1 ? P::R2 : 16);
    constexpr int NSL = N / RL;
    if constexpr (GEN) {
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
            for (int r = 0; r < RL; ++r) l[F::pad(F::template out_index<RL, NSL>(t, b, r))] = v[b * RL + r];
        __syncthreads();
        if (!active) return;
#pragma unroll 1
        for (int e = 0; e < 16; ++e) {
            int idx = t + e * NT;
            io_store(io, vec, (size_t)idx, l[F::pad(idx)]);
        }
    } else {
        if (!active) return;
        cpx<T>* out = reinterpret_cast<cpx<T>*>(io.out) + vec * io.out_stride;
        // fft_shift of the output (even n): the last stage's digit r is the top digit of the output index
        const int sx = (io.flags & BDSP_FFT_SHIFT_OUT) ? RL / 2 : 0;
        if (io.flags & (BDSP_FFT_MAGNITUDE | FFT_OUT_REAL)) {
            T* outr = reinterpret_cast<T*>(io.out) + vec * io.out_stride;
            const bool mag = (io.flags & BDSP_FFT_MAGNITUDE) != 0;
#pragma unroll
            for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
                for (int r = 0; r < RL; ++r) {
                    const cpx<T> z = v[b * RL + r];
                    outr[F::template out_index<RL, NSL>(t, b, r ^ sx)] = mag ? dev_hypot<T>(z.x, z.y) : z.x;
                }
            return;
        }
#pragma unroll
        for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
            for (int r = 0; r < RL; ++r) out[F::template out_index<RL, NSL>(t, b, r ^ sx)] = v[b * RL + r];
    }
}

// Persistent batched variant of k_fft_wg for N in {1024, 2048, 4096}, plain I/O, large batches: a
// workgroup walks the batch with a grid stride, keeps the last stage's twiddles in registers and the
// 16 x 15 second-stage twiddles in an LDS table (k_fft_wg re-reads both from L2 for every transform,
// twice in its dependency chain), and uses the conflict-free exchange layouts for N = 4096.
// *Measured* (16M points in all): 4096 x 4096: 75.9 -> 53.2 us, 2048 x 8192: 66.9 -> 54.4 us,
// 1024 x 16384: 62.7 -> 54.0 us (5.0 TB/s algorithmic).
template <typename T, int N, int DIR>
__global__ __launch_bounds__(256) void k_fft_wg_batch(FftIo<T> io, const cpx<T>* __restrict__ wtab, size_t batch)
{
    constexpr int NT = N / 16;
    constexpr int B = 256 / NT;
    using F = WgFft<T, N, NT>;
    using P = Radix16Plan<N>;
    static_assert(P::R2 == 16 && P::R3 >= 4, "1024 <= N <= 4096");
    constexpr int R3 = P::R3, NTW3 = (16 / R3) * (R3 - 1);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cpx<T>* lds = reinterpret_cast<cpx<T>*>(smem_raw);
    const int tid = threadIdx.x;
    const int c = tid / NT, t = tid % NT;
    cpx<T>* l = lds + (size_t)c * col_stride(N);
    cpx<T>* tw2l = lds + (size_t)B * col_stride(N);
    auto tw = [&](int m) { return wtab[m]; };

    // R3 = 16 (N = 4096): six values instead of fifteen (w^r = w^(4a) w^b) keep the kernel at 4 per CU
    cpx<T> tw3[R3 == 16 ? 1 : NTW3], tw3a[3], tw3b[3];
    if constexpr (R3 == 16) F::template load_twiddles16_split<256>(tw3a, tw3b, t, tw);
    else F::template load_twiddles<R3, 256>(tw3, t, tw);
    if (tid < 240) {
        int k = tid / 15, r = tid % 15 + 1;
        tw2l[k * 17 + r - 1] = wtab[r * k * (N / 256)];
    }
    __syncthreads();
    const cpx<T>* tw2p = tw2l + (t & 15) * 17;
    const int nvalid = io.in_valid ? (int)io.in_valid : N;
    const size_t groups = (batch + B - 1) / B;
    for (size_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        const size_t vec = gi * B + c;
        const bool active = vec < batch;
        const cpx<T>* in = reinterpret_cast<const cpx<T>*>(io.in) + vec * io.in_stride;
        cpx<T> v[16];
        const int rx = (io.flags & BDSP_FFT_SHIFT_IN) ? 8 : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int idx = t + (r ^ rx) * NT;
            v[r] = (active && idx < nvalid) ? in[idx] : cpx<T>{0, 0};
        }
        if (io.in_scale != (T)1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = cpx<T>{v[r].x * io.in_scale, v[r].y * io.in_scale};
        }
        F::template compute<16, 1, DIR>(v, t, tw);
        __syncthreads(); // the previous transform's last gather is done
        if constexpr (N == 4096) F::scatter_a(v, t, l); else F::template scatter<16, 1>(v, t, l);
        __syncthreads();
        if constexpr (N == 4096) F::gather_a(v, t, l); else F::template gather<16>(v, t, l);
        F::template compute_pre<16, 16, DIR>(v, tw2p);
        __syncthreads();
        if constexpr (N == 4096) F::scatter_b(v, t, l); else F::template scatter<16, 16>(v, t, l);
        __syncthreads();
        if constexpr (N == 4096) F::gather_b(v, t, l); else F::template gather<R3>(v, t, l);
        if constexpr (R3 == 16) F::template compute_pre16_split<256, DIR>(v, tw3a, tw3b);
        else F::template compute_pre<R3, 256, DIR>(v, tw3);
        if (active) {
            cpx<T>* out = reinterpret_cast<cpx<T>*>(io.out) + vec * io.out_stride;
            const int sx = (io.flags & BDSP_FFT_SHIFT_OUT) ? R3 / 2 : 0;
#pragma unroll
            for (int b = 0; b < 16 / R3; ++b)
#pragma unroll
                for (int r = 0; r < R3; ++r) out[F::template out_index<R3, N / R3>(t, b, r ^ sx)] = v[b * R3 + r];
        }
    }
}

// 8192-point transforms in ONE workgroup (f32, plain I/O): 512 threads x 16 points,
// four stages 16 x 16 x 16 x 2 (the template also covers 16384 = ... x 4 with 1024 threads), three LDS exchanges -- one trip through HBM (16 B per point) where the
// two-pass plan makes two, and one launch instead of two for a single transform.  Persistent over the batch;
// second-stage twiddles in an LDS table, last-stage twiddles in registers, third-stage twiddles from L2.
template <typename T, int N, int DIR>
__global__ __launch_bounds__(N / 16) void k_fft_wg4(FftIo<T> io, const cpx<T>* __restrict__ wtab, size_t batch)
{
    constexpr int NT = N / 16, R4 = N / 4096, NTW4 = (16 / R4) * (R4 - 1);
    static_assert(R4 == 2 || R4 == 4, "N in {8192, 16384}");
    using F = WgFft<T, N, NT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cpx<T>* l = reinterpret_cast<cpx<T>*>(smem_raw);
    cpx<T>* tw2l = l + F::LDS_ELEMS;
    const int t = threadIdx.x;
    auto tw = [&](int m) { return wtab[m]; };
    cpx<T> tw4[NTW4];
    F::template load_twiddles<R4, 4096>(tw4, t, tw);
    if (t < 240) {
        int k = t / 15, r = t % 15 + 1;
        tw2l[k * 17 + r - 1] = wtab[r * k * (N / 256)];
    }
    __syncthreads();
    const cpx<T>* tw2p = tw2l + (t & 15) * 17;
    const int nvalid = io.in_valid ? (int)io.in_valid : N;
    for (size_t vec = blockIdx.x; vec < batch; vec += gridDim.x) {
        const cpx<T>* in = reinterpret_cast<const cpx<T>*>(io.in) + vec * io.in_stride;
        cpx<T> v[16];
        const int rx = (io.flags & BDSP_FFT_SHIFT_IN) ? 8 : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int idx = t + (r ^ rx) * NT;
            v[r] = idx < nvalid ? in[idx] : cpx<T>{0, 0};
        }
        if (io.in_scale != (T)1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = cpx<T>{v[r].x * io.in_scale, v[r].y * io.in_scale};
        }
        F::template compute<16, 1, DIR>(v, t, tw);
        __syncthreads(); // the previous transform's last gather is done
        F::template scatter<16, 1>(v, t, l);
        __syncthreads();
        F::template gather<16>(v, t, l);
        F::template compute_pre<16, 16, DIR>(v, tw2p);
        __syncthreads();
        F::template scatter<16, 16>(v, t, l);
        __syncthreads();
        F::template gather<16>(v, t, l);
        F::template compute<16, 256, DIR>(v, t, tw);
        __syncthreads();
        F::template scatter<16, 256>(v, t, l);
        __syncthreads();
        F::template gather<R4>(v, t, l);
        F::template compute_pre<R4, 4096, DIR>(v, tw4);
        cpx<T>* out = reinterpret_cast<cpx<T>*>(io.out) + vec * io.out_stride;
        const int sx = (io.flags & BDSP_FFT_SHIFT_OUT) ? R4 / 2 : 0;
#pragma unroll
        for (int b = 0; b < 16 / R4; ++b)
#pragma unroll
            for (int r = 0; r < R4; ++r) out[F::template out_index<R4, N / R4>(t, b, r ^ sx)] = v[b * R4 + r];
    }
}

// ------------------------------------------------------------------------------ n > 4096
// exp(-2*pi*i*e/n) for an exact integer e < n (n a power of two): the argument 2e/n is exact in
// float for n <= 2^24 and always exact in double, so the only error is sincospi's own.
template <typename T>
__device__ __forceinline__ cpx<T> unit_root(size_t e, size_t n);
template <>
__device__ __forceinline__ cpx<float> unit_root<float>(size_t e, size_t n)
{
    if (n <= (size_t(1) << 24)) {
        float s, c;
        sincospif((float)e * (2.0f / (float)n), &s, &c);
        return {c, -s};
    }
    double s, c;
    sincospi((double)e * (2.0 / (double)n), &s, &c);
    return {(float)c, (float)-s};
}
template <>
__device__ __forceinline__ cpx<double> unit_root<double>(size_t e, size_t n)
{
    double s, c;
    sincospi((double)e * (2.0 / (double)n), &s, &c);
    return {c, -s};
}

// One global Stockham iteration of super-radix RP on vectors of n points:
//   column j (0 <= j < n/RP), k = j mod nsg:
//     v[row] = in[j + row*n/RP] * w_{nsg*RP}^{row*k}            row = 0..RP-1
//     v      = DFT_RP(v)
//     out[(j/nsg)*nsg*RP + k + row*nsg] = v[row]
// A workgroup (256 threads, 16 points each) owns W = 4096/RP adjacent columns.
// ROWMAP selects how the LAST inner stage maps lanes: along rows (first global pass, where each
// column's RP results are contiguous in memory) or along columns (later passes, where adjacent
// columns are contiguous).
// GEN: fused options on the vector's input (first pass = the ROWMAP instantiation) or output (last
// pass = a !ROWMAP instantiation), staged through LDS by a rolled loop like k_fft_wg<GEN>.
// SIMPLE: plain complex input without scale / window / shift / real input on the first pass and a plain complex output
// on a later one -- the instantiation the headline transforms take.  The run-time option checks around the loads and
// stores are then compiled out: the branches themselves are free, but hipcc's code around their merge points is not
// (the same lesson as in conv_v2.hip).
// The reference's windows on the sixteen values a pass thread holds, in registers (round 4).  In the first pass
// (input side) and in the last one (output side) a thread's sixteen points form the lattice i0 + m n/16, m = 0..15, with
// i0 < n/16 (rows are n/16 points apart); lattice(reg) says which m register `reg` holds.  Evaluated symmetrically like the
// reference (vector_types/mod.rs:567-594: w(i) = w(n-1-i)): point m >= 8 takes the value of its mirror image
// i1 + (15 - m) n/16, i1 = n/16 - 1 - i0.
//   Hamming / Hann (id 1) and Blackman-Harris (id 2): cos(2 pi i/(n-1)) = cos(theta_b + mm D) from TWO small base angles
//   per thread and the eight constants cos / sin(mm D) the launcher put into io (before: sixteen cospi per thread in f32,
//   three sincospi + sixteen chained rotations in f64, and Blackman-Harris through the staged generic loop with three
//   cospi per ELEMENT); Blackman-Harris's harmonics by cos 2t = 2c^2 - 1, cos 3t = c (4c^2 - 3).
//   Triangular (id 0): the reference's formula, 1 - |(jm - (n-1)/2) / (n/2)|, on the mirrored index jm.
// INV: divide by the window instead (windowed_ifft's un-windowing of the output, time.rs:50-66).
// FIXED >= 0: the window id is a compile-time constant.  The f64 tiles with the split exchange live at a 128-register
// budget; with the code of all three windows in one kernel they spilled 24-54 registers, so THEIR kernels are instantiated
// per window (k_fft_pass WIN) and each carries one loop.
template <typename T, int FIXED, bool INV, class LATTICE>
__device__ __forceinline__ void pass_window16(const FftIo<T>& io, size_t i0, size_t n, cpx<T> (&v)[16], LATTICE lattice)
{
    const size_t i1 = n / 16 - 1 - i0;
    auto put = [&](int reg, T w) {
        if (INV) w = (T)1 / w;
        v[reg] = cpx<T>{v[reg].x * w, v[reg].y * w};
    };
    const int wid = FIXED >= 0 ? FIXED : io.window_id;
    if (wid == 0) {
        const T b0 = ((T)i0 - ((T)n - (T)1) / (T)2) / ((T)n / (T)2), b1 = ((T)i1 - ((T)n - (T)1) / (T)2) / ((T)n / (T)2);
        const T step = (T)0.125; // (n/16) / (n/2)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = lattice(reg);
            put(reg, (T)1 - dev_abs((m < 8 ? b0 : b1) + step * (T)(m < 8 ? m : 15 - m)));
        }
        return;
    }
    const T two_over = (T)2 / ((T)n - (T)1);
    T s0, c0, s1, c1;
    dev_sincospi<T>((T)i0 * two_over, &s0, &c0);
    dev_sincospi<T>((T)i1 * two_over, &s1, &c1);
    if (wid == 1) {
        const T beta = (T)1 - io.window_alpha;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = lattice(reg), mm = m < 8 ? m : 15 - m;
            const T c = (m < 8 ? c0 : c1) * io.win_c[mm] - (m < 8 ? s0 : s1) * io.win_s[mm];
            put(reg, io.window_alpha - beta * c);
        }
    } else {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = lattice(reg), mm = m < 8 ? m : 15 - m;
            const T c = (m < 8 ? c0 : c1) * io.win_c[mm] - (m < 8 ? s0 : s1) * io.win_s[mm];
            const T c2 = c * c;
            put(reg, (T)0.35875 - (T)0.48829 * c + (T)0.14128 * ((T)2 * c2 - (T)1) - (T)0.01168 * (c * ((T)4 * c2 - (T)3)));
        }
    }
}

// WIN: -1 = the window id is read at run time (and is Hamming / Hann where the tile uses the split exchange); 0 / 2: the
// split-exchange tiles' instantiations for the triangular and the Blackman-Harris window (pass_window16 FIXED).
// NTL (round 5): the FIRST pass reads its input -- dead once read -- with non-temporal loads.  f64 only, and only where the
// tile's runs are whole 128-byte lines (pass_ntl_candidate): see launch_pass for the measurements.
template <typename T, int RP, int W, int DIR, bool ROWMAP, bool GEN, bool SIMPLE = false, int WIN = -1, bool NTL = false>
__global__ __launch_bounds__(W * (RP / 16), (pass_min_waves<T, RP, W, GEN>())) void k_fft_pass(FftIo<T> io, const cpx<T>* src, // (src may equal dst: the in-place last pass)
                                                   cpx<T>* dst,
                                                   const cpx<T>* __restrict__ wtab, size_t n,
                                                   size_t nsg, size_t tiles_per_vec, int last)
{
    constexpr int NT = RP / 16;
    constexpr int CS = col_stride(RP, W);
    using F = WgFft<T, RP, NT>;
    using P = Radix16Plan<RP>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr bool SPLIT = pass_split_exchange<T, RP, W, GEN>();
    using LE = typename std::conditional<SPLIT, T, cpx<T>>::type; // what an LDS slot holds
    LE* lds = reinterpret_cast<LE*>(smem_raw);

    const int tid = threadIdx.x;
    size_t blk = blockIdx.x;
    const size_t vec = blk / tiles_per_vec;
    size_t tile = blk % tiles_per_vec;
    // XCD-aware placement: block b runs on XCD b % 8; give each XCD a contiguous run of tiles so
    // neighbouring tiles (which share cache lines when W*sizeof(cpx) < 128 B) meet in one L2.
    if ((tiles_per_vec & 7) == 0) tile = (tile & 7) * (tiles_per_vec >> 3) + (tile >> 3);
    const size_t j0 = tile * W;
    const size_t stride_in = n / RP;
    constexpr bool LTW = pass_lds_twiddles<T, RP, W, GEN>();
    static_assert(!(LTW && SPLIT), "a split tile has no room for the table");
    cpx<T>* ltw = reinterpret_cast<cpx<T>*>(lds + (size_t)W * CS); // [RP] copy of the twiddle table (visible after the first barrier below)
    if constexpr (LTW) {
        for (int i = tid; i < RP; i += W * NT) ltw[i] = wtab[i];
    }
    auto tw = [&](int m) { return LTW ? ltw[m] : wtab[m]; };

    // ---- load (lanes along columns: W contiguous points per row)
    const int c = tid % W, ti = tid / W;
    const size_t j = j0 + c;
    cpx<T> v[16];
    if constexpr (GEN && ROWMAP) {
#pragma unroll 1
        for (int e = 0; e < 16; ++e) {
            int row = ti + e * NT;
            lds[(size_t)c * CS + F::pad(row)] = io_load(io, vec, j + (size_t)row * stride_in);
        }
        __syncthreads();
        F::template gather<16>(v, ti, lds + (size_t)c * CS);
        __syncthreads();
    } else {
        const cpx<T>* in = src + vec * n + j;
        // first pass (ROWMAP): ifft_shift = the row index's top bit flipped = register r ^ 8's address
        const int rx = (!SIMPLE && ROWMAP && (io.flags & BDSP_FFT_SHIFT_IN)) ? 8 : 0;
        if (!SIMPLE && ROWMAP && (io.flags & FFT_IN_REAL)) {
            // real input: `points` scalars per vector, imaginary parts are zero (time_to_freq.rs:147-150)
            const T* inr = reinterpret_cast<const T*>(io.in) + vec * io.in_stride + j;
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = cpx<T>{inr[(size_t)(ti + (r ^ rx) * NT) * stride_in], (T)0};
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                v[r] = NTL ? nt_load(&in[(size_t)(ti + (r ^ rx) * NT) * stride_in]) : in[(size_t)(ti + (r ^ rx) * NT) * stride_in];
        }
        if (!SIMPLE && ROWMAP && io.in_scale != (T)1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = cpx<T>{v[r].x * io.in_scale, v[r].y * io.in_scale};
        }
        if (!SIMPLE && ROWMAP && io.window_id >= 0 && io.window_id <= 2 && !(io.flags & FFT_WINDOW_OUT_DIV)) {
            // the window on the input, in registers: register r holds row q = r ^ rx (rx is 0 or 8), i.e. lattice point q
            pass_window16<T, (SPLIT ? (WIN >= 0 ? WIN : 1) : -1), false>(io, j + (size_t)ti * stride_in, n, v, [&](int r) { return r ^ rx; });
        }
    }
    if (!ROWMAP) { // (nsg > 1 exactly on the later passes)
        // inter-pass twiddle w_n^{row*q}, q = k * n/(nsg*RP); row = ti + r*NT: register r carries bs * d1^r with
        // bs = w_n^(ti q), d1 = w_n^(NT q) -- i.e. the first inner stage IS a twiddled 16-point transform with base
        // d1 on inputs scaled by bs (round 3: dft16_tw from d1, d1^2 and their products with constants; before, fifteen
        // powers of d1 were built and multiplied in one by one: 44 complex multiplies and 64 more f64 registers)
        const size_t k = j % nsg;
        const size_t q = k * (n / (nsg * RP));
        const cpx<T> bs = unit_root<T>(((size_t)ti * q) & (n - 1), n);
        const cpx<T> d1 = unit_root<T>(((size_t)NT * q) & (n - 1), n);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = twmul<DIR>(v[r], bs);
        const cpx<T> held[2] = {cmul(d1, d1), d1};
        cpx<T> t8[8];
        expand_twiddles16_fma<2>(held, t8);
        dft16_tw<DIR>(&v[0], t8);
    } else {
        F::template compute<16, 1, DIR>(v, ti, tw);
    }

    // ---- RP-point sub-FFT of every column
    const int c2 = ROWMAP ? tid / NT : tid % W;
    const int t2 = ROWMAP ? tid % NT : tid / W;
    LE* l1 = lds + (size_t)c * CS;
    LE* l2 = lds + (size_t)c2 * CS;
    if constexpr (SPLIT) {
        // real parts, then imaginary parts, through the half-size buffer (straight from / into the registers' halves)
        F::template scatter<16, 1>(PartRef<cpx<T>, false>{v}, ti, l1);
        __syncthreads();
        F::template gather<P::R2>(PartRef<cpx<T>, false>{v}, t2, l2);
        __syncthreads();
        F::template scatter<16, 1>(PartRef<cpx<T>, true>{v}, ti, l1);
        __syncthreads();
        F::template gather<P::R2>(PartRef<cpx<T>, true>{v}, t2, l2);
    } else {
        F::template scatter<16, 1>(v, ti, l1);
        __syncthreads();
        F::template gather<P::R2>(v, t2, l2);
    }
    F::template compute<P::R2, 16, DIR>(v, t2, tw);
    if constexpr (P::R3 > 1) {
        __syncthreads();
        if constexpr (SPLIT) {
            F::template scatter<P::R2, 16>(PartRef<cpx<T>, false>{v}, t2, l2);
            __syncthreads();
            F::template gather<P::R3>(PartRef<cpx<T>, false>{v}, t2, l2);
            __syncthreads();
            F::template scatter<P::R2, 16>(PartRef<cpx<T>, true>{v}, t2, l2);
            __syncthreads();
            F::template gather<P::R3>(PartRef<cpx<T>, true>{v}, t2, l2);
        } else {
            F::template scatter<P::R2, 16>(v, t2, l2);
            __syncthreads();
            F::template gather<P::R3>(v, t2, l2);
        }
        F::template compute<P::R3, 16 * P::R2, DIR>(v, t2, tw);
    }

    // ---- autosorted store
    constexpr int RL = P::R3 > 1 ? P::R3 : P::R2;
    constexpr int NSL = RP / RL;
    const size_t jj = j0 + c2;
    const size_t base = (jj / nsg) * nsg * RP + (jj % nsg);
    bool staged = false;
    if constexpr (GEN && !ROWMAP) {
        if (last) {
            staged = true;
            __syncthreads();
#pragma unroll
            for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
                for (int r = 0; r < RL; ++r)
                    l2[F::pad(F::template out_index<RL, NSL>(t2, b, r))] = v[b * RL + r];
            __syncthreads();
#pragma unroll 1
            for (int e = 0; e < 16; ++e) {
                int row = t2 + e * NT;
                io_store(io, vec, base + (size_t)row * nsg, l2[F::pad(row)]);
            }
        }
    }
    if (!staged) {
        cpx<T>* out = dst + vec * n + base;
        // last pass: fft_shift = the row index's top bit flipped; the last inner stage's digit r is that top digit
        const int sx = (!SIMPLE && last && !ROWMAP && (io.flags & BDSP_FFT_SHIFT_OUT)) ? RL / 2 : 0;
        if (!SIMPLE && last && !ROWMAP && (io.flags & FFT_WINDOW_OUT_DIV) && io.window_id >= 0 && io.window_id <= 2) {
            // windowed_ifft: the division by the window in the registers of the last pass (round 4; before: the staged
            // loop, 16M points f32 150 us for Hamming and 181 for Blackman-Harris against 133 for ifft).  Register
            // b RL + r goes to row t2 + (b + (r ^ sx) 16/RL) RP/16, i.e. lattice point b + (r ^ sx) 16/RL of jj + t2 n/RP
            pass_window16<T, (SPLIT ? (WIN >= 0 ? WIN : 1) : -1), true>(io, jj + (size_t)t2 * nsg, n, v, [&](int reg) { return reg / RL + ((reg % RL) ^ sx) * (16 / RL); });
        }
        if (!SIMPLE && last && !ROWMAP && (io.flags & (BDSP_FFT_MAGNITUDE | FFT_OUT_REAL))) {
            // magnitude / real part straight from the registers: `points` reals per vector
            T* outr = reinterpret_cast<T*>(io.out) + vec * io.out_stride + base;
            const bool mag = (io.flags & BDSP_FFT_MAGNITUDE) != 0;
#pragma unroll
            for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
                for (int r = 0; r < RL; ++r) {
                    const cpx<T> z = v[b * RL + r];
                    // (streamed with non-temporal stores: C2 x 64 377 -> 422 us -- 4-byte pieces of a line arrive from different
                    // lanes and instructions and need the cache to be merged)
                    outr[(size_t)F::template out_index<RL, NSL>(t2, b, r ^ sx) * nsg] = mag ? dev_hypot<T>(z.x, z.y) : z.x;
                }
            return;
        }
#pragma unroll
        for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
            for (int r = 0; r < RL; ++r)
                // (plain stores: non-temporal ones measured 16M f32 points 127 -> 181 us, C2 x 64 379 -> 427 -- a pass's output
                // is the next pass's input and the Infinity Cache holds it; 2^25 / 2^26 points and 16M f64, whose buffers exceed
                // the cache: +-1 %; streaming only the LAST pass's result: no difference.  DESIGN.md 4.2)
                out[(size_t)F::template out_index<RL, NSL>(t2, b, r ^ sx) * nsg] = v[b * RL + r];
    }
}

// (one 2^20-point f32 vector as two half-column launches, k_fft_half512: measured slower, round 4 -- docs/HISTORY.md A)

// ------------------------------------------------------------------------------ launchers
// (plain or generic I/O -- io_in_generic, io_out_generic, io_is_generic -- is decided in fft_plan_core.h)

template <typename T>
static size_t wg_lds_bytes(int n)
{
    int nt = n / 16;
    int b = 256 / nt;
    return (size_t)b * col_stride(n) * sizeof(cpx<T>);
}

template <typename T, int N>
static int launch_wg4(const FftIo<T>& io, size_t batch, bool inverse, hipStream_t s)
{
    const cpx<T>* wtab;
    BDSP_TRY(twiddle_table<T>(N, &wtab));
    using F = WgFft<T, N, N / 16>;
    const size_t lds = (size_t)(F::LDS_ELEMS + 16 * 17) * sizeof(cpx<T>);
    const size_t slots = (size_t)num_cus() * (N == 8192 ? 2 : 1);
    const unsigned grid = (unsigned)(batch < slots ? batch : slots);
    if (inverse) {
        BDSP_TRY(kernel_lds(k_fft_wg4<T, N, 1>, lds));
        hipLaunchKernelGGL((k_fft_wg4<T, N, 1>), dim3(grid), dim3(N / 16), lds, s, io, wtab, batch);
    } else {
        BDSP_TRY(kernel_lds(k_fft_wg4<T, N, -1>, lds));
        hipLaunchKernelGGL((k_fft_wg4<T, N, -1>), dim3(grid), dim3(N / 16), lds, s, io, wtab, batch);
    }
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, int N>
static int launch_wg(const FftIo<T>& io, size_t batch, bool inverse, hipStream_t s)
{
    const cpx<T>* wtab;
    BDSP_TRY(twiddle_table<T>(N, &wtab));
    constexpr int B = 256 / (N / 16);
    size_t lds = wg_lds_bytes<T>(N);
    unsigned grid = (unsigned)((batch + B - 1) / B);
    const bool gen = io_is_generic(io);
    // k_fft_wg_batch (persistent workgroups) serves f32 only.  Round 5, on valid data (profiles/r05_plan_probe_valid.txt; the
    // round-2 figures came from loops on inf / NaN): f32 4096 x 4096 points 53.5 us cold / 46 hot against 61.3 / 49.7 for the
    // plain launch, 16384 x 4096 213 / 190 against 209-220 / 200-233; f64 LOSES at every size -- 16384 x 1024 points 107 / 94
    // against 97 / 89, x 2048 210 / 199 against 186 / 171, x 4096 439 / 426 against 387 / 374, 4096 x 4096 113 / 97 against
    // 105 / 96 -- so it has no f64 instantiations.
    constexpr bool WGBATCH = N >= 1024 && sizeof(T) == 4;
#if BDSP_FFT_PART == 1
    if (gen) return launch_wg_gen<T>(N, io, batch, inverse, s); // the options unit
#endif
    if constexpr (WGBATCH && BDSP_FFT_PART != 2) {
        // enough transforms to keep persistent workgroups busy for several rounds
        // resident workgroups per CU as the runtime computes it (registers and LDS); the forward kernel's for both directions
        size_t lds2 = lds + 16 * 17 * sizeof(cpx<T>);
        int occ = 1;
        if (kernel_slots(k_fft_wg_batch<T, N, -1>, 256, lds2, &occ) != BDSP_OK) occ = 1; // (the launch taken reports)
        const size_t slots = (size_t)num_cus() * (size_t)occ;
        if (!gen && grid >= 4 * slots && !(io.flags & (BDSP_FFT_MAGNITUDE | FFT_OUT_REAL | FFT_IN_REAL))) {
            if (inverse) {
                BDSP_TRY(kernel_lds(k_fft_wg_batch<T, N, 1>, lds2));
                hipLaunchKernelGGL((k_fft_wg_batch<T, N, 1>), dim3((unsigned)slots), dim3(256), lds2, s, io, wtab, batch);
            } else {
                BDSP_TRY(kernel_lds(k_fft_wg_batch<T, N, -1>, lds2));
                hipLaunchKernelGGL((k_fft_wg_batch<T, N, -1>), dim3((unsigned)slots), dim3(256), lds2, s, io, wtab, batch);
            }
            BDSP_LAUNCH_CHECK();
            return BDSP_OK;
        }
    }
#define BDSP_WG(DIRV, GENV)                                                                        \
    do {                                                                                           \
        BDSP_TRY(kernel_lds(k_fft_wg<T, N, DIRV, GENV>, lds));                                     \
        hipLaunchKernelGGL((k_fft_wg<T, N, DIRV, GENV>), dim3(grid), dim3(256), lds, s, io, wtab,  \
                           batch);                                                                 \
    } while (0)
#if BDSP_FFT_PART == 1
    if (inverse) BDSP_WG(1, false); else BDSP_WG(-1, false);
#elif BDSP_FFT_PART == 2
    if (!gen) { set_last_error("plain transform in the options unit"); return BDSP_ERR_UNSUPPORTED; }
    if (inverse) BDSP_WG(1, true); else BDSP_WG(-1, true);
#else
    if (inverse) { if (gen) BDSP_WG(1, true); else BDSP_WG(1, false); }
    else { if (gen) BDSP_WG(-1, true); else BDSP_WG(-1, false); }
#endif
#undef BDSP_WG
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, int N>
static int launch_tiny(const FftIo<T>& io, size_t batch, bool inverse, hipStream_t s)
{
    unsigned grid = (unsigned)((batch + 255) / 256);
    if (inverse) hipLaunchKernelGGL((k_fft_tiny<T, N, 1>), dim3(grid), dim3(256), 0, s, io, batch);
    else hipLaunchKernelGGL((k_fft_tiny<T, N, -1>), dim3(grid), dim3(256), 0, s, io, batch);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// One global pass as fft_pass_route (fft_plan_core.h) describes it: this function only picks the instantiation the route
// names; it decides nothing itself.
template <typename T, int RP, int W>
static int launch_pass(const FftPassRoute& r, const FftIo<T>& io_in, const cpx<T>* src, cpx<T>* dst, size_t n, size_t nsg,
                       size_t batch, hipStream_t s)
{
    FftIo<T> io = io_in;
    const cpx<T>* const src0 = src;
    cpx<T>* const dst0 = dst;
    (void)src0; (void)dst0; // (used by the plain unit only, BDSP_FFT_PART == 1)
    const bool first = r.rowmap, last = r.last, inverse = r.dir > 0;
    if (r.rp != RP || r.w != W || r.rowmap != (nsg == 1) || r.threads != W * (RP / 16) || r.grid != (n / RP) / W * batch) {
        set_last_error("fft pass: route and launch disagree");
        return BDSP_ERR_UNSUPPORTED;
    }
    if ((first || last) && (io.window_id == 1 || io.window_id == 2) && n > 1) {
        // the window constants of k_fft_pass: cos / sin of q * 2 pi (n/16) / (n-1), q = 0..7, from double precision
        const double step = 2.0 * (double)(n / 16) / ((double)n - 1.0); // in units of pi
        for (int q = 0; q < 8; ++q) {
            io.win_c[q] = (T)std::cos(M_PI * step * q);
            io.win_s[q] = (T)std::sin(M_PI * step * q);
        }
    }
    const cpx<T>* wtab;
    BDSP_TRY(twiddle_table<T>(RP, &wtab));
    constexpr int THREADS = W * (RP / 16);
    const size_t tiles = r.tiles_per_vec;
    dim3 grid((unsigned)r.grid);
    const bool rowmap = r.rowmap; // the first pass
    const bool gen = r.gen;
    // (triangular / Blackman-Harris on a split-exchange f64 tile: the kernel instantiated for that window, see k_fft_pass)
    const int win_fixed = r.win_fixed;
    (void)win_fixed; // (the plain unit sends every windowed pass to the options unit)
    if (first && !gen) src = reinterpret_cast<const cpx<T>*>(io.in);
    if (last && !gen) dst = reinterpret_cast<cpx<T>*>(io.out);
    // plain first / last pass?  (then no option is looked at inside the kernel)
    const bool simple = r.simple;
#if BDSP_FFT_PART == 1
    if (!simple) return launch_pass_opts_rp<T>(r, io_in, src0, dst0, n, nsg, batch, s); // the options unit
#endif
    // Non-temporal loads in the FIRST pass of an f64 transform whose tile reads whole 128-byte lines (W >= 8: the 3-pass plans'
    // 256 x 16 / 128 x 32 tiles, the 1024 x 8 / 512 x 8 tiles of batches and of 2^18 points).  *Measured* (round 5, cold / input in
    // the caches, profiles/r05_plan_probe_valid.txt runs 4-5): 16 x 2^20 214 -> 185 / 205 -> 185 us,
    // 4 x 2^20 61.6 -> 54.0 / =, 2^23 141 -> 133 / 130 -> 127, 2^24 327 -> 324 / 312 -> 304, 32 x 2^20 419 -> 417 / 404 -> 398, 256 x 2^16 and
    // 2^18 equal.  NOT where the tile reads half lines (2^21 / 2^22 f64 single vectors: cold 36.6 -> 33.7 / 67.2 -> 60.8 but with
    // the input in the caches 28.1 -> 32.5 / 46.1 -> 62.3 -- every half line becomes a fetch of its own), and not in f32, where it
    // is a wash or worse (2^23 -5 % cold, 2^24 -6 % cold / +1 % hot, 2^25 +6 %, 64 x 2^20 +8 %, 4096 x 2^14 +1 %).
    const bool ntl = r.ntl;
#define BDSP_PASS_K(DIRV, RM, GENV, SV, WINV, NTLV)                                                 \
    do {                                                                                           \
        constexpr size_t lds = pass_tile_lds_bytes<T, RP, W, GENV>() +                             \
                               (pass_lds_twiddles<T, RP, W, GENV>() ? (size_t)RP * sizeof(cpx<T>) : 0); \
        if (lds != r.lds_bytes) { set_last_error("fft pass: route and kernel disagree on LDS"); return BDSP_ERR_UNSUPPORTED; } \
        BDSP_TRY(kernel_lds(k_fft_pass<T, RP, W, DIRV, RM, GENV, SV, WINV, NTLV>, lds));           \
        hipLaunchKernelGGL((k_fft_pass<T, RP, W, DIRV, RM, GENV, SV, WINV, NTLV>), grid, dim3(THREADS), lds, s, \
                           io, src, dst, wtab, n, nsg, tiles, (int)last);                          \
    } while (0)
#define BDSP_PASS(DIRV, RM, GENV, SV, WINV)                                                        \
    do {                                                                                           \
        if constexpr (pass_ntl_candidate<T, RP, W>() && RM && !GENV) {                             \
            if (ntl) { BDSP_PASS_K(DIRV, RM, GENV, SV, WINV, true); break; }                       \
        }                                                                                          \
        BDSP_PASS_K(DIRV, RM, GENV, SV, WINV, false);                                              \
    } while (0)
#if BDSP_FFT_PART == 1
#define BDSP_PASS_V(DIRV, RM) BDSP_PASS(DIRV, RM, false, true, -1) /* (everything else went to the options unit above) */
#else
#if BDSP_FFT_PART == 2
#define BDSP_PASS_SIMPLE(DIRV, RM) do { set_last_error("plain pass in the options unit"); return BDSP_ERR_UNSUPPORTED; } while (0)
#else
#define BDSP_PASS_SIMPLE(DIRV, RM) BDSP_PASS(DIRV, RM, false, true, -1)
#endif
#define BDSP_PASS_V(DIRV, RM)                                                                      \
    do {                                                                                           \
        if (gen) BDSP_PASS(DIRV, RM, true, false, -1);                                             \
        else if (simple) BDSP_PASS_SIMPLE(DIRV, RM);                                               \
        else {                                                                                     \
            if constexpr (pass_split_exchange<T, RP, W, false>()) {                                \
                if (win_fixed == 0) { BDSP_PASS(DIRV, RM, false, false, 0); break; }               \
                if (win_fixed == 2) { BDSP_PASS(DIRV, RM, false, false, 2); break; }               \
            }                                                                                      \
            BDSP_PASS(DIRV, RM, false, false, -1);                                                 \
        }                                                                                          \
    } while (0)
#endif
#define BDSP_PASS_D(DIRV)                                                                          \
    do {                                                                                           \
        if (rowmap) BDSP_PASS_V(DIRV, true);                                                       \
        else if constexpr (pass_first_only<RP, W>()) { set_last_error("first-pass-only tile"); return BDSP_ERR_UNSUPPORTED; } \
        else BDSP_PASS_V(DIRV, false);                                                             \
    } while (0)
    if (inverse) BDSP_PASS_D(1); else BDSP_PASS_D(-1);
#undef BDSP_PASS_D
#undef BDSP_PASS_V
#undef BDSP_PASS
#undef BDSP_PASS_K
#if BDSP_FFT_PART != 1
#undef BDSP_PASS_SIMPLE
#endif
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// (super-radix, tile width) pairs that are instantiated: the ones pass_tile_built (fft_plan_core.h) names.  Default tile:
// W = 4096/RP columns (256 threads); the wider variants trade LDS for longer contiguous global segments.
template <typename T>
static int launch_pass_rp(const FftPassRoute& r, const FftIo<T>& io, const cpx<T>* src, cpx<T>* dst,
                          size_t n, size_t nsg, size_t batch, hipStream_t s)
{
#define BDSP_CASE(RPV, WV)                                                                         \
    if (r.rp == RPV && r.w == WV) {                                                                \
        static_assert(pass_tile_built(sizeof(T), RPV, WV), "pass_tile_built lists the instantiated tiles"); \
        return launch_pass<T, RPV, WV>(r, io, src, dst, n, nsg, batch, s);                         \
    }
    // every pair plan_passes can choose
    BDSP_CASE(64, 64) BDSP_CASE(128, 32) BDSP_CASE(256, 16) BDSP_CASE(512, 8) BDSP_CASE(1024, 4)
    BDSP_CASE(1024, 8) BDSP_CASE(2048, 4)
    // (the first pass of 2^22 f32 points, round 5: the ROWMAP instantiations only, see pass_first_only; f64 4096 x 4 tiles spill
    // 12-76 bytes per lane)
    if constexpr (sizeof(T) == 4) { BDSP_CASE(4096, 4) }
#undef BDSP_CASE
    set_last_error("unsupported super-radix / tile width");
    return BDSP_ERR_UNSUPPORTED;
}

// (the plan -- how many passes, which tiles, when the one-workgroup kernel serves -- is fft_plan of fft_plan_core.h)

// Runs the transform described by `io` on power-of-two n.  io.in holds the input.  For n <= 4096
// the result goes to io.out (io.out may equal io.in unless the input is real).  For n > 4096 the
// passes ping-pong: in -> scratch_a -> [scratch_b ->] io.out; scratch buffers hold n*batch complex.
// scratch_b may be null for 2-pass sizes, and may alias io.in if the caller allows the input to be
// clobbered; io.out may alias io.in (it is written only by the last pass, which reads scratch).
template <typename T>
int fft_pow2(const FftIo<T>& io, T* scratch_a, T* scratch_b, size_t batch, bool inverse,
             hipStream_t s)
{
    const size_t n = io.n;
    if (batch == 0 || n == 0) return BDSP_OK;
    if (n == 1) {
        // a 1-point DFT is the identity; still honour scale/window/magnitude through the tiny path
        return launch_tiny<T, 1>(io, batch, inverse, s);
    }
    switch (n) {
    case 2: return launch_tiny<T, 2>(io, batch, inverse, s);
    case 4: return launch_tiny<T, 4>(io, batch, inverse, s);
    case 8: return launch_tiny<T, 8>(io, batch, inverse, s);
    case 16: return launch_wg<T, 16>(io, batch, inverse, s);
    case 32: return launch_wg<T, 32>(io, batch, inverse, s);
    case 64: return launch_wg<T, 64>(io, batch, inverse, s);
    case 128: return launch_wg<T, 128>(io, batch, inverse, s);
    case 256: return launch_wg<T, 256>(io, batch, inverse, s);
    case 512: return launch_wg<T, 512>(io, batch, inverse, s);
    case 1024: return launch_wg<T, 1024>(io, batch, inverse, s);
    case 2048: return launch_wg<T, 2048>(io, batch, inverse, s);
    case 4096: return launch_wg<T, 4096>(io, batch, inverse, s);
    default: break;
    }
    const FftPlan plan = fft_plan(sizeof(T), n, batch, num_cus(), io.flags, io.in_scale != (T)1, io.window_id, io.in_stride,
                                  io.out_stride, io.in_valid, inverse);
    const int passes = plan.passes;
    if constexpr (sizeof(T) == 4) {
        // *measured*: 8192 points, batch 2048: 94.8 us as two passes, 73.3 us in one workgroup each (batch 256:
        // 19.8 -> 13.2 us, a single transform 7.7 vs 7.9 us); the 16384-point instantiation (1024 threads, one
        // workgroup per CU) measured SLOWER than two passes at every batch size and is not built
        // (wg4_takes: the predicate this dispatch and bdsp_hip_fft_passes share, fft_plan_core.h)
        if (passes == 1) return launch_wg4<T, 8192>(io, batch, inverse, s);
    }
    if (passes == 0) { set_last_error("FFT length above 2^30 points"); return BDSP_ERR_UNSUPPORTED; }
    if (passes == 1) { set_last_error("fft_pow2: no one-workgroup kernel for this precision"); return BDSP_ERR_UNSUPPORTED; }
    if (!scratch_a || (passes == 3 && !scratch_b)) {
        set_last_error("fft_pow2: scratch missing");
        return BDSP_ERR_UNSUPPORTED;
    }
    cpx<T>* sa = reinterpret_cast<cpx<T>*>(scratch_a);
    cpx<T>* sb = reinterpret_cast<cpx<T>*>(scratch_b);
    size_t nsg = 1;
    // (the intermediate in natural order: a tiled layout, one contiguous block per second-pass tile, measured no faster --
    // round 4, profiles/r04_fft_tiled_intermediate.txt: the narrow reads were never the cost, its scattered stores are one)
    BDSP_TRY(launch_pass_rp<T>(plan.r[0], io, nullptr, sa, n, nsg, batch, s));
    nsg *= plan.r[0].rp;
    if (passes == 2) {
        BDSP_TRY(launch_pass_rp<T>(plan.r[1], io, sa, nullptr, n, nsg, batch, s));
    } else {
        BDSP_TRY(launch_pass_rp<T>(plan.r[1], io, sa, sb, n, nsg, batch, s));
        nsg *= plan.r[1].rp;
        BDSP_TRY(launch_pass_rp<T>(plan.r[2], io, sb, nullptr, n, nsg, batch, s));
    }
    return BDSP_OK;
}

// trips through global memory a power-of-two transform of n points makes (callers size and order their ping-pong
// buffers by it: 2 = in -> scratch_a -> out, 3 = in -> scratch_a -> scratch_b -> out)
template <typename T>
int fft_pow2_passes(size_t n)
{
    if (n <= 4096) return 1;
    return plan_pass_count(n, sizeof(T));
}

template <typename T>
int fft_pow2_plain_trips(size_t n)
{
    if (n == 0 || (n & (n - 1)) != 0) return 0;
    return wg4_serves<T>(n) ? 1 : fft_pow2_passes<T>(n);
}

#if BDSP_FFT_PART != 1
// the options unit's two entry points (with BDSP_FFT_PART == 0 they are defined here too and simply never called)
template <typename T>
int launch_pass_opts_rp(const FftPassRoute& r, const FftIo<T>& io, const cpx<T>* src, cpx<T>* dst, size_t n, size_t nsg, size_t batch,
                        hipStream_t s)
{
    return launch_pass_rp<T>(r, io, src, dst, n, nsg, batch, s);
}
template <typename T>
int launch_wg_gen(int n, const FftIo<T>& io, size_t batch, bool inverse, hipStream_t s)
{
    switch (n) {
    case 16: return launch_wg<T, 16>(io, batch, inverse, s);
    case 32: return launch_wg<T, 32>(io, batch, inverse, s);
    case 64: return launch_wg<T, 64>(io, batch, inverse, s);
    case 128: return launch_wg<T, 128>(io, batch, inverse, s);
    case 256: return launch_wg<T, 256>(io, batch, inverse, s);
    case 512: return launch_wg<T, 512>(io, batch, inverse, s);
    case 1024: return launch_wg<T, 1024>(io, batch, inverse, s);
    case 2048: return launch_wg<T, 2048>(io, batch, inverse, s);
    case 4096: return launch_wg<T, 4096>(io, batch, inverse, s);
    default: break;
    }
    set_last_error("launch_wg_gen: unsupported length");
    return BDSP_ERR_UNSUPPORTED;
}
#endif
#if BDSP_FFT_PART == 2
template int launch_pass_opts_rp<BDSP_FFT_T>(const FftPassRoute&, const FftIo<BDSP_FFT_T>&, const cpx<BDSP_FFT_T>*, cpx<BDSP_FFT_T>*, size_t, size_t, size_t,
                                             hipStream_t);
template int launch_wg_gen<BDSP_FFT_T>(int, const FftIo<BDSP_FFT_T>&, size_t, bool, hipStream_t);
#else
template int fft_pow2<BDSP_FFT_T>(const FftIo<BDSP_FFT_T>&, BDSP_FFT_T*, BDSP_FFT_T*, size_t, bool, hipStream_t);
template int fft_pow2_passes<BDSP_FFT_T>(size_t);
template int fft_pow2_plain_trips<BDSP_FFT_T>(size_t);
#endif

} // namespace bdsp
