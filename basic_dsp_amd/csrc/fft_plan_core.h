// fft_plan_core.h -- what a power-of-two transform above 4096 points launches, as host+device functions without a HIP
// runtime call: the plan (how many global passes, which (super-radix, tile width) each), the route of every pass (which
// k_fft_pass instantiation, its LDS, threads and grid), the buffer order of the two-buffer driver, and the mapping from
// the facade's operations to transform options.  fft_impl.h launches from these structs and capi.cpp orders its buffers
// by them; tests/host_sim/sim_fft_passes.cpp compiles the same text with the host compiler and checks
// tests/fft_pass_shapes.txt against it (tests/test_fft_plan_abi.py), and tests/test_gpu_fft_pass_routes.py runs every
// line of that table on the device.  There is no second copy of the rule.
#pragma once
#include <cstddef>

#include "../../include/basic_dsp_hip.h"
#include "fft_core.h"

#if defined(__HIPCC__)
#define BDSP_HDC __host__ __device__ constexpr
#else
#define BDSP_HDC constexpr
#endif

namespace bdsp {

// ---------------------------------------------------------------- fused FFT prologue / epilogue
template <typename T>
struct FftIo {
    const void* in;
    void* out;
    size_t n;          // points per vector
    size_t in_stride;  // elements (of the input element type) between consecutive batch vectors
    size_t out_stride; // elements (of the output element type) between consecutive batch vectors
    unsigned flags;    // BDSP_FFT_* (SHIFT_IN, SHIFT_OUT, MAGNITUDE) + internal bits below
    T in_scale;        // applied to every input element (1 = none)
    int window_id;     // -1 none; else reference window id (4 = Hann)
    T window_alpha;
    size_t in_valid;   // 0 = all n points; else points >= in_valid read as zero (fused End zero-padding)
    // cos / sin of q * 2 pi (n/16) / (n-1), q = 0..7: a pass thread's sixteen rows are n/16 points apart, so a generalised
    // Hamming window costs it two sincospi and sixteen multiply-adds (filled by launch_pass; k_fft_pass, round 4)
    T win_c[8], win_s[8];
};
constexpr unsigned FFT_IN_REAL = 1u << 8;        // input is a real vector (zero imaginary parts)
constexpr unsigned FFT_WINDOW_OUT_DIV = 1u << 9; // divide OUTPUT by the window (windowed_ifft)
constexpr unsigned FFT_OUT_REAL = 1u << 10;      // write only the real parts

// ---------------------------------------------------------------- tiles of a global pass
// LDS stride (in elements) between the regions of adjacent columns / transforms of one workgroup.
// Lanes that run along columns hit addresses c*stride + const: with the padded length alone the
// stride is a multiple of 16 elements = a multiple of 32 banks, i.e. a 16-way conflict (measured:
// 90 % of LDS cycles were conflict cycles).  stride = 16*k + max(1, 16/W) spreads the W columns of a
// 16-lane group over all banks, and leaves room for the rows of a second thread-row when W < 16.
BDSP_HDC int col_stride(int n, int w = 0)
{
    int nt = n / 16 > 0 ? n / 16 : 1;
    if (w == 0) w = 256 / nt;
    int padded = n + (n >> 4);
    int base = (padded + 15) / 16 * 16;
    return base + (w >= 16 ? 1 : 16 / w);
}

// Inner-stage twiddles of a pass kernel from an LDS copy of the RP-entry table instead of global memory?  Yes whenever
// the copy does not cost a resident workgroup.  *Measured* on 64 x 2^20 points (two passes of 1024-point columns):
// 479 us with the 27 dependent global loads per thread and tile between an LDS gather and its butterflies, 405 us with
// the loads removed altogether (a timing experiment); keeping the twiddles in registers across a persistent tile
// loop instead made hipcc allocate 200+ VGPRs (532 us) or, with the budget capped at 128, spill (890 us).
BDSP_HDC int pass_wgs_per_cu(size_t lds_bytes, int threads)
{
    size_t k = (size_t)(160 * 1024) / (lds_bytes + 64);
    if (k > (size_t)(2048 / threads)) k = (size_t)(2048 / threads);
    if (k > 8) k = 8;
    return (int)k;
}

// The tile predicates on run-time values (esz = sizeof(T), a complex element is 2 esz bytes); the templates the kernels
// are instantiated with (below) are these functions on their own parameters.
// SPLIT exchange (round 3): an f64 tile of 2048 x 4 or 1024 x 8 points is 136 KB of LDS -- ONE 512-thread workgroup per
// CU, which loads, transforms and stores its tile with nothing to overlap any phase (config C4a's 4M points are two such
// tiles per CU in all).  These tiles therefore cross their real and imaginary parts one after the other through a
// buffer of HALF the size (8-byte elements: twice the LDS instructions and barriers, the same bytes), which lets two
// workgroups share a CU.  Not for the GEN instantiations, which stage whole complex values through the buffer.
BDSP_HDC bool pass_split_exchange_rt(size_t esz, int rp, int w, bool gen)
{
    return !gen && esz == 8 && (size_t)w * col_stride(rp, w) * (2 * esz) > 80 * 1024;
}
BDSP_HDC size_t pass_tile_lds_bytes_rt(size_t esz, int rp, int w, bool gen)
{
    return (size_t)w * col_stride(rp, w) * (pass_split_exchange_rt(esz, rp, w, gen) ? esz : 2 * esz);
}
BDSP_HDC bool pass_lds_twiddles_rt(size_t esz, int rp, int w, bool gen)
{
    // ... and always for the 4-wide 1024-point f32 tiles: the plan picks them only when the launch has fewer than two
    // tiles per CU (one 2^20-point vector: 256 tiles), where the fourth resident workgroup the table costs is never there
    return (esz == 4 && rp == 1024 && w == 4)
               ? true
               : (rp >= 256 && pass_wgs_per_cu(pass_tile_lds_bytes_rt(esz, rp, w, gen), w * (rp / 16)) ==
                                   pass_wgs_per_cu(pass_tile_lds_bytes_rt(esz, rp, w, gen) + (size_t)rp * (2 * esz), w * (rp / 16)));
}
// first-pass tiles that read their (dead) input with non-temporal loads: f64, whole 128-byte lines per row (launch_pass)
BDSP_HDC bool pass_ntl_candidate_rt(size_t esz, int w) { return esz == 8 && (size_t)w * (2 * esz) >= 128; }
// tiles the plans use as a FIRST pass only: their later-pass instantiations are not built
BDSP_HDC bool pass_first_only_rt(int rp) { return rp == 4096; }

template <typename T, int RP, int W, bool GEN>
constexpr bool pass_split_exchange()
{
    return pass_split_exchange_rt(sizeof(T), RP, W, GEN);
}
template <typename T, int RP, int W, bool GEN>
constexpr size_t pass_tile_lds_bytes()
{
    return pass_tile_lds_bytes_rt(sizeof(T), RP, W, GEN);
}
// waves per SIMD the pass kernel is compiled for: the split tiles want two 512-thread workgroups per CU = 4 (128 VGPRs)
template <typename T, int RP, int W, bool GEN>
constexpr int pass_min_waves()
{
    return pass_split_exchange<T, RP, W, GEN>() ? 2 * (W * (RP / 16)) / 256 : 1;
}
template <typename T, int RP, int W, bool GEN = true>
constexpr bool pass_lds_twiddles()
{
    return pass_lds_twiddles_rt(sizeof(T), RP, W, GEN);
}
template <typename T, int RP, int W>
constexpr bool pass_ntl_candidate()
{
    return pass_ntl_candidate_rt(sizeof(T), W);
}
template <int RP, int W>
constexpr bool pass_first_only()
{
    return pass_first_only_rt(RP);
}

// (super-radix, tile width) pairs launch_pass_rp instantiates k_fft_pass for (its BDSP_CASE list is written from this)
BDSP_HDC bool pass_tile_built(size_t esz, int rp, int w)
{
    return (rp == 64 && w == 64) || (rp == 128 && w == 32) || (rp == 256 && w == 16) || (rp == 512 && w == 8) ||
           (rp == 1024 && w == 4) || (rp == 1024 && w == 8) || (rp == 2048 && w == 4) ||
           // (the first pass of 2^22 f32 points, round 5: the ROWMAP instantiations only, see pass_first_only; f64 4096 x 4
           // tiles spill 12-76 bytes per lane)
           (esz == 4 && rp == 4096 && w == 4);
}

// ---------------------------------------------------------------- plain or generic I/O
// plain complex in/out with the natural batch stride and no fused option?  The input side and the
// output side are judged separately so that e.g. fft->magnitude pays the staged path only in its
// last pass.
BDSP_HDC bool io_in_generic_rt(size_t n, unsigned flags, int window_id, size_t in_stride, size_t in_valid)
{
    // ifft_shift (a register renaming for even n) and the input scale are handled by the plain path
    // ... and so is a generalised Hamming window on the first global pass (n > 4096)
    // (... and so are all four reference windows -- the rectangular one multiplies by one -- on the first global pass)
    // ... and real input (zero imaginary parts)
    return (window_id >= 0 && !(flags & FFT_WINDOW_OUT_DIV) && !(window_id <= 3 && n > 4096)) || in_stride != n ||
           (in_valid != 0 && n > 4096);
}
BDSP_HDC bool io_out_generic_rt(size_t n, unsigned flags, int window_id, size_t out_stride)
{
    // fft_shift is handled by the plain path
    // ... and magnitude / real-part outputs are written straight from the registers
    // ... and so is the division by one of the reference's windows (windowed_ifft) on the last global pass
    return ((flags & FFT_WINDOW_OUT_DIV) != 0 && !(window_id >= 0 && window_id <= 3 && n > 4096)) || out_stride != n;
}
template <typename T>
BDSP_HD bool io_in_generic(const FftIo<T>& io) { return io_in_generic_rt(io.n, io.flags, io.window_id, io.in_stride, io.in_valid); }
template <typename T>
BDSP_HD bool io_out_generic(const FftIo<T>& io) { return io_out_generic_rt(io.n, io.flags, io.window_id, io.out_stride); }
template <typename T>
BDSP_HD bool io_is_generic(const FftIo<T>& io) { return io_in_generic(io) || io_out_generic(io); }

// ---------------------------------------------------------------- the plan
// Super-radix plan for n = 2^bits > 4096: 2 passes up to 2^20, 3 passes up to 2^30, bits split as
// evenly as possible, largest first (the first pass is the one whose stores are always long
// contiguous runs, so it can afford the narrowest tile).  0: n is above 2^30.
BDSP_HD int plan_passes(size_t n, size_t batch, size_t esz, int num_cus, int rp[3], int w[3])
{
    int bits = 0;
    while ((size_t(1) << bits) < n) ++bits;
    if (bits > 30) return 0;
    // 2^21 and 2^22 points: two passes of long columns beat three fully coalesced ones although their runs are only 32-64
    // bytes.  Round 5, re-measured on VALID data with input and scratch cold / input in the caches
    // (profiles/r05_plan_probe_valid.txt; the figures of rounds 2-3 came from loops that transformed their own output, i.e.
    // inf / NaN), last pass in place:
    //   2^21 f32  1024x8 + 2048x4  24.3 / 19.8 us   (2048x4 + 1024x8 24.6 / 19.2; three passes 30.3 / 26.9 out of place)
    //   2^22 f32  4096x4 + 1024x8  40.4 / 32.3      (2048x4 + 2048x4, the plan until round 5: 42.9 / 33.3; three passes 41.4 / 34.0)
    //   2^21 f64  1024x4 + 2048x4  36.6 / 28.4      (three passes 39.5 / 34.5)
    //   2^22 f64  2048x4 + 2048x4  66.9 / 47.0      (2048x2 + 2048x4 70.8 / 50.8; three passes 76.5 / 65.6)
    // From 2^23 on three passes win on a cold input: f32 71.2 / 65.7 against 78.9-86.7 / 63.3-63.8 for the 4096-point
    // columns, f64 137.9 / 131.1 against 140-147 / 121-132; 2^24 f32 132.5 / 129.2 against 173 / 149.
    if (bits == 21 || bits == 22) {
        if (esz == 4) {
            if (bits == 21) { rp[0] = 1024; w[0] = 8; rp[1] = 2048; w[1] = 4; }
            else { rp[0] = 4096; w[0] = 4; rp[1] = 1024; w[1] = 8; }
        } else {
            rp[0] = bits == 21 ? 1024 : 2048; rp[1] = 2048;
            w[0] = 4; w[1] = 4; // 2^22 f64: 2-wide first-pass tiles are no faster plain (above) and 7 us slower with a fused window
        }
        return 2;
    }
    int passes = bits <= 20 ? 2 : 3;
    int base = bits / passes, extra = bits % passes;
    for (int i = 0; i < passes; ++i) {
        rp[i] = 1 << (base + (i < extra ? 1 : 0));
        w[i] = 4096 / rp[i];
        // 1024-point columns: 8-wide tiles (64-byte segments, 512 threads) measured 14 % faster than
        // 4-wide ones on 64 x 2^20 points; 2-pass plans for 2^24 (4096x2 / 4096x4 tiles) measured
        // 30-70 % SLOWER than three fully coalesced 256-point passes, so 3 passes stay.
        // ... unless that leaves fewer tiles than two per CU (a single 2^20-point vector has 128):
        // then 4-wide tiles fill the chip (measured 19.8 -> 17.2 us for one 2^20-point transform)
        if (rp[i] == 1024) w[i] = (n * batch / 8192 >= (size_t)2 * (size_t)num_cus) ? 8 : 4;
    }
    return passes;
}

// trips through global memory of the passes above (the count does not depend on the batch or the device)
BDSP_HD int plan_pass_count(size_t n, size_t esz)
{
    int rp[3], w[3];
    return plan_passes(n, 1, esz, 1, rp, w);
}

// lengths whose PLAIN transform (no fused option) runs in the one-workgroup kernel k_fft_wg4 instead of two passes
BDSP_HDC bool wg4_serves_rt(size_t esz, size_t n) { return esz == 4 && n == 8192; }
template <typename T>
constexpr bool wg4_serves(size_t n)
{
    return wg4_serves_rt(sizeof(T), n);
}
// ... and what "plain" means there: complex in and out at the natural stride, no window, no real input or output (the
// input scale and the two shifts are register work in k_fft_wg4)
BDSP_HDC bool wg4_takes(size_t esz, size_t n, unsigned flags, int window_id, size_t in_stride, size_t out_stride, size_t in_valid)
{
    return wg4_serves_rt(esz, n) && !io_in_generic_rt(n, flags, window_id, in_stride, in_valid) &&
           !io_out_generic_rt(n, flags, window_id, out_stride) && window_id < 0 &&
           !(flags & (BDSP_FFT_MAGNITUDE | FFT_OUT_REAL | FFT_IN_REAL));
}

// ---------------------------------------------------------------- the route of one pass
struct FftPassRoute {
    int rp, w;         // super-radix and tile width: launch_pass<T, RP, W>
    bool rowmap;       // the first pass (nsg == 1): lanes of the last inner stage along rows
    bool gen;          // generic I/O staged through LDS (strided or zero-padded input on the first pass, strided output on the last)
    bool simple;       // no option is looked at inside the kernel
    int win_fixed;     // 0 / 2: the split tiles' kernels for the triangular / Blackman-Harris window; else -1
    bool ntl;          // non-temporal loads of the input (f64 first passes whose runs are whole 128-byte lines)
    bool split;        // real and imaginary parts cross LDS one after the other
    bool lds_twiddles; // the RP-entry twiddle table is copied behind the tile
    int dir;           // -1 forward, +1 inverse
    bool last;         // the pass that writes the result
    size_t lds_bytes;  // dynamic LDS of the launch
    int threads;       // per workgroup
    size_t grid;       // workgroups
    size_t tiles_per_vec;
};

BDSP_HD FftPassRoute fft_pass_route(size_t esz, int rp, int w, size_t n, size_t batch, bool first, bool last, bool inverse,
                                    unsigned flags, bool scaled /* in_scale != 1 */, int window_id, size_t in_stride,
                                    size_t out_stride, size_t in_valid)
{
    FftPassRoute r{};
    r.rp = rp;
    r.w = w;
    r.rowmap = first; // nsg == 1 exactly on the first pass
    r.last = last;
    r.dir = inverse ? 1 : -1;
    r.gen = (first && io_in_generic_rt(n, flags, window_id, in_stride, in_valid)) || (last && io_out_generic_rt(n, flags, window_id, out_stride));
    // (triangular / Blackman-Harris on a split-exchange f64 tile: the kernel instantiated for that window, see k_fft_pass)
    const bool win_here = window_id >= 0 && ((first && !(flags & FFT_WINDOW_OUT_DIV)) || (last && (flags & FFT_WINDOW_OUT_DIV)));
    r.win_fixed = (!r.gen && win_here && pass_split_exchange_rt(esz, rp, w, false) && (window_id == 0 || window_id == 2)) ? window_id : -1;
    // plain first / last pass?  (then no option is looked at inside the kernel)
    r.simple = !r.gen && (r.rowmap ? ((flags & (FFT_IN_REAL | BDSP_FFT_SHIFT_IN)) == 0 && !scaled && window_id < 0)
                                   : (!last || (flags & (BDSP_FFT_SHIFT_OUT | BDSP_FFT_MAGNITUDE | FFT_OUT_REAL | FFT_WINDOW_OUT_DIV)) == 0));
    // Non-temporal loads in the FIRST pass of an f64 transform whose tile reads whole 128-byte lines: measurements at launch_pass
    r.ntl = pass_ntl_candidate_rt(esz, w) && first && r.rowmap && !r.gen && !(flags & FFT_IN_REAL);
    r.split = pass_split_exchange_rt(esz, rp, w, r.gen);
    r.lds_twiddles = pass_lds_twiddles_rt(esz, rp, w, r.gen);
    r.lds_bytes = pass_tile_lds_bytes_rt(esz, rp, w, r.gen) + (r.lds_twiddles ? (size_t)rp * (2 * esz) : 0);
    r.threads = w * (rp / 16);
    r.tiles_per_vec = (n / (size_t)rp) / (size_t)w;
    r.grid = r.tiles_per_vec * batch;
    return r;
}

// ---------------------------------------------------------------- a whole transform of n = 2^k > 4096 points
struct FftPlan {
    int passes;        // 0: above 2^30 points; 1: the one-workgroup kernel k_fft_wg4 (no route); 2 or 3 global passes
    FftPassRoute r[3];
};
BDSP_HD FftPlan fft_plan(size_t esz, size_t n, size_t batch, int num_cus, unsigned flags, bool scaled, int window_id,
                         size_t in_stride, size_t out_stride, size_t in_valid, bool inverse)
{
    FftPlan p{};
    if (wg4_takes(esz, n, flags, window_id, in_stride, out_stride, in_valid)) { p.passes = 1; return p; }
    int rp[3], w[3];
    p.passes = plan_passes(n, batch, esz, num_cus, rp, w);
    for (int i = 0; i < p.passes; ++i)
        p.r[i] = fft_pass_route(esz, rp[i], w[i], n, batch, i == 0, i == p.passes - 1, inverse, flags, scaled, window_id,
                                in_stride, out_stride, in_valid);
    return p;
}

// ---------------------------------------------------------------- buffer order of the two-buffer driver (capi.cpp)
// a holds the input, b is scratch of the same size.  n > 4096:
//   a -> b -> a        two passes
//   a -> b -> b        two passes from 2^19 points on when input and output have the same shape: the last pass reads and
//                      writes the same index set per workgroup, so it runs in place (measurements at fft_two_buffers)
//   a -> b -> a -> b   three passes
// (k_fft_wg4 transforms a in place; the plan above says when it runs.)
enum { FFT_BUF_ABA = 0, FFT_BUF_ABB = 1, FFT_BUF_ABAB = 2 };
BDSP_HD int fft_buffer_order(size_t esz, size_t n, unsigned flags)
{
    if (plan_pass_count(n, esz) == 3) return FFT_BUF_ABAB;
    const bool reshaping = (flags & (FFT_IN_REAL | BDSP_FFT_MAGNITUDE | FFT_OUT_REAL)) != 0;
    return (!reshaping && n >= (size_t(1) << 19)) ? FFT_BUF_ABB : FFT_BUF_ABA;
}

// ---------------------------------------------------------------- the facade's operations as transform options
// window ids: facade ids 0..3 (interop/src/lib.rs:153-164, unknown -> rectangular) + 4 = Hann
template <typename T>
BDSP_HD void map_window(int id, int* wid, T* alpha)
{
    *alpha = (T)0.54;
    if (id == 4) { *wid = 1; *alpha = (T)0.5; }
    else if (id >= 0 && id <= 3) *wid = id;
    else *wid = 3;
}

// plain_fft / fft / windowed_fft (time_to_freq.rs:136-176) and plain_ifft / ifft / windowed_ifft
// (freq_to_time.rs:136-177) with the shift, window and 1/N scale fused into the transform:
//   plain_fft      (false, false, -1)        0 (+ FFT_IN_REAL on a real vector)
//   fft            (false, true, -1)         SHIFT_OUT
//   windowed_fft   (false, true, window)     SHIFT_OUT + the window on the input
//   plain_ifft     (true, false, -1)         inverse
//   ifft           (true, true, -1)          inverse, in_scale = 1/points, SHIFT_IN
//   windowed_ifft  (true, true, window)      that + FFT_WINDOW_OUT_DIV
template <typename T>
struct FftOpArgs {
    unsigned flags;
    T in_scale;
    int window_id; // -1 none
    T window_alpha;
};
template <typename T>
BDSP_HD FftOpArgs<T> fft_op_args(bool inverse, bool shift, int window /* facade id, -1 none */, bool real_input, size_t points)
{
    FftOpArgs<T> a{};
    a.flags = real_input ? FFT_IN_REAL : 0u; // real input is zero-interleaved to complex first (:147-150)
    a.window_id = -1;
    a.window_alpha = 0;
    a.in_scale = (T)1;
    if (!inverse) {
        if (window >= 0) map_window<T>(window, &a.window_id, &a.window_alpha);
        if (shift) a.flags |= BDSP_FFT_SHIFT_OUT;
    } else if (shift) {
        // ifft = scale(1/points) -> ifft_shift -> plain_ifft (freq_to_time.rs:160-168)
        a.in_scale = (T)1 / (T)points;
        a.flags |= BDSP_FFT_SHIFT_IN;
        if (window >= 0) { map_window<T>(window, &a.window_id, &a.window_alpha); a.flags |= FFT_WINDOW_OUT_DIV; }
    }
    return a;
}

} // namespace bdsp
