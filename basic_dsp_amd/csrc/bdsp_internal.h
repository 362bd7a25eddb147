// bdsp_internal.h -- shared declarations of libbasic_dsp_hip.so (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/basic_dsp_hip.h"
#include "fft_core.h"
#include "fft_plan_core.h"

namespace bdsp {

// ---------------------------------------------------------------- errors
void set_last_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define BDSP_HIP_TRY(expr)                                                                         \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return ::bdsp::hip_fail(_e, #expr, __FILE__, __LINE__);              \
    } while (0)
#define BDSP_TRY(expr)                                                                             \
    do {                                                                                           \
        int _c = (expr);                                                                           \
        if (_c != BDSP_OK) return _c;                                                              \
    } while (0)
#define BDSP_LAUNCH_CHECK() BDSP_HIP_TRY(hipGetLastError())

// ---------------------------------------------------------------- runtime
// One context per (process, device).  B1/B2 work runs on the library's own non-blocking stream;
// B3 callers pass theirs.  Workspace blocks are cached per stream so that a block freed on one
// stream is never handed to work queued on another.
int device_ready();                       // BDSP_OK or BDSP_ERR_NO_DEVICE
hipStream_t lib_stream();                 // library stream of the current device
// B3 `stream` argument: NULL = the library's own (non-blocking) stream; BDSP_HIP_STREAM_DEFAULT = (void*)1, the value
// of hipStreamLegacy = HIP's null stream, which is what a framework's "default stream" handle 0 means -- a caller
// that forwards such a handle must map 0 to it, or its work would run unordered on the library stream.
inline hipStream_t pick_stream(void* s)
{
    if (!s) return lib_stream();
    if (s == reinterpret_cast<void*>(1)) return nullptr;
    return reinterpret_cast<hipStream_t>(s);
}
int ws_alloc(void** p, size_t bytes, hipStream_t stream);
void ws_free(void* p, hipStream_t stream);
// HIP-graph capture on `stream`: blocks freed between begin and end are not recycled; end hands them to the caller
// (the graph handle), which gives them back with ws_free when the graph is destroyed
int ws_capture_begin(hipStream_t stream);
void ws_capture_end(hipStream_t stream, std::vector<void*>* pinned);
// Streaming store of one complex value (8 or 16 bytes): bypasses the caches' allocation.  For outputs too large for the
// 256 MB Infinity Cache to hold until their reader comes (a 256 MB interpolation result ran 82 -> 69 us).
template <typename C>
__device__ __forceinline__ void nt_store(C* p, C v)
{
    using R = typename real_of<C>::type;
    typedef R vec2 __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store(vec2{v.x, v.y}, reinterpret_cast<vec2*>(p));
}

// Streaming load of one complex value: the first pass of an f64 transform reads its input, dead once read, this way
// (k_fft_pass NTL)
template <typename C>
__device__ __forceinline__ C nt_load(const C* p)
{
    using R = typename real_of<C>::type;
    typedef R vec2 __attribute__((ext_vector_type(2)));
    const vec2 v = __builtin_nontemporal_load(reinterpret_cast<const vec2*>(p));
    return C{v.x, v.y};
}

int num_cus();

// Launch attributes of a kernel on the CURRENT device (runtime.cpp).  kernel_lds: call before every launch with `bytes` of
// dynamic LDS; raises the kernel's limit where bytes > 64 KiB.  kernel_slots: the same, and *per_cu = the resident workgroups
// per CU as the runtime computes them (at least 1), asked once per (device, kernel, threads, lds) -- for persistent grids.
int kernel_lds(const void* kernel, size_t bytes);
int kernel_slots(const void* kernel, int threads, size_t lds, int* per_cu);
template <typename K> int kernel_lds(K* kernel, size_t bytes) { return kernel_lds(reinterpret_cast<const void*>(kernel), bytes); }
template <typename K> int kernel_slots(K* kernel, int threads, size_t lds, int* per_cu) { return kernel_slots(reinterpret_cast<const void*>(kernel), threads, lds, per_cu); }

struct WsBlock { // RAII workspace
    void* p = nullptr;
    hipStream_t s = nullptr;
    int alloc(size_t bytes, hipStream_t stream) { s = stream; return ws_alloc(&p, bytes, stream); }
    ~WsBlock() { if (p) ws_free(p, s); }
    template <typename U> U* as() const { return reinterpret_cast<U*>(p); }
};

// Forward twiddle table exp(-2*pi*i*m/n), m in [0, n), generated on the host in double precision,
// rounded once, cached per (device, n, precision).  n <= 8192.
template <typename T> int twiddle_table(int n, const cpx<T>** table);
template <typename T> bool twiddle_table_available(int n); // cached already, or the cache still has room

// ---------------------------------------------------------------- fused FFT prologue / epilogue
// FftIo and the internal flag bits FFT_IN_REAL / FFT_WINDOW_OUT_DIV / FFT_OUT_REAL: fft_plan_core.h (no HIP call in there)

// ---------------------------------------------------------------- kernel launchers (per .hip TU)
// fft.hip
template <typename T>
int fft_pow2(const FftIo<T>& io, T* scratch_a, T* scratch_b, size_t batch, bool inverse,
             hipStream_t s);
template <typename T> int fft_pow2_passes(size_t n); // 1 (n <= 4096), 2 or 3 trips through memory
// trips of a PLAIN complex transform (no fused option): the same, except where fft_pow2 has a workgroup-resident kernel
// for that case only (f32 8192 points: k_fft_wg4); one predicate for the dispatch and for bdsp_hip_fft_passes
template <typename T> int fft_pow2_plain_trips(size_t n);
template <typename T>
int fft_any(const FftIo<T>& io, size_t batch, bool inverse, hipStream_t s);
bool is_pow2(size_t n);

// conv.hip
template <typename T>
int convolve_overlap_save(const T* in, T* out, size_t points, size_t batch, const T* taps_dev,
                          size_t taps, long long in_off, long long out_off, size_t nblocks_limit,
                          T* last_block_out, const T* h_freq_dev, hipStream_t s);
template <typename T>
int convolve_direct(const T* in, T* out, size_t points, size_t batch, const T* taps_dev,
                    size_t taps, bool is_complex, hipStream_t s);
size_t conv_fft_len(size_t taps);
// block step (valid outputs per 4096-point block) of the kernel conv_run_blocks<T> will use for these taps
template <typename T> size_t conv_block_step(size_t points, size_t taps, bool real_data);
// conv_v2.hip: the second-generation block kernel (complex f32 and f64)
size_t conv_v2_block_step(size_t taps);
bool conv_v2_applies(size_t points, size_t taps);
// shares of the block kernel's dispatch groups in percent (-1: the measured defaults) for the CALLING THREAD's next launches
// (bdsp_hip_dev_convolve_ex sets them around one call)
void conv_v2_set_shares(int first_pct, int second_pct);
template <typename T>
int conv_v2_run(const T* in, T* out, size_t points, size_t batch, const T* hs, size_t taps,
                size_t first_block, size_t nblocks, bool hs_is_taps, hipStream_t s, bool real = false);
template <typename T>
int conv_prepare_spectrum(const T* taps_dev, size_t taps, const T* h_freq_dev, T* hs, hipStream_t s);
template <typename T>
int conv_run_blocks(const T* in, T* out, size_t points, size_t batch, const T* hs, size_t taps,
                    long long in_off, long long out_off, size_t nblocks_limit, T* last_block_out,
                    hipStream_t s, bool real_data = false, bool hs_is_taps = false);
// real_data: in/out are REAL vectors of `points` samples and hs is the spectrum of REAL taps; two real
// blocks share one complex transform pair
// the spectrum handed to conv_run_blocks is UNSCALED; the kernel multiplies by 1/L while it loads it
template <typename T> int mul_bcast(T* z, const T* h, size_t l, size_t nb, T scale, hipStream_t s);
template <typename T>
int scatter_valid(const T* z, T* x, size_t l, size_t skip, size_t step, size_t dst_off, size_t nb,
                  size_t x_points, hipStream_t s);

// elementwise.hip
template <typename T> int ew_real_scale(T* x, size_t len, T f, hipStream_t s);
template <typename T> int ew_real_offset(T* x, size_t len, bool is_complex, T f, hipStream_t s);
template <typename T> int ew_complex_scale(T* x, size_t len, T re, T im, hipStream_t s);
template <typename T> int ew_complex_offset(T* x, size_t len, T re, T im, hipStream_t s);
template <typename T> int ew_binary(T* x, const T* y, size_t len, bool is_complex, int op, hipStream_t s);
template <typename T> int ew_point_table(T* x, size_t len, bool is_complex, const T* table, bool divide, hipStream_t s);
template <typename T> int ew_conj(T* x, size_t len, hipStream_t s);
template <typename T> int ew_mul_cexp(T* x, size_t len, T a, T b, hipStream_t s);
template <typename T> int ew_complex_to_real(const T* x, T* out, size_t len, int kind, hipStream_t s);
template <typename T> int ew_window(T* x, size_t len, bool is_complex, int id, T alpha, bool unapply, hipStream_t s);
template <typename T> int ew_window_rows(T* x, size_t rows, size_t row_len, bool is_complex, int id, T alpha, bool unapply, hipStream_t s);
template <typename T> int ew_fill(T* x, size_t len, T value, hipStream_t s);
template <typename T> int ew_freq_response_rows(T* x, size_t rows, size_t row_len, bool is_complex, int fid, T rolloff, T ratio, bool shifted, hipStream_t s);
template <typename T> int ew_linear_phase(T* x, size_t len, T delay, hipStream_t s);
// spectrum of N points -> dst_points, out of place, one trip (mode 0: periodic repetition = the transform of the
// zero-interleaved vector; mode 1: zero_pad(Center) with the linear phase on the source bin), x the frequency response
// on the destination axis (fid >= 0), x ratio (fid == -1) or nothing (fid == -2); elementwise.hip
template <typename T> int ew_spectrum_resample(const T* in, T* out, size_t src_points, size_t dst_points, int mode, int fid, T rolloff, T ratio, double phase_inc, hipStream_t s);

// reorg.hip
template <typename T> int rg_wrap_copy(const T* in, T* out, size_t points, size_t elem, size_t total, long long start, hipStream_t s);
template <typename T> int rg_zero_interleave(const T* in, T* out, size_t len, size_t elem, size_t factor, hipStream_t s);

// interp.hip
template <typename T>
int interpolatef_dev(const T* in, T* out, size_t len, bool is_complex, int fid, T rolloff, T factor,
                     T delay, size_t conv_len, T delta, hipStream_t s,
                     T (*host_fn)(const void*, T) = nullptr, const void* host_fn_data = nullptr);
template <typename T> size_t interpolatef_new_len(size_t len, T factor);
// what row r of mat_interpolatef_dev takes instead of kernel arguments when every row has a delay of its own: the delay
// (already divided by the matrix's delta) and frac_slow_pairs of it
template <typename T>
struct InterpRowPrm {
    T delay;
    unsigned long long slow_pairs;
};
unsigned long long frac_slow_pairs(size_t conv_len, double delay, int fid, double rolloff); // conv_len as clipped to points / 2
template <typename T>
int mat_interpolatef_dev(const T* in, T* out, size_t rows, size_t row_len, bool is_complex, int fid, T rolloff, T factor,
                         T delay, const InterpRowPrm<T>* prm, size_t conv_len, T delta, hipStream_t s);
template <typename T> int conv_function_taps(T* taps, size_t conv_len, int fid, T rolloff, T ratio, int stride, bool reversed, hipStream_t s);
template <typename T> int conv_function_direct(const T* in, T* out, size_t points, bool is_complex, const T* taps, size_t conv_len, hipStream_t s,
                                                   bool complex_taps = false);
template <typename T> size_t interpolate_real_len(size_t len, T factor);
template <typename T> int interpolate_real_dev(const T* in, T* out, size_t len, T factor, T delay, bool hermite, hipStream_t s);

// reduce.hip: what one walk over a vector accumulates (sums in double; min / max with their keys and indices)
// mixed_radix.hip: lengths 2^a 3^b 5^c 7^d that are not powers of two
template <typename T> bool mr_supported(size_t n);
template <typename T> bool mr_resident(size_t n); // one workgroup-resident transform (may run in place)
template <typename T> int mr_passes(size_t n);    // 1 resident, 2 four-step (result in `out`), 3 Stockham passes (out must be `scratch`)
template <typename T> int mr_fft(const T* in, T* out, T* scratch, size_t n, size_t batch, bool inverse, unsigned flags, T in_scale,
                                 int window_id, T window_alpha, hipStream_t s);

// per-element math family ids (vecmath.hip); the oracle uses the same numbering
enum MathFn {
    MATH_SQRT = 0, MATH_SQUARE, MATH_POWF, MATH_LN, MATH_EXP, MATH_LOG, MATH_EXPF, MATH_SIN, MATH_COS, MATH_TAN,
    MATH_ASIN, MATH_ACOS, MATH_ATAN, MATH_SINH, MATH_COSH, MATH_TANH, MATH_ASINH, MATH_ACOSH, MATH_ATANH, MATH_ABS,
    MATH_WRAP, MATH_EXPF_APPROX, MATH_POWF_APPROX
};
template <typename T> int ew_math(T* x, size_t len, bool is_complex, int fn, T arg, hipStream_t s);
template <typename T> int vm_diff(const T* in, T* out, size_t n_out, size_t step, bool with_start, hipStream_t s);
template <typename T> int vm_complex_split(const T* x, T* a, T* b, size_t points, int kind, hipStream_t s);
template <typename T> int vm_complex_join(T* x, const T* a, const T* b, size_t points, int kind, hipStream_t s);
template <typename T> int vm_split_merge(T* whole, T* const* parts_dev, size_t len, bool is_complex, size_t n, bool merge, hipStream_t s);

struct StatPartial {
    double sr, si, qr, qi;       // sum, sum of squares (complex: z*z, not |z|^2 -- statistics.rs:344)
    double mn_key, mx_key;       // ordering keys: the value (real) or its norm (complex)
    double mnr, mni, mxr, mxi;   // the extreme elements themselves
    unsigned long long imn, imx, cnt;
};
template <typename T>
int red_stats(const T* x, size_t total, size_t buckets, bool is_complex, bool minmax, StatPartial* partials, StatPartial* out, hipStream_t s);
template <typename T>
int red_dot(const T* x, const T* y, size_t count, bool is_complex, StatPartial* partials, StatPartial* out, hipStream_t s);

// mat_reduce.hip -- per-row reductions of a matrix.  `out` (device) receives one result per row (row-major [row][bucket]
// for nb > 1) in the layout `kind` names: the header's Statistics / ComplexStatistics struct in T or double, or one
// (complex) sum / sum of squares in T or double.
enum MrOut { MR_OUT_PARTIAL, MR_OUT_STATS, MR_OUT_STATS_PREC, MR_OUT_SUM, MR_OUT_SUM_PREC, MR_OUT_SUM_SQ, MR_OUT_SUM_SQ_PREC };
struct MrGeom {            // one launch's work: units = rows * nb * chunks
    size_t n;              // elements (scalars, or complex pairs) per row
    size_t stride;         // scalars from one row to the next
    size_t nb;             // buckets of statistics_split (1 = the whole row)
    unsigned chunks;       // workgroups per segment (long rows)
    size_t per;            // elements of a segment per chunk
    size_t units;
    int kind;
    void* out;
};
// statistics / sums of `rows` rows of `n` elements (complex pairs if cplx), element j of bucket j % nb at index j / nb
template <typename T>
int mr_stats(const T* x, size_t rows, size_t n, size_t stride, size_t nb, bool cplx, bool minmax, int kind, void* out,
             hipStream_t s);
// dot products of row r of x with row r of y (ystride scalars apart; 0 = one vector for every row), n elements each
template <typename T>
int mr_dot(const T* x, size_t xstride, const T* y, size_t ystride, size_t rows, size_t n, bool cplx, int kind,
           void* out, hipStream_t s);

// mat_correlate.hip -- cross-correlation of the rows of a matrix with a prepared argument
// every row Surround-padded from p to l elements (complex pairs if is_complex), out of place, one launch
template <typename T> int mc_pad_rows(const T* in, T* out, size_t rows, size_t p, size_t l, bool is_complex, hipStream_t s);
bool mc_fused_len(size_t l); // a power of two in [16, 4096]: mc_correlate_fused applies
// rows x p complex points -> rows x l: pad, transform, x arg (row r at arg + r * arg_stride complex points; 0 = one
// argument for every row), inverse transform, 1/l, swap_halves -- one launch; in and out must not overlap
template <typename T>
int mc_correlate_fused(const T* in, T* out, const T* arg, size_t arg_stride, size_t rows, size_t p, size_t l, hipStream_t s);

// mat_scan.hip -- diff, cum_sum and unwrap of every row of a matrix (a vector is one row); the launch counts do not depend on `rows`
// `rows` rows of row_len scalars -> rows of row_len - step (diff) or row_len (with_start) scalars, dense, out of place
template <typename T> int ms_diff(const T* in, T* out, size_t rows, size_t row_len, size_t step, bool with_start, hipStream_t s);
// in-place prefix sums per row; `scratch`: ms_cum_sum_scratch bytes (0 for rows of at most one scan chunk)
template <typename T> size_t ms_cum_sum_scratch(size_t rows, size_t row_points, bool is_complex);
template <typename T> int ms_cum_sum(T* x, size_t rows, size_t row_points, bool is_complex, void* scratch, hipStream_t s);
// in-place unwrap of every (real) row: one launch
template <typename T> int ms_unwrap(T* x, size_t rows, size_t row_len, T divisor, hipStream_t s);

// mat_resample.hip -- FFT-domain resampling and decimation of every row of a matrix; the launch counts do not depend on
// `rows`
// ew_spectrum_resample for `rows` spectra at once (src_points complex apart in `in`, dst_points apart in `out`), plus
// mode 2 = the crop of interpolate_downsample; mode 1 with dst_points == src_points applies a pure delay; one launch
template <typename T>
int rs_spectrum_rows(const T* in, T* out, size_t rows, size_t src_points, size_t dst_points, int mode, int fid, T rolloff,
                     T ratio, double phase_inc, hipStream_t s);
// out[row][j] = in[row][delay + j * factor] for `rows` rows of `points` elements (elem scalars each) -> out_points
// elements (a vector is one row); one launch
template <typename T>
int rs_decimate_rows(const T* in, T* out, size_t rows, size_t points, size_t out_points, size_t elem, size_t factor,
                     size_t delay, hipStream_t s);
// new_points = f * points with f >= 2 an integer and new_points a power of two in [16, 4096]: rs_fused applies
bool rs_fused_applies(size_t points, size_t new_points);
// rows x points (real scalars if is_real, else complex) -> rows x new_points of the same number space: zero interleave,
// transform, x the multiplier ew_spectrum_resample applies per destination bin (mode 0: interpolatei; mode 1:
// interpolate / interpft with fid, ratio and phase_inc as there), inverse transform, 1/new_points -- one launch; in and
// out must not overlap
template <typename T>
int rs_fused(const T* in, T* out, size_t rows, size_t points, size_t new_points, bool is_real, int mode, int fid,
             T rolloff, T ratio, double phase_inc, hipStream_t s);

// mat_sym.hip -- the index moves of the symmetric real-signal transforms of a matrix; one launch each, whatever `rows`
// rows of 2p - 1 complex bins -> rows of their first p bins, dense, out of place
template <typename T> int sy_crop_rows(const T* in, T* out, size_t rows, size_t p, hipStream_t s);
// rows of p complex bins -> rows of 2p - 1: h(j) = (scaled ? scale : 1) * in[(j + rot) mod p], out[g] = g < p ? h(g) :
// conj(h(2p - 1 - g)), out of place; rot < p.  flag (device, zeroed by the caller; may be null): set to 1 if h(0) of any
// row fails sy_first_bin_fails (mat_sym_core.h)
template <typename T>
int sy_mirror_rows(const T* in, T* out, size_t rows, size_t p, size_t rot, bool scaled, T scale, unsigned* flag, hipStream_t s);

// mat_interp.hip -- time-domain convolution with a weight table and real-row interpolation of every row of a matrix; one
// launch each, whatever `rows`
// out[r][i] = sum_{k=0}^{2 conv_len} in[r][(i - conv_len + k) mod points] * taps[k] for `rows` rows of `points` elements
// (complex pairs if is_complex); taps: 2 conv_len + 1 weights in window order, (re, im) pairs if complex_taps (complex
// rows only); conv_len <= points; out of place
template <typename T>
int mt_conv_direct(const T* in, T* out, size_t rows, size_t points, bool is_complex, const T* taps, size_t conv_len,
                   bool complex_taps, hipStream_t s);
// interpolate_real_dev for `rows` real rows of `len` scalars -> rows of interpolate_real_len(len, factor), dense, out of
// place, bit-equal to the vector kernels
template <typename T>
int mt_interpolate_real(const T* in, T* out, size_t rows, size_t len, T factor, T delay, bool hermite, hipStream_t s);

// mat_ew.hip -- the row-aware elementwise operations of a matrix (a vector is one row); one launch each, whatever `rows`
// z[r][k] *= exp(j (a k + b)) for `rows` rows of `points` complex points, k from 0 in every row; in place
template <typename T> int mw_cexp(T* x, size_t rows, size_t points, double a, double b, hipStream_t s);
// out[r][i] = in[r][points - 1 - i] in elements (complex pairs if is_complex); out of place
template <typename T> int mw_reverse(const T* in, T* out, size_t rows, size_t points, bool is_complex, hipStream_t s);
// x[r][i] (.)= y[r * ystride + i mod ypoints] in elements, op 0 .. 3 = add, sub, mul, div (elementary.rs:591-640);
// ystride 0: one operand for every row; ypoints must divide points (else BDSP_ERR_ARG_LENGTH); in place
template <typename T>
int mw_smaller(T* x, const T* y, size_t rows, size_t points, size_t ypoints, size_t ystride, bool is_complex, int op,
               hipStream_t s);

// mat_frame.hip -- vector <-> matrix moves and the index moves of the rows; one launch each, whatever `rows`; sizes in
// elements (complex pairs if is_complex), everything out of place, bit-exact
// out[r][j] = x[r * hop + j], zero at or past `points`; out: rows x frame_points
template <typename T>
int mf_from_frames(const T* x, T* out, size_t points, size_t rows, size_t frame_points, size_t hop, bool is_complex,
                   hipStream_t s);
// y[i] = sum of m[r][i - r * hop] over the rows that reach i, ascending r, from +0; y: (rows - 1) * hop + frame_points
template <typename T>
int mf_overlap_add(const T* m, T* y, size_t rows, size_t frame_points, size_t hop, bool is_complex, hipStream_t s);
// out[r] = vectors[r] (a DEVICE table of `rows` device pointers to `points` elements each)
template <typename T>
int mf_from_vectors(const T* const* vectors, T* out, size_t rows, size_t points, bool is_complex, hipStream_t s);
// every row zero-padded (option 0 End, 1 Surround, else Center: mat_frame_core.h); BDSP_ERR_ARG_LENGTH unless points > points_before
template <typename T>
int mf_zero_pad(const T* in, T* out, size_t rows, size_t points_before, size_t points, bool is_complex, int option,
                hipStream_t s);
// every row rotated: out[r][i] = in[r][(i + shift) mod points]
template <typename T>
int mf_rotate(const T* in, T* out, size_t rows, size_t points, size_t shift, bool is_complex, hipStream_t s);

// mat_transpose.hip -- src: R rows of C elements (complex pairs if is_complex) -> dst: C rows of R elements, out of place
// (BDSP_ERR_UNSUPPORTED if src == dst), bit-exact, one launch; a row may start at any element
template <typename T>
int tp_transpose(const T* src, T* dst, size_t R, size_t C, bool is_complex, hipStream_t s);

// mat_mul.hip -- out (M x N, dense) = a (M x K) . b (K x N), or a . b^H with b N x K if `trans`; elements are complex
// pairs if is_complex; the path is mm_dispatch's (mat_mul_core.h).  scratch: mm_scratch_factor(M, N, K, trans) * M * N
// elements (0 unless the split path runs: one launch, or two there).  out must not overlap a or b; a may be b
size_t mm_scratch_factor(size_t M, size_t N, size_t K, bool trans);
template <typename T>
int mm_matmul(const T* a, const T* b, T* out, size_t M, size_t N, size_t K, bool is_complex, bool trans, T* scratch,
              hipStream_t s);

// mat_chol.hip -- out (N x N, dense) = the lower Cholesky factor of a (only a's lower triangle and the real part of its
// diagonal are read; loading is added to the diagonal as it is read); *flag (a zeroed device word) is non-zero afterwards
// if a pivot was <= 0 or not finite.  scratch: la_chol_scratch(N) elements.  la_cholesky_solve: x (N x P) from the factor
// l and b (N x P), part as LaPart (mat_chol_core.h); scratch: la_solve_scratch(N, P, part) elements.  x overlaps nothing
size_t la_chol_scratch(size_t N);
size_t la_solve_scratch(size_t N, size_t P, int part);
template <typename T>
int la_cholesky(const T* a, T* out, size_t N, bool is_complex, T loading, T* scratch, unsigned* flag, hipStream_t s);
template <typename T>
int la_cholesky_solve(const T* l, const T* b, T* x, size_t N, size_t P, bool is_complex, int part, T* scratch, hipStream_t s);

// mat_eigh.hip -- w (N scalars, ascending) and v (N x N, row k the k-th eigenvector conjugate-transposed) of the Hermitian
// matrix a (only a's lower triangle and the real part of its diagonal are read).  scratch: je_scratch(N) elements; thr: one
// device scalar; counts: je_count_words(N) device words; host_counts: as many host words.  *sweeps: the sweeps taken, or
// JE_STATUS_NOT_FINITE / JE_STATUS_NOT_CONVERGED (mat_eigh_core.h), after which w and v hold nothing.  Synchronises: once on
// the small path, once per outer sweep on the blocked one
size_t je_scratch(size_t N);
size_t je_count_words(size_t N);
template <typename T>
int je_eigh(const T* a, T* w, T* v, size_t N, bool is_complex, T* scratch, T* thr, unsigned* counts, unsigned* host_counts,
            unsigned* sweeps, hipStream_t s);

// bluestein.hip
template <typename T> int bs_chirp(T* c, size_t n, bool inverse, hipStream_t s);
template <typename T> int bs_kernel(const T* c, T* b, size_t n, size_t m, hipStream_t s);
template <typename T> int bs_fused(const T* x, T* y, const T* c, const T* bspec, size_t n, size_t m, size_t batch, hipStream_t s);
template <typename T>
int bs_pre(const T* x, T* a, const T* c, size_t n, size_t m, size_t batch, bool in_real, T in_scale, size_t rot,
           int window_id, T alpha, hipStream_t s);
template <typename T>
int bs_post(const T* conv, T* out, const T* c, size_t n, size_t m, size_t batch, int out_kind, size_t rot,
            int div_window_id, T alpha, hipStream_t s);

// iir.hip -- S second-order sections along every row of rows x n points, in place (iir_core.h); tab, m (the cascade's
// transition over one tile) and carry (iir_carry_doubles doubles) are device buffers, m and carry only for rows longer than
// a tile; state (may be null): rows x 2S points, read and overwritten.  One launch or three, whatever the row count
template <typename T> struct IirSec;
size_t iir_carry_doubles(size_t rows, size_t n, bool is_complex, size_t S);
template <typename T>
int iir_sosfilt(T* data, size_t rows, size_t n, bool is_complex, const IirSec<T>* tab, size_t S, T* state, const double* m,
                double* carry, hipStream_t s);

// rank_filter.hip -- the element of rank `rank` of the window guard < |d| <= half (guard < 0: |d| <= half) around every point
// of rows x n real values, from `in` to `out` (two buffers), in IEEE totalOrder on the bit patterns (rank_filter_core.h);
// the arguments are valid (rank_args_valid) and half <= RANK_MAX_HALF.  One launch, whatever the row count
template <typename T>
int rank_filter_rows(const T* in, T* out, size_t rows, size_t n, size_t half, size_t rank, int64_t guard, int boundary, hipStream_t s);

// detect.hip -- the cells of rows x n real values that are above the threshold of `kind` and strict local maxima of `order`
// (detect_core.h), compacted in row-major order: row_count[row] detections per row, index and value of the first `capacity`
// (none, and one launch less, where capacity == 0).  rows, n > 0, the arguments are valid (detect_args_valid) and
// order <= DETECT_MAX_ORDER; all pointers but x's threshold of another kind are device memory.  Four launches, whatever the
// row count
template <typename T>
int detect_rows(const T* x, size_t rows, size_t n, int kind, double t, const double* t_rows, const T* t_cells, size_t t_stride,
                size_t order, int boundary, size_t capacity, int64_t* tile_ws, int64_t* row_count, int64_t* row_off,
                int64_t* index, T* value, hipStream_t s);

// sort.hip -- every row of rows x n real values in IEEE totalOrder on the bit patterns (descending: the ascending order of the
// complemented keys), sort_core.h; rows, n > 0 and sort_supported(rows, n).  sort_rows: between data and buf, the result in buf
// iff *in_buf; 1 + P launches, P = ceil(log2(ceil(n / SORT_TILE))).  sort_select_rows: x is not modified; (key, u32 index)
// pairs travel in ws_a and ws_b (sort_select_ws_bytes each; ws_b only where a row is more than one tile), index and value
// (device, rows x count entries, each may be null) receive the elements of the sorted ranks `ranks` (device, count values
// below n; null: 0 .. count - 1); 2 + P launches, whatever the row count
template <typename T> int sort_rows(T* data, T* buf, size_t rows, size_t n, bool descending, bool* in_buf, hipStream_t s);
size_t sort_select_ws_bytes(size_t rows, size_t n, size_t key_bytes);
template <typename T>
int sort_select_rows(const T* x, size_t rows, size_t n, bool descending, size_t count, const uint64_t* ranks, void* ws_a, void* ws_b,
                     int64_t* index, T* value, hipStream_t s);

// zoom_fft.hip -- chirp-z transform of a band: rows x n points -> rows x bins complex, l = zf_conv_len(n, bins)
// (zoom_fft_core.h); the launch counts do not depend on `rows`
// the three tables of a plan: pre (n), post (bins) and the wrapped kernel (l, not yet transformed); start reduced modulo
// 1 and step modulo 2 by the caller; one launch
template <typename T>
int zf_tables(T* pre, T* post, T* kern, size_t n, size_t bins, size_t l, double start, double step, hipStream_t s);
// l in {512, 1024, 2048, 4096}: the whole transform in one launch; x (real scalars if in_real) and y must not overlap;
// starts: null, or one start per row (device, reduced modulo 1) on top of a pre table built with start 0
template <typename T>
int zf_fused(const T* x, T* y, const T* pre, const T* post, const T* kspec, const double* starts, size_t n, size_t bins,
             size_t l, size_t rows, bool in_real, hipStream_t s);
// larger l: x -> rows x l complex (chirped, zero filled), and rows x l complex -> rows x bins (post-chirp, crop)
template <typename T>
int zf_pre(const T* x, T* a, const T* pre, const double* starts, size_t n, size_t l, size_t rows, bool in_real, hipStream_t s);
template <typename T> int zf_post(const T* conv, T* out, const T* post, size_t bins, size_t l, size_t rows, hipStream_t s);

// window value shared by fft.hip and elementwise.hip (device) -- defined inline in window.h
} // namespace bdsp
