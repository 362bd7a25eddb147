// mat_mul.hip -- the product of two matrices, C (M x N) = A (M x K) . B (K x N) or A . B^H (B: N x K), real or
// complex, f32 or f64: the one dense contraction of the library.  Every matrix is dense and row-major; an element is a
// real scalar or an interleaved (re, im) pair.  A row may start at any element (an f32 row of odd length puts row 1 on a
// 4-byte boundary), so real data move one scalar per access and complex data one pair.
//
// Three paths, chosen by mm_dispatch (mat_mul_core.h) from (M, N, K, form) alone:
//   k_mm_stream  plain form, M <= 16, K <= 64 (few channels -> few beams; memory-bound).  A sits in LDS; a workgroup owns
//                runs of 256 columns of B, one column per thread; the thread reads its K elements of B once, a wave
//                256 / 512 / 1024 contiguous bytes per row of B, keeps all M sums in registers (4, 8 or 16 accumulator
//                rows, the smallest that holds M) and writes its column of C.  B is read once and C written once: 1.00 x
//                the algorithmic bytes, plus A once per workgroup.  Vector ALU.
//   k_mm_tiled   both forms.  A workgroup computes a 64 x 64 tile of C in steps of 32 (f32) or 16 (f64) along K through
//                LDS planes [k][row] / [k][column] of pitch 65, real and imaginary parts in planes of their own.
//                f32: v_mfma_f32_32x32x2_f32, one 32 x 32 quadrant per wave (issue interval = dependent latency = 64
//                cycles, so one chain per wave keeps the pipe full; complex has three).  f64: the vector ALU, a 4 x 4
//                block per thread -- DESIGN.md records the f64 matrix pipe at the vector rate; a v_mfma_f64_16x16x4_f64
//                variant was not built, so its time is "not measured".  One LDS buffer; the elements of step k + 1
//                are loaded into registers before step k is multiplied and written to LDS after it.  Edge tiles are
//                predicated: a lane past an edge stages +0 and stores nothing.
//   split        K >= 256 and at most 64 tiles of C (a Gram matrix of 64 rows x 1M points): k_mm_tiled again with every
//                (chunk of K, tile) pair as one workgroup, writing chunk c's M x N partial to a temporary; then
//                k_mm_split_sum adds the partials in ascending c.  Two launches, whatever the shape.
//
// Order of summation, every path: each element of C (of a partial) is ONE chain over ascending k from +0, one rounding
// per product (fma, or the matrix instruction, which is bit for bit that chain); the split path then adds the chunk sums
// in ascending chunk order.  Complex: four real products on three chains (mm_cplx_step; the real chain of the f32 tiled
// kernel takes its two kinds of product in pairs of k, as the instruction delivers them).  Every element of C and of a
// partial is written by exactly one thread, once, with a plain store; nothing depends on the grid size, the CU count or
// timing, so the same call gives the same bits on every run, and A . A^H is Hermitian to the bit with a diagonal whose
// imaginary part is +0.
//
// No scratch, no stream or device synchronisation.  tests/host_sim/sim_mat_mul.cpp runs the maps of mat_mul_core.h with
// threads as loops.
#include "bdsp_internal.h"
#include "mat_mul_core.h"

namespace bdsp {

template <typename T> struct mm_pair { typedef T type __attribute__((ext_vector_type(2))); };
typedef float mm_f32x16 __attribute__((ext_vector_type(16)));

struct MmFma {
    __device__ __forceinline__ float operator()(float a, float b, float c) const { return __builtin_fmaf(a, b, c); }
    __device__ __forceinline__ double operator()(double a, double b, double c) const { return __builtin_fma(a, b, c); }
};
// D = C + A B for one 32 x 32 quadrant, k = 0 and 1 (lane maps: mat_mul_core.h)
struct MmMfma {
    __device__ __forceinline__ mm_f32x16 operator()(float a, float b, mm_f32x16 c) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#else
        return c;
#endif
    }
};

// ---------------------------------------------------------------------------------------------
// staging: 64 rows (of A, or of B in the transposed form) x TK elements, k-contiguous (ROWS; ld = K), or TK rows of B x
// 64 columns (ld = N).  In two halves, global -> registers and registers -> LDS, so that the next step's loads are in
// flight while this one is multiplied.
// ---------------------------------------------------------------------------------------------
template <typename T, int TK>
struct MmStage {
    T re[TK / 4], im[TK / 4];
};

template <typename T, bool CPLX, int TK, bool ROWS>
__device__ __forceinline__ void mm_stage_load(MmStage<T, TK>& st, const T* __restrict__ src, size_t X, size_t ld, size_t x0,
                                              size_t k0, size_t kend, int tid, bool neg_im)
{
    constexpr int E = CPLX ? 2 : 1;
    using P = typename mm_pair<T>::type;
#pragma unroll
    for (int r = 0; r < TK / 4; ++r) {
        int x, k;
        if (ROWS) mm_stage_kc(tid, r, TK, &x, &k);
        else mm_stage_xc(tid, r, &x, &k);
        const size_t gx = x0 + x, gk = k0 + k;
        st.re[r] = (T)0;
        st.im[r] = (T)0;
        if (gx < X && gk < kend) {
            const T* p = src + (ROWS ? gx * ld + gk : gk * ld + gx) * E;
            if (CPLX) {
                const P v = *reinterpret_cast<const P*>(p);
                st.re[r] = v.x;
                st.im[r] = neg_im ? -v.y : v.y;
            } else st.re[r] = *p;
        }
    }
}

template <typename T, bool CPLX, int TK, bool ROWS>
__device__ __forceinline__ void mm_stage_store(const MmStage<T, TK>& st, T* plane, int tid)
{
    constexpr int PL = mm_plane_elems(TK);
#pragma unroll
    for (int r = 0; r < TK / 4; ++r) {
        int x, k;
        if (ROWS) mm_stage_kc(tid, r, TK, &x, &k);
        else mm_stage_xc(tid, r, &x, &k);
        plane[mm_lds_slot(k, x)] = st.re[r];
        if (CPLX) plane[PL + mm_lds_slot(k, x)] = st.im[r];
    }
}

// both operands of step k0: A always by rows; B by rows with its imaginary part negated (transposed form), else by columns
template <typename T, bool CPLX, bool TRANS, int TK>
__device__ __forceinline__ void mm_load_step(MmStage<T, TK>& sa, MmStage<T, TK>& sb, const T* __restrict__ a,
                                             const T* __restrict__ b, size_t M, size_t N, size_t K, size_t i0, size_t j0,
                                             size_t k0, size_t kend, int tid)
{
    mm_stage_load<T, CPLX, TK, true>(sa, a, M, K, i0, k0, kend, tid, false);
    if (TRANS) mm_stage_load<T, CPLX, TK, true>(sb, b, N, K, j0, k0, kend, tid, true);
    else mm_stage_load<T, CPLX, TK, false>(sb, b, N, N, j0, k0, kend, tid, false);
}
template <typename T, bool CPLX, bool TRANS, int TK>
__device__ __forceinline__ void mm_store_step(const MmStage<T, TK>& sa, const MmStage<T, TK>& sb, T* pA, T* pB, int tid)
{
    mm_stage_store<T, CPLX, TK, true>(sa, pA, tid);
    mm_stage_store<T, CPLX, TK, TRANS>(sb, pB, tid);
}

template <typename T, bool CPLX>
__device__ __forceinline__ void mm_store(T* dst, size_t M, size_t N, size_t row, size_t col, T re, T im)
{
    using P = typename mm_pair<T>::type;
    if (row >= M || col >= N) return;
    if (CPLX) *reinterpret_cast<P*>(dst + (row * N + col) * 2) = P{re, im};
    else dst[row * N + col] = re;
}

// work item w = chunk * ntiles + tile: sums k in [chunk * chunk_len, min(K, (chunk + 1) * chunk_len)) of one 64 x 64
// tile into out + chunk * M * N elements (the tiled path: one chunk, out = C)
template <typename T, bool CPLX, bool TRANS>
__global__ __launch_bounds__(MM_THREADS) void k_mm_tiled(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                                                          size_t M, size_t N, size_t K, size_t tiles_n, size_t ntiles,
                                                          size_t chunk_len, size_t nwork)
{
    constexpr bool DBL = sizeof(T) == 8;
    constexpr int TK = mm_tk(DBL), E = CPLX ? 2 : 1, PL = mm_plane_elems(TK);
    __shared__ T sA[E * PL];
    __shared__ T sB[E * PL];
    const int tid = (int)threadIdx.x;
    for (size_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        size_t chunk, i0, j0;
        mm_work_item(w, ntiles, tiles_n, &chunk, &i0, &j0);
        const size_t kbeg = chunk * chunk_len, kend = K - kbeg < chunk_len ? K : kbeg + chunk_len;
        T* dst = out + chunk * (M * N * E);
        if constexpr (!DBL) {
            const int lane = tid & (MM_LANES - 1), wave = tid / MM_LANES;
            const int ax = mm_wave_row0(wave) + mm_mfma_ab_x(lane), bx = mm_wave_col0(wave) + mm_mfma_ab_x(lane);
            const int kl = mm_mfma_ab_k(lane);
            mm_f32x16 re = {}, ia = {}, ib = {};
            MmStage<T, TK> ra, rb;
            mm_load_step<T, CPLX, TRANS, TK>(ra, rb, a, b, M, N, K, i0, j0, kbeg, kend, tid);
            for (size_t k0 = kbeg; k0 < kend; k0 += TK) {
                mm_store_step<T, CPLX, TRANS, TK>(ra, rb, sA, sB, tid);
                __syncthreads();
                // the next step's elements travel while this one is multiplied (past kend: nothing is loaded)
                mm_load_step<T, CPLX, TRANS, TK>(ra, rb, a, b, M, N, K, i0, j0, k0 + TK, kend, tid);
#pragma unroll
                for (int kk = 0; kk < TK; kk += 2) {
                    const int pa = mm_lds_slot(kk + kl, ax), pb = mm_lds_slot(kk + kl, bx);
                    if (CPLX) mm_cplx_step(sA[pa], sA[PL + pa], sB[pb], sB[PL + pb], &re, &ia, &ib, MmMfma());
                    else re = MmMfma()(sA[pa], sB[pb], re);
                }
                __syncthreads();
            }
#pragma unroll
            for (int g = 0; g < 16; ++g)
                mm_store<T, CPLX>(dst, M, N, i0 + mm_wave_row0(wave) + mm_mfma_c_row(lane, g),
                                  j0 + mm_wave_col0(wave) + mm_mfma_c_col(lane), re[g], ia[g] + ib[g]);
        } else {
            T re[4][4] = {}, ia[4][4] = {}, ib[4][4] = {};
            MmStage<T, TK> ra, rb;
            mm_load_step<T, CPLX, TRANS, TK>(ra, rb, a, b, M, N, K, i0, j0, kbeg, kend, tid);
            for (size_t k0 = kbeg; k0 < kend; k0 += TK) {
                mm_store_step<T, CPLX, TRANS, TK>(ra, rb, sA, sB, tid);
                __syncthreads();
                mm_load_step<T, CPLX, TRANS, TK>(ra, rb, a, b, M, N, K, i0, j0, k0 + TK, kend, tid);
#pragma unroll 4
                for (int kk = 0; kk < TK; ++kk) {
                    T ar[4], ai[4], br[4], bi[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int pa = mm_lds_slot(kk, mm_valu_row(tid, r)), pb = mm_lds_slot(kk, mm_valu_col(tid, r));
                        ar[r] = sA[pa];
                        br[r] = sB[pb];
                        ai[r] = CPLX ? sA[PL + pa] : (T)0;
                        bi[r] = CPLX ? sB[PL + pb] : (T)0;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (CPLX) mm_cplx_step(ar[r], ai[r], br[c], bi[c], &re[r][c], &ia[r][c], &ib[r][c], MmFma());
                            else re[r][c] = MmFma()(ar[r], br[c], re[r][c]);
                        }
                }
                __syncthreads();
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    mm_store<T, CPLX>(dst, M, N, i0 + mm_valu_row(tid, r), j0 + mm_valu_col(tid, c), re[r][c],
                                      ia[r][c] + ib[r][c]);
        }
    }
}

// out[i] = part[0][i] + part[1][i] + ... in ascending chunk order; total scalars per partial
template <typename T>
__global__ __launch_bounds__(MM_THREADS) void k_mm_split_sum(const T* __restrict__ part, T* __restrict__ out, size_t total,
                                                              size_t nchunks)
{
    for (size_t i = (size_t)blockIdx.x * MM_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * MM_THREADS) {
        T s = part[i];
        for (size_t c = 1; c < nchunks; ++c) s += part[c * total + i];
        out[i] = s;
    }
}

// plain form, M <= MB <= 16, K <= 64
template <typename T, bool CPLX, int MB>
__global__ __launch_bounds__(MM_THREADS) void k_mm_stream(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                                                           size_t M, size_t N, size_t K, size_t nruns)
{
    constexpr int E = CPLX ? 2 : 1;
    using P = typename mm_pair<T>::type;
    __shared__ T sa[MM_STREAM_MAX_K * MB * E];
    const int tid = (int)threadIdx.x, kn = (int)K, mn = (int)M;
    for (int idx = tid; idx < kn * MB * E; idx += MM_THREADS) { // idx = mm_stream_slot(m, k, c, MB, E); rows past M: +0
        const int c = idx % E, m = (idx / E) % MB, k = idx / (E * MB);
        sa[idx] = m < mn ? a[((size_t)m * K + k) * E + c] : (T)0;
    }
    __syncthreads();
    for (size_t run = blockIdx.x; run < nruns; run += gridDim.x) {
        const size_t n = run * MM_STREAM_COLS + tid;
        if (n >= N) continue;
        T re[MB], ia[MB], ib[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) re[m] = ia[m] = ib[m] = (T)0;
#pragma unroll 4
        for (int k = 0; k < kn; ++k) {
            const T* p = b + ((size_t)k * N + n) * E;
            T br, bi = (T)0;
            if (CPLX) {
                const P v = *reinterpret_cast<const P*>(p);
                br = v.x;
                bi = v.y;
            } else br = *p;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (CPLX)
                    mm_cplx_step(sa[mm_stream_slot(m, k, 0, MB, E)], sa[mm_stream_slot(m, k, E - 1, MB, E)], br, bi, &re[m],
                                 &ia[m], &ib[m], MmFma());
                else re[m] = MmFma()(sa[mm_stream_slot(m, k, 0, MB, E)], br, re[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < MB; ++m)
            if (m < mn) mm_store<T, CPLX>(out, M, N, (size_t)m, n, re[m], ia[m] + ib[m]);
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
constexpr size_t MM_MAX_GRID = 0x7fffffffu;
// workgroups of the streaming kernel at most: 8 per CU of a 256-CU part, a constant (not measured)
constexpr size_t MM_STREAM_MAX_BLOCKS = 2048;

template <typename T, bool CPLX, bool TRANS>
static int mm_launch_tiled(const T* a, const T* b, T* out, size_t M, size_t N, size_t K, size_t chunk_len, size_t nchunks,
                           hipStream_t s)
{
    const size_t tiles_n = mm_tiles_along(N, MM_TN), ntiles = mm_tiles(M, N), nwork = ntiles * nchunks;
    const size_t blocks = nwork < MM_MAX_GRID ? nwork : MM_MAX_GRID;
    hipLaunchKernelGGL((k_mm_tiled<T, CPLX, TRANS>), dim3((unsigned)blocks), dim3(MM_THREADS), 0, s, a, b, out, M, N, K, tiles_n,
                       ntiles, chunk_len, nwork);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, bool CPLX, int MB>
static int mm_launch_stream(const T* a, const T* b, T* out, size_t M, size_t N, size_t K, hipStream_t s)
{
    const size_t nruns = (N + MM_STREAM_COLS - 1) / MM_STREAM_COLS;
    const size_t blocks = nruns < MM_STREAM_MAX_BLOCKS ? nruns : MM_STREAM_MAX_BLOCKS;
    hipLaunchKernelGGL((k_mm_stream<T, CPLX, MB>), dim3((unsigned)blocks), dim3(MM_THREADS), 0, s, a, b, out, M, N, K, nruns);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, bool CPLX>
static int mm_run(const T* a, const T* b, T* out, size_t M, size_t N, size_t K, bool trans, T* scratch, hipStream_t s)
{
    const MmPath path = mm_dispatch(M, N, K, trans);
    if (path == MM_PATH_STREAM) {
        switch (mm_stream_mb(M)) {
        case 4: return mm_launch_stream<T, CPLX, 4>(a, b, out, M, N, K, s);
        case 8: return mm_launch_stream<T, CPLX, 8>(a, b, out, M, N, K, s);
        default: return mm_launch_stream<T, CPLX, 16>(a, b, out, M, N, K, s);
        }
    }
    const bool split = path == MM_PATH_SPLIT;
    if (split && !scratch) return BDSP_ERR_UNSUPPORTED;
    const size_t chunk_len = split ? mm_split_chunk(M, N, K) : K, nchunks = split ? mm_split_chunks(M, N, K) : 1;
    T* dst = split ? scratch : out;
    if (trans) BDSP_TRY((mm_launch_tiled<T, CPLX, true>(a, b, dst, M, N, K, chunk_len, nchunks, s)));
    else BDSP_TRY((mm_launch_tiled<T, CPLX, false>(a, b, dst, M, N, K, chunk_len, nchunks, s)));
    if (split) {
        const size_t total = M * N * (CPLX ? 2 : 1), want = (total + MM_THREADS - 1) / MM_THREADS;
        const size_t blocks = want < MM_MAX_GRID ? want : MM_MAX_GRID;
        hipLaunchKernelGGL((k_mm_split_sum<T>), dim3((unsigned)blocks), dim3(MM_THREADS), 0, s, scratch, out, total, nchunks);
        BDSP_LAUNCH_CHECK();
    }
    return BDSP_OK;
}

// the temporary the call needs holds this many partials of M * N elements: the chunks of the split path, else 0
size_t mm_scratch_factor(size_t M, size_t N, size_t K, bool trans)
{
    if (!M || !N || !K || mm_dispatch(M, N, K, trans) != MM_PATH_SPLIT) return 0;
    return mm_split_chunks(M, N, K);
}

template <typename T>
int mm_matmul(const T* a, const T* b, T* out, size_t M, size_t N, size_t K, bool is_complex, bool trans, T* scratch, hipStream_t s)
{
    if (!M || !N || !K) return BDSP_OK;
    if (is_complex) return mm_run<T, true>(a, b, out, M, N, K, trans, scratch, s);
    return mm_run<T, false>(a, b, out, M, N, K, trans, scratch, s);
}

template int mm_matmul<float>(const float*, const float*, float*, size_t, size_t, size_t, bool, bool, float*, hipStream_t);
template int mm_matmul<double>(const double*, const double*, double*, size_t, size_t, size_t, bool, bool, double*, hipStream_t);

} // namespace bdsp
