// mat_chol.hip -- the Cholesky factorisation A = L L^H of a Hermitian positive-definite N x N matrix (real symmetric or
// complex Hermitian, f32 or f64) and the triangular solves L X = B, L^H X = B and both with an N x P right-hand side.
// Every matrix is dense and row-major; an element is a real scalar or an interleaved (re, im) pair; a row may start at
// any element, so real data move one scalar per access and complex data one pair.
//
// Two paths, chosen by la_dispatch (mat_chol_core.h) from N alone:
//   small (N <= 64)  cholesky: ONE launch of k_la_panel, one workgroup, the lower triangle in LDS, factored column by
//                    column (right-looking; two barriers per column).  cholesky_solve: ONE launch of k_la_trsolve per
//                    triangular pass: L's triangle in LDS, read as broadcasts; a thread owns a column of B, holds its N
//                    unknowns in registers (8, 16, 32 or 64 of them, the smallest that holds N), walks down the rows
//                    (forward) or up (backward); a wave reads 256 / 512 / 1024 contiguous bytes per row; B is read once
//                    and X written once.
//   blocked          blocks of 64.  Factorisation, per block column: k_la_update (form 0) writes the column minus the
//                    product of the blocks to its left, C - A B^H, to a temporary (64 x 64 tiles through LDS as in
//                    k_mm_tiled: v_mfma_f32_32x32x2_f32 for f32, a 4 x 4 block per thread on the vector ALU for f64),
//                    with the accumulator STARTING at C, so the chain of every element is the small path's; then
//                    k_la_panel with one workgroup per 64 rows below the diagonal block: each factors the diagonal block
//                    for itself (the same bits in all of them) and carries its rows along.  2 nb - 1 launches.  Solve,
//                    per block row: k_la_update (form 1: C - A B; form 2, backward: C - A^H B) into a temporary, then
//                    k_la_trsolve on the 64 rows over all columns.  2 nb - 1 launches per pass, whatever P.
//
// Every element of L and of X is written by exactly one thread, once, with a plain store; what a launch wrote is read
// by later launches only.  Plain loads and stores only, no scratch, no index or bound that depends on matrix data: a
// failed pivot (<= 0 or not finite) lets NaN flow on and is reported through one flag word that workgroup 0 of every
// panel launch ORs into with a plain load and store (launches of one stream are ordered).
// tests/host_sim/sim_mat_chol.cpp runs the templates of mat_chol_core.h with threads as loops.
#include <type_traits>

#include "bdsp_internal.h"
#include "mat_chol_core.h"

namespace bdsp {

template <typename T> struct la_pair { typedef T type __attribute__((ext_vector_type(2))); };
typedef float la_f32x16 __attribute__((ext_vector_type(16)));

// raw-pointer accessor of the core templates: scalars, and the (re, im) pair of a complex element in one access
template <typename T>
struct LaRaw {
    T* p;
    using V = typename std::remove_const<T>::type;
    using P = typename la_pair<V>::type;
    __device__ __forceinline__ V ld(size_t i) const { return p[i]; }
    __device__ __forceinline__ void st(size_t i, V v) const { p[i] = v; }
    __device__ __forceinline__ void ld2(size_t i, V* re, V* im) const
    {
        const P v = *reinterpret_cast<const P*>(p + i);
        *re = v.x;
        *im = v.y;
    }
    __device__ __forceinline__ void st2(size_t i, V re, V im) const { *reinterpret_cast<P*>(p + i) = P{re, im}; }
};

extern __shared__ __align__(16) unsigned char la_smem[];

// ---------------------------------------------------------------------------------------------
// the panel kernel: src is element (c0, c0) of the caller's matrix (masked, ld = N) or of the updated block column
// (ld = 64); out is element (c0, c0) of L.  n: order of the diagonal block; rows_below: rows under it (0: one workgroup
// that only factors).  Workgroup b carries rows n + 64 b ... of the panel.
// ---------------------------------------------------------------------------------------------
template <typename T, bool CPLX>
__global__ __launch_bounds__(LA_THREADS) void k_la_panel(const T* __restrict__ src, size_t ld_src, int masked, T loading,
                                                          T* __restrict__ out, size_t ld_out, int n, size_t rows_below,
                                                          unsigned* flag)
{
    const LaPanelLds<T, CPLX, LaRaw<T>> l{{reinterpret_cast<T*>(la_smem)}};
    const int tid = (int)threadIdx.x;
    const size_t sub0 = (size_t)n + (size_t)LA_BLOCK * blockIdx.x, left = rows_below - (size_t)LA_BLOCK * blockIdx.x;
    const int m = rows_below ? (int)(left < (size_t)LA_BLOCK ? left : (size_t)LA_BLOCK) : 0;
    la_panel_load<T, CPLX>(l, LaRaw<const T>{src}, ld_src, n, m, sub0, masked != 0, loading, tid);
    __syncthreads();
    unsigned bad = 0;
    for (int c = 0; c < n; ++c) {
        bad |= la_panel_scale<T, CPLX>(l, c, n, m, tid);
        __syncthreads();
        la_panel_update<T, CPLX>(l, c, n, m, tid);
        __syncthreads();
    }
    la_panel_store<T, CPLX>(l, LaRaw<T>{out}, ld_out, n, m, sub0, blockIdx.x == 0, tid);
    if (blockIdx.x == 0 && tid == 0) *flag = *flag | bad;
}

// ---------------------------------------------------------------------------------------------
// the diagonal solve: l is element (r0, r0) of L (ld = N), src / dst the block's first row of B / X (ld = P)
// ---------------------------------------------------------------------------------------------
template <typename T, bool CPLX, int NB, bool BACK>
__global__ __launch_bounds__(LA_THREADS) void k_la_trsolve(const T* __restrict__ l, size_t ldl, const T* __restrict__ src,
                                                            T* __restrict__ dst, size_t P, int n, size_t nruns)
{
    __shared__ T sl[NB * (NB + 1) / 2 * (CPLX ? 2 : 1)];
    const int tid = (int)threadIdx.x;
    const LaRaw<T> s{sl};
    la_solve_load_l<T, CPLX, NB>(s, LaRaw<const T>{l}, ldl, n, tid);
    __syncthreads();
    for (size_t run = blockIdx.x; run < nruns; run += gridDim.x) {
        // L is read from LDS again in every trip: lifted out of the loop, its 2080 elements would not fit the registers
        __asm__ volatile("" ::: "memory");
        const size_t col = run * LA_SOLVE_COLS + tid;
        if (col < P) la_solve_column<T, CPLX, NB, BACK>(s, LaRaw<const T>{src}, LaRaw<T>{dst}, P, n, col);
    }
}

// ---------------------------------------------------------------------------------------------
// the update kernel: D (M x NN, ld ldd) = C - A' B' over k < K, one 64 x 64 tile per workgroup, LDS planes and lane maps
// of mat_mul_core.h.  The accumulator starts at C and every product enters negated through A, so an element is ONE chain.
//   FORM 0 (factorisation)  A'[x][k] = a[x lda + k], B'[k][y] = conj(b[y ldb + k]); C is the caller's matrix from its
//                           diagonal on: only row >= col is read, of the diagonal re + loading
//   FORM 1 (forward)        A'[x][k] = a[x lda + k], B'[k][y] = b[k ldb + y]
//   FORM 2 (backward)       A'[x][k] = conj(a[k lda + x]), B'[k][y] = b[k ldb + y]
// ---------------------------------------------------------------------------------------------
struct LaFma {
    __device__ __forceinline__ float operator()(float a, float b, float c) const { return __builtin_fmaf(a, b, c); }
    __device__ __forceinline__ double operator()(double a, double b, double c) const { return __builtin_fma(a, b, c); }
};
struct LaMfma {
    __device__ __forceinline__ la_f32x16 operator()(float a, float b, la_f32x16 c) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#else
        return c;
#endif
    }
};

// (re, im) += (ar, ai) (br, bi): four real products on two chains
template <typename S, typename A, typename F>
__device__ __forceinline__ void la_cplx_acc(S ar, S ai, S br, S bi, A* re, A* im, F fma3)
{
    *re = fma3(ar, br, *re);
    *re = fma3(-ai, bi, *re);
    *im = fma3(ar, bi, *im);
    *im = fma3(ai, br, *im);
}

template <typename T, int TK>
struct LaStage {
    T re[TK / 4], im[TK / 4];
};

// 64 x TK elements of one operand: KC, k-contiguous (element (x, k) at x ld + k), else x-contiguous (k ld + x)
template <typename T, bool CPLX, int TK, bool KC>
__device__ __forceinline__ void la_stage_load(LaStage<T, TK>& st, const T* __restrict__ src, size_t X, size_t ld, size_t x0,
                                              size_t k0, size_t K, int tid, bool neg_re, bool neg_im)
{
    constexpr int E = CPLX ? 2 : 1;
    using P = typename la_pair<T>::type;
#pragma unroll
    for (int r = 0; r < TK / 4; ++r) {
        int x, k;
        if (KC) mm_stage_kc(tid, r, TK, &x, &k);
        else mm_stage_xc(tid, r, &x, &k);
        const size_t gx = x0 + x, gk = k0 + k;
        st.re[r] = (T)0;
        st.im[r] = (T)0;
        if (gx < X && gk < K) {
            const T* p = src + (KC ? gx * ld + gk : gk * ld + gx) * E;
            T re, im = (T)0;
            if (CPLX) {
                const P v = *reinterpret_cast<const P*>(p);
                re = v.x;
                im = v.y;
            } else re = *p;
            st.re[r] = neg_re ? -re : re;
            st.im[r] = neg_im ? -im : im;
        }
    }
}

template <typename T, bool CPLX, int TK, bool KC>
__device__ __forceinline__ void la_stage_store(const LaStage<T, TK>& st, T* plane, int tid)
{
    constexpr int PL = mm_plane_elems(TK);
#pragma unroll
    for (int r = 0; r < TK / 4; ++r) {
        int x, k;
        if (KC) mm_stage_kc(tid, r, TK, &x, &k);
        else mm_stage_xc(tid, r, &x, &k);
        plane[mm_lds_slot(k, x)] = st.re[r];
        if (CPLX) plane[PL + mm_lds_slot(k, x)] = st.im[r];
    }
}

template <typename T, bool CPLX, int FORM, int TK>
__device__ __forceinline__ void la_load_step(LaStage<T, TK>& sa, LaStage<T, TK>& sb, const T* __restrict__ a, size_t lda,
                                             const T* __restrict__ b, size_t ldb, size_t M, size_t NN, size_t K, size_t i0,
                                             size_t j0, size_t k0, int tid)
{
    // A enters negated: -a (forms 0, 1), -conj(a) (form 2); B: conj(b) (form 0), b (forms 1, 2)
    la_stage_load<T, CPLX, TK, FORM != 2>(sa, a, M, lda, i0, k0, K, tid, true, FORM != 2);
    la_stage_load<T, CPLX, TK, FORM == 0>(sb, b, NN, ldb, j0, k0, K, tid, false, FORM == 0);
}

// the chain's first value: element (row, col) of C; past an edge +0
template <typename T, bool CPLX, int FORM>
__device__ __forceinline__ void la_c_load(const T* __restrict__ c, size_t ldc, size_t M, size_t NN, size_t row, size_t col,
                                          T loading, T* re, T* im)
{
    using P = typename la_pair<T>::type;
    *re = (T)0;
    *im = (T)0;
    if (row >= M || col >= NN) return;
    if (FORM == 0 && col > row) return;
    const T* p = c + (row * ldc + col) * (CPLX ? 2 : 1);
    if (FORM == 0 && col == row) {
        *re = *p + loading;
        return;
    }
    if (CPLX) {
        const P v = *reinterpret_cast<const P*>(p);
        *re = v.x;
        *im = v.y;
    } else *re = *p;
}

template <typename T, bool CPLX>
__device__ __forceinline__ void la_d_store(T* dst, size_t ldd, size_t M, size_t NN, size_t row, size_t col, T re, T im)
{
    using P = typename la_pair<T>::type;
    if (row >= M || col >= NN) return;
    if (CPLX) *reinterpret_cast<P*>(dst + (row * ldd + col) * 2) = P{re, im};
    else dst[row * ldd + col] = re;
}

template <typename T, bool CPLX, int FORM>
__global__ __launch_bounds__(MM_THREADS) void k_la_update(const T* __restrict__ c, size_t ldc, const T* __restrict__ a, size_t lda,
                                                           const T* __restrict__ b, size_t ldb, T* __restrict__ d, size_t ldd,
                                                           size_t M, size_t NN, size_t K, size_t tiles_n, T loading)
{
    constexpr bool DBL = sizeof(T) == 8;
    constexpr int TK = mm_tk(DBL), E = CPLX ? 2 : 1, PL = mm_plane_elems(TK);
    __shared__ T sA[E * PL];
    __shared__ T sB[E * PL];
    const int tid = (int)threadIdx.x;
    const size_t i0 = (blockIdx.x / tiles_n) * (size_t)MM_TM, j0 = (blockIdx.x % tiles_n) * (size_t)MM_TN;
    LaStage<T, TK> ra, rb;
    la_load_step<T, CPLX, FORM, TK>(ra, rb, a, lda, b, ldb, M, NN, K, i0, j0, 0, tid);
    if constexpr (!DBL) {
        const int lane = tid & (MM_LANES - 1), wave = tid / MM_LANES;
        const int ax = mm_wave_row0(wave) + mm_mfma_ab_x(lane), bx = mm_wave_col0(wave) + mm_mfma_ab_x(lane);
        const int kl = mm_mfma_ab_k(lane);
        la_f32x16 re, im;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            T r, i;
            la_c_load<T, CPLX, FORM>(c, ldc, M, NN, i0 + mm_wave_row0(wave) + mm_mfma_c_row(lane, g),
                                     j0 + mm_wave_col0(wave) + mm_mfma_c_col(lane), loading, &r, &i);
            re[g] = r;
            im[g] = i;
        }
        for (size_t k0 = 0; k0 < K; k0 += TK) {
            la_stage_store<T, CPLX, TK, FORM != 2>(ra, sA, tid);
            la_stage_store<T, CPLX, TK, FORM == 0>(rb, sB, tid);
            __syncthreads();
            la_load_step<T, CPLX, FORM, TK>(ra, rb, a, lda, b, ldb, M, NN, K, i0, j0, k0 + TK, tid);
#pragma unroll
            for (int kk = 0; kk < TK; kk += 2) {
                const int pa = mm_lds_slot(kk + kl, ax), pb = mm_lds_slot(kk + kl, bx);
                if (CPLX) la_cplx_acc(sA[pa], sA[PL + pa], sB[pb], sB[PL + pb], &re, &im, LaMfma());
                else re = LaMfma()(sA[pa], sB[pb], re);
            }
            __syncthreads();
        }
#pragma unroll
        for (int g = 0; g < 16; ++g)
            la_d_store<T, CPLX>(d, ldd, M, NN, i0 + mm_wave_row0(wave) + mm_mfma_c_row(lane, g),
                                j0 + mm_wave_col0(wave) + mm_mfma_c_col(lane), re[g], im[g]);
    } else {
        T re[4][4], im[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
                la_c_load<T, CPLX, FORM>(c, ldc, M, NN, i0 + mm_valu_row(tid, r), j0 + mm_valu_col(tid, cc), loading, &re[r][cc],
                                         &im[r][cc]);
        for (size_t k0 = 0; k0 < K; k0 += TK) {
            la_stage_store<T, CPLX, TK, FORM != 2>(ra, sA, tid);
            la_stage_store<T, CPLX, TK, FORM == 0>(rb, sB, tid);
            __syncthreads();
            la_load_step<T, CPLX, FORM, TK>(ra, rb, a, lda, b, ldb, M, NN, K, i0, j0, k0 + TK, tid);
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
                    for (int cc = 0; cc < 4; ++cc) {
                        if (CPLX) la_cplx_acc(ar[r], ai[r], br[cc], bi[cc], &re[r][cc], &im[r][cc], LaFma());
                        else re[r][cc] = LaFma()(ar[r], br[cc], re[r][cc]);
                    }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
                la_d_store<T, CPLX>(d, ldd, M, NN, i0 + mm_valu_row(tid, r), j0 + mm_valu_col(tid, cc), re[r][cc], im[r][cc]);
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
constexpr size_t LA_MAX_GRID = 0x7fffffffu;

template <typename T, bool CPLX>
static int la_launch_panel(const T* src, size_t ld_src, bool masked, T loading, T* out, size_t ld_out, size_t n, size_t rows_below,
                           unsigned* flag, hipStream_t s)
{
    const size_t lds = sizeof(T) * la_panel_lds_scalars(CPLX, rows_below != 0);
    const size_t blocks = rows_below ? (rows_below + LA_BLOCK - 1) / LA_BLOCK : 1;
    auto kern = k_la_panel<T, CPLX>;
    BDSP_TRY(kernel_lds(kern, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(LA_THREADS), lds, s, src, ld_src, masked ? 1 : 0, loading, out, ld_out,
                       (int)n, rows_below, flag);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, bool CPLX, int FORM>
static int la_launch_update(const T* c, size_t ldc, const T* a, size_t lda, const T* b, size_t ldb, T* d, size_t ldd, size_t M,
                            size_t NN, size_t K, T loading, hipStream_t s)
{
    const size_t tiles_n = mm_tiles_along(NN, MM_TN), tiles = mm_tiles_along(M, MM_TM) * tiles_n;
    if (tiles > LA_MAX_GRID) { set_last_error("cholesky_solve: too many columns for one launch"); return BDSP_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL((k_la_update<T, CPLX, FORM>), dim3((unsigned)tiles), dim3(MM_THREADS), 0, s, c, ldc, a, lda, b, ldb, d, ldd,
                       M, NN, K, tiles_n, loading);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, bool CPLX, int NB, bool BACK>
static int la_launch_trsolve_nb(const T* l, size_t ldl, const T* src, T* dst, size_t P, size_t n, hipStream_t s)
{
    const size_t nruns = (P + LA_SOLVE_COLS - 1) / LA_SOLVE_COLS;
    const size_t blocks = nruns < LA_SOLVE_MAX_BLOCKS ? nruns : LA_SOLVE_MAX_BLOCKS;
    hipLaunchKernelGGL((k_la_trsolve<T, CPLX, NB, BACK>), dim3((unsigned)blocks), dim3(LA_THREADS), 0, s, l, ldl, src, dst, P, (int)n,
                       nruns);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T, bool CPLX, bool BACK>
static int la_launch_trsolve(const T* l, size_t ldl, const T* src, T* dst, size_t P, size_t n, hipStream_t s)
{
    switch (la_solve_nb(n)) {
    case 8: return la_launch_trsolve_nb<T, CPLX, 8, BACK>(l, ldl, src, dst, P, n, s);
    case 16: return la_launch_trsolve_nb<T, CPLX, 16, BACK>(l, ldl, src, dst, P, n, s);
    case 32: return la_launch_trsolve_nb<T, CPLX, 32, BACK>(l, ldl, src, dst, P, n, s);
    default: return la_launch_trsolve_nb<T, CPLX, 64, BACK>(l, ldl, src, dst, P, n, s);
    }
}

template <typename T, bool CPLX>
static int la_chol_run(const T* a, T* out, size_t N, T loading, T* scratch, unsigned* flag, hipStream_t s)
{
    constexpr size_t E = CPLX ? 2 : 1;
    if (la_dispatch(N) == LA_PATH_SMALL) return la_launch_panel<T, CPLX>(a, N, true, loading, out, N, N, 0, flag, s);
    if (!scratch) return BDSP_ERR_UNSUPPORTED;
    for (size_t c0 = 0; c0 < N; c0 += LA_BLOCK) {
        const size_t n = N - c0 < (size_t)LA_BLOCK ? N - c0 : (size_t)LA_BLOCK, below = N - c0 - n;
        T* dst = out + (c0 * N + c0) * E;
        if (c0 == 0) {
            BDSP_TRY((la_launch_panel<T, CPLX>(a, N, true, loading, dst, N, n, below, flag, s)));
            continue;
        }
        const T* left = out + c0 * N * E; // rows c0 ..., columns 0 .. c0 - 1 of L
        BDSP_TRY((la_launch_update<T, CPLX, 0>(a + (c0 * N + c0) * E, N, left, N, left, N, scratch, LA_BLOCK, N - c0, n, c0, loading, s)));
        BDSP_TRY((la_launch_panel<T, CPLX>(scratch, LA_BLOCK, false, (T)0, dst, N, n, below, flag, s)));
    }
    return BDSP_OK;
}

// one triangular pass b -> x; w: 64 x P elements (blocked path)
template <typename T, bool CPLX, bool BACK>
static int la_solve_pass(const T* l, const T* b, T* x, size_t N, size_t P, T* w, hipStream_t s)
{
    constexpr size_t E = CPLX ? 2 : 1;
    if (la_dispatch(N) == LA_PATH_SMALL) return la_launch_trsolve<T, CPLX, BACK>(l, N, b, x, P, N, s);
    if (!w) return BDSP_ERR_UNSUPPORTED;
    const size_t nb = la_blocks(N);
    for (size_t t = 0; t < nb; ++t) {
        const size_t i = BACK ? nb - 1 - t : t, r0 = i * LA_BLOCK;
        const size_t n = N - r0 < (size_t)LA_BLOCK ? N - r0 : (size_t)LA_BLOCK;
        const T* rhs = b + r0 * P * E;
        if (t > 0) {
            if (BACK) { // rows r0 + 64 ... of L, columns r0 ...: conj-transposed; the X below
                const size_t k0 = r0 + LA_BLOCK;
                BDSP_TRY((la_launch_update<T, CPLX, 2>(rhs, P, l + (k0 * N + r0) * E, N, x + k0 * P * E, P, w, P, n, P, N - k0, (T)0, s)));
            } else BDSP_TRY((la_launch_update<T, CPLX, 1>(rhs, P, l + r0 * N * E, N, x, P, w, P, n, P, r0, (T)0, s)));
            rhs = w;
        }
        BDSP_TRY((la_launch_trsolve<T, CPLX, BACK>(l + (r0 * N + r0) * E, N, rhs, x + r0 * P * E, P, n, s)));
    }
    return BDSP_OK;
}

template <typename T, bool CPLX>
static int la_solve_run(const T* l, const T* b, T* x, size_t N, size_t P, int part, T* scratch, hipStream_t s)
{
    constexpr size_t E = CPLX ? 2 : 1;
    T* w = la_dispatch(N) == LA_PATH_BLOCKED ? scratch : nullptr;
    if (part == LA_PART_FORWARD) return la_solve_pass<T, CPLX, false>(l, b, x, N, P, w, s);
    if (part == LA_PART_BACKWARD) return la_solve_pass<T, CPLX, true>(l, b, x, N, P, w, s);
    if (!scratch) return BDSP_ERR_UNSUPPORTED;
    T* y = scratch + (w ? (size_t)LA_BLOCK * P * E : 0); // the forward pass's result
    BDSP_TRY((la_solve_pass<T, CPLX, false>(l, b, y, N, P, w, s)));
    return la_solve_pass<T, CPLX, true>(l, y, x, N, P, w, s);
}

// elements of the temporary each call needs
size_t la_chol_scratch(size_t N) { return N && la_dispatch(N) == LA_PATH_BLOCKED ? N * LA_BLOCK : 0; }
size_t la_solve_scratch(size_t N, size_t P, int part)
{
    if (!N || !P) return 0;
    return (la_dispatch(N) == LA_PATH_BLOCKED ? (size_t)LA_BLOCK * P : 0) + (part == LA_PART_BOTH ? N * P : 0);
}

template <typename T>
int la_cholesky(const T* a, T* out, size_t N, bool is_complex, T loading, T* scratch, unsigned* flag, hipStream_t s)
{
    if (!N) return BDSP_OK;
    if (is_complex) return la_chol_run<T, true>(a, out, N, loading, scratch, flag, s);
    return la_chol_run<T, false>(a, out, N, loading, scratch, flag, s);
}

template <typename T>
int la_cholesky_solve(const T* l, const T* b, T* x, size_t N, size_t P, bool is_complex, int part, T* scratch, hipStream_t s)
{
    if (!N || !P) return BDSP_OK;
    if (is_complex) return la_solve_run<T, true>(l, b, x, N, P, part, scratch, s);
    return la_solve_run<T, false>(l, b, x, N, P, part, scratch, s);
}

template int la_cholesky<float>(const float*, float*, size_t, bool, float, float*, unsigned*, hipStream_t);
template int la_cholesky<double>(const double*, double*, size_t, bool, double, double*, unsigned*, hipStream_t);
template int la_cholesky_solve<float>(const float*, const float*, float*, size_t, size_t, bool, int, float*, hipStream_t);
template int la_cholesky_solve<double>(const double*, const double*, double*, size_t, size_t, bool, int, double*, hipStream_t);

} // namespace bdsp
