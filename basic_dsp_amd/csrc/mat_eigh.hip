// mat_eigh.hip -- the eigendecomposition v a v^H = diag(w) of a Hermitian N x N matrix (real symmetric or complex
// Hermitian, f32 or f64) by the cyclic two-sided Jacobi method in a round-robin ordering (mat_eigh_core.h has the
// iteration, the schedule, the LDS maps and the arithmetic).  Every matrix is dense and row-major; an element is a real
// scalar or an interleaved (re, im) pair.
//
// Two paths, chosen by je_dispatch from N alone:
//   small (N <= 64)  ONE launch of k_je_small, one workgroup: A (both triangles, completed from the lower one) and V in
//                    LDS; per step the first threads fill the rotation table, then the row pass on A and V (lanes along
//                    the columns), then the column pass on A (lanes along the rows), a barrier after each; the sweep
//                    loop, the convergence test (a sum over LDS, the same in every thread), the ranking of the
//                    eigenvalues and the sorted store are all inside the kernel.  One status word comes back.
//   blocked          blocks of 32 columns, the same tournament over the blocks.  k_je_complete writes the work matrix
//                    (both triangles) and V = I, k_je_norm (one workgroup) the threshold.  Per block step: k_je_pivot,
//                    one workgroup per block pair, gathers the <= 64 x 64 pivot problem, runs at most 2 sweeps of the
//                    small path's code on it, writes it back with its accumulated transform and its first sweep's
//                    rotation count; k_je_rows applies the transform to the pair's rows of A outside the pivot block and
//                    of V, one workgroup per pair and tile of 32 columns, in place (a tile is read whole into LDS before
//                    it is written); k_je_cols applies its conjugate transpose to the pair's columns of A outside the
//                    pivot block.  Vector-ALU kernels with the transform in LDS: the matrix instruction was not built
//                    and not measured.  The counts are read back once per outer sweep; k_je_sorted ranks and stores.
//
// Every element of w and v is written by exactly one thread, once; within a launch no workgroup reads what another
// writes.  Plain loads and stores only, no scratch, no register array, no index or bound that depends on matrix data
// beyond the rank an eigenvalue is stored at.  tests/host_sim/sim_mat_eigh.cpp runs the templates of mat_eigh_core.h
// with threads as loops.
#include <type_traits>

#include "bdsp_internal.h"
#include "mat_eigh_core.h"

namespace bdsp {

template <typename T> struct je_pair_t { typedef T type __attribute__((ext_vector_type(2))); };

// raw-pointer accessor of the core templates: scalars, and the (re, im) pair of a complex element in one access
template <typename T>
struct JeRaw {
    T* p;
    using V = typename std::remove_const<T>::type;
    using P = typename je_pair_t<V>::type;
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

extern __shared__ __align__(16) unsigned char je_smem[];

// one sweep over n players on the LDS image; returns the rotations of this thread's pairs
template <typename T, bool CPLX>
__device__ __forceinline__ unsigned je_sweep(const JeLds<T, CPLX, JeRaw<T>>& l, int n, T thr, int tid)
{
    unsigned count = 0;
    const int steps = je_steps(n);
    for (int step = 0; step < steps; ++step) {
        count += je_params<T, CPLX>(l, n, step, thr, tid);
        __syncthreads();
        je_row_pass<T, CPLX>(l, n, step, tid);
        __syncthreads();
        je_col_pass<T, CPLX>(l, n, step, tid);
        __syncthreads();
    }
    return count;
}

// the workgroup's rotations of a sweep, the same number in every thread
template <typename T, bool CPLX>
__device__ __forceinline__ unsigned je_sweep_total(const JeLds<T, CPLX, JeRaw<T>>& l, unsigned count, int tid)
{
    je_count_put<T, CPLX>(l, count, tid);
    __syncthreads();
    const unsigned total = je_count_total<T, CPLX>(l);
    __syncthreads();
    return total;
}

// ---------------------------------------------------------------------------------------------
// the small path: a is the caller's matrix, w (n scalars) and v (n x n) the results, status one word
// ---------------------------------------------------------------------------------------------
template <typename T, bool CPLX>
__global__ __launch_bounds__(JE_THREADS) void k_je_small(const T* __restrict__ a, int n, T* __restrict__ w, T* __restrict__ v,
                                                          unsigned* __restrict__ status)
{
    const JeLds<T, CPLX, JeRaw<T>> l{{reinterpret_cast<T*>(je_smem)}};
    const int tid = (int)threadIdx.x;
    je_load_lower<T, CPLX>(l, JeRaw<const T>{a}, n, tid);
    __syncthreads();
    je_norm_partial<T, CPLX>(l, n, tid);
    __syncthreads();
    unsigned finite;
    const T thr = je_norm_total<T>(l.s, l.red(0), (size_t)n, &finite);
    __syncthreads();
    unsigned word = JE_STATUS_NOT_CONVERGED;
    for (int sweep = 1; sweep <= JE_MAX_SWEEPS; ++sweep) {
        const unsigned count = je_sweep<T, CPLX>(l, n, thr, tid);
        if (je_sweep_total<T, CPLX>(l, count, tid) == 0u) { word = (unsigned)sweep; break; }
    }
    if (!finite) word = JE_STATUS_NOT_FINITE;
    je_rank_put<T, CPLX>(l, n, tid);
    __syncthreads();
    je_store_sorted<T, CPLX>(l, JeRaw<T>{w}, JeRaw<T>{v}, n, tid);
    if (tid == 0) *status = word;
}

// ---------------------------------------------------------------------------------------------
// the blocked path
// ---------------------------------------------------------------------------------------------
template <typename T, bool CPLX>
__global__ __launch_bounds__(JE_THREADS) void k_je_complete(const T* __restrict__ a, T* __restrict__ wk, T* __restrict__ vw, size_t N)
{
    je_complete_row<T, CPLX>(JeRaw<const T>{a}, JeRaw<T>{wk}, JeRaw<T>{vw}, N, (size_t)blockIdx.x, (int)threadIdx.x);
}

// thr[0] = eps |A|_F / N; counts[0] = 1 unless the norm is finite
template <typename T, bool CPLX>
__global__ __launch_bounds__(JE_THREADS) void k_je_norm(const T* __restrict__ wk, size_t N, T* __restrict__ thr, unsigned* __restrict__ counts)
{
    __shared__ T red[JE_THREADS];
    const int tid = (int)threadIdx.x;
    const JeRaw<T> s{red};
    je_norm_partial_global<T, CPLX>(s, 0, JeRaw<const T>{wk}, N, tid);
    __syncthreads();
    unsigned finite;
    const T t = je_norm_total<T>(s, 0, N, &finite);
    if (tid == 0) { thr[0] = t; counts[0] = finite ? 0u : 1u; }
}

// workgroup k: pair k of the block step.  jt: 64 x 64 elements per pair; count: this step's slots
template <typename T, bool CPLX>
__global__ __launch_bounds__(JE_THREADS) void k_je_pivot(T* __restrict__ wk, size_t N, int nb, int step, const T* __restrict__ thr,
                                                          T* __restrict__ jt, unsigned* __restrict__ count)
{
    const JeLds<T, CPLX, JeRaw<T>> l{{reinterpret_cast<T*>(je_smem)}};
    const int tid = (int)threadIdx.x, k = (int)blockIdx.x;
    JeMap mp;
    if (!je_block_map(N, nb, step, k, &mp)) return; // the bye: its slot stays 0
    je_load_pivot<T, CPLX>(l, JeRaw<const T>{wk}, N, mp, tid);
    const T t = thr[0];
    __syncthreads();
    unsigned first = 0;
    for (int sweep = 0; sweep < JE_INNER_SWEEPS; ++sweep) {
        const unsigned total = je_sweep_total<T, CPLX>(l, je_sweep<T, CPLX>(l, mp.m(), t, tid), tid);
        if (sweep == 0) first = total;
        if (total == 0u) break;
    }
    je_store_pivot<T, CPLX>(l, JeRaw<T>{wk}, N, JeRaw<T>{jt + (size_t)k * 64 * 64 * (CPLX ? 2 : 1)}, mp, tid);
    if (tid == 0) count[k] = first;
}

// blockIdx.x = pair * 2 nb + tile: tiles 0 .. nb - 1 are A's columns (the pair's own two blocks are the pivot kernel's),
// tiles nb .. 2 nb - 1 the columns of V
template <typename T, bool CPLX>
__global__ __launch_bounds__(JE_THREADS) void k_je_rows(T* __restrict__ wk, T* __restrict__ vw, size_t N, int nb, int step,
                                                         const T* __restrict__ jt)
{
    const int tid = (int)threadIdx.x, k = (int)(blockIdx.x / (unsigned)(2 * nb)), tile = (int)(blockIdx.x % (unsigned)(2 * nb));
    JeMap mp;
    if (!je_block_map(N, nb, step, k, &mp)) return;
    const bool onv = tile >= nb;
    const size_t c0 = (size_t)(onv ? tile - nb : tile) * JE_BLOCK;
    if (!onv && (c0 == mp.p0 || c0 == mp.q0)) return;
    const int nc = N - c0 < (size_t)JE_BLOCK ? (int)(N - c0) : JE_BLOCK;
    const JeRaw<T> s{reinterpret_cast<T*>(je_smem)}, x{onv ? vw : wk};
    je_tile_load_vt<T, CPLX>(s, JeRaw<const T>{jt + (size_t)k * 64 * 64 * (CPLX ? 2 : 1)}, mp.m(), tid);
    je_rows_load<T, CPLX>(s, x, N, mp, c0, nc, tid);
    __syncthreads();
    je_rows_apply<T, CPLX>(s, x, N, mp, c0, nc, tid);
}

// blockIdx.x = pair * nb + tile of 32 rows of A (the pair's own two blocks are the pivot kernel's)
template <typename T, bool CPLX>
__global__ __launch_bounds__(JE_THREADS) void k_je_cols(T* __restrict__ wk, size_t N, int nb, int step, const T* __restrict__ jt)
{
    const int tid = (int)threadIdx.x, k = (int)(blockIdx.x / (unsigned)nb), tile = (int)(blockIdx.x % (unsigned)nb);
    JeMap mp;
    if (!je_block_map(N, nb, step, k, &mp)) return;
    const size_t r0 = (size_t)tile * JE_BLOCK;
    if (r0 == mp.p0 || r0 == mp.q0) return;
    const int nr = N - r0 < (size_t)JE_BLOCK ? (int)(N - r0) : JE_BLOCK;
    const JeRaw<T> s{reinterpret_cast<T*>(je_smem)}, x{wk};
    je_tile_load_vt<T, CPLX>(s, JeRaw<const T>{jt + (size_t)k * 64 * 64 * (CPLX ? 2 : 1)}, mp.m(), tid);
    je_cols_load<T, CPLX>(s, x, N, mp, r0, nr, tid);
    __syncthreads();
    je_cols_apply<T, CPLX>(s, x, N, mp, r0, nr, tid);
}

// workgroup k: eigenvalue k to its rank in w, row k of V to that row of v
template <typename T, bool CPLX>
__global__ __launch_bounds__(JE_THREADS) void k_je_sorted(const T* __restrict__ wk, const T* __restrict__ vw, T* __restrict__ w,
                                                           T* __restrict__ v, size_t N)
{
    __shared__ T red[JE_THREADS];
    const int tid = (int)threadIdx.x;
    const JeRaw<T> s{red};
    const JeRaw<const T> g{wk}, gv{vw};
    je_rank_partial<T, CPLX>(s, g, N, (size_t)blockIdx.x, tid);
    __syncthreads();
    je_rank_store<T, CPLX>(s, g, gv, JeRaw<T>{w}, JeRaw<T>{v}, N, (size_t)blockIdx.x, tid);
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
template <typename T, bool CPLX>
static int je_run_small(const T* a, T* w, T* v, size_t N, unsigned* status, hipStream_t s)
{
    const size_t lds = sizeof(T) * je_lds_scalars(CPLX);
    auto kern = k_je_small<T, CPLX>;
    BDSP_TRY(kernel_lds(kern, lds));
    hipLaunchKernelGGL(kern, dim3(1), dim3(JE_THREADS), lds, s, a, (int)N, w, v, status);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// scratch (elements): the work matrix, V, one transform per pair of a step
size_t je_scratch(size_t N)
{
    if (!N || je_dispatch(N) == JE_PATH_SMALL) return 0;
    return 2 * N * N + (size_t)je_pair_slots((int)je_blocks(N)) * 64 * 64;
}
// words of the counts buffer: the not-finite flag, then one slot per step and pair of a sweep
size_t je_count_words(size_t N)
{
    if (!N || je_dispatch(N) == JE_PATH_SMALL) return 1;
    const size_t nb = je_blocks(N);
    return 1 + (size_t)je_steps((int)nb) * (size_t)je_pair_slots((int)nb);
}

template <typename T, bool CPLX>
static int je_run_blocked(const T* a, T* w, T* v, size_t N, T* scratch, T* thr, unsigned* counts, unsigned* host_counts,
                          unsigned* sweeps, hipStream_t s)
{
    constexpr size_t E = CPLX ? 2 : 1;
    const int nb = (int)je_blocks(N), steps = je_steps(nb), pairs = je_pair_slots(nb);
    const size_t words = je_count_words(N);
    T *wk = scratch, *vw = scratch + N * N * E, *jt = scratch + 2 * N * N * E;
    BDSP_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned) * words, s));
    hipLaunchKernelGGL((k_je_complete<T, CPLX>), dim3((unsigned)N), dim3(JE_THREADS), 0, s, a, wk, vw, N);
    BDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_je_norm<T, CPLX>), dim3(1), dim3(JE_THREADS), 0, s, (const T*)wk, N, thr, counts);
    BDSP_LAUNCH_CHECK();
    const size_t lds_pivot = sizeof(T) * je_lds_scalars(CPLX), lds_tile = sizeof(T) * je_tile_lds_scalars(CPLX);
    auto pivot = k_je_pivot<T, CPLX>;
    auto rows = k_je_rows<T, CPLX>;
    auto cols = k_je_cols<T, CPLX>;
    *sweeps = 0;
    for (int sweep = 1; sweep <= JE_MAX_SWEEPS; ++sweep) {
        for (int step = 0; step < steps; ++step) {
            BDSP_TRY(kernel_lds(pivot, lds_pivot));
            hipLaunchKernelGGL(pivot, dim3((unsigned)pairs), dim3(JE_THREADS), lds_pivot, s, wk, N, nb, step, (const T*)thr, jt,
                               counts + 1 + (size_t)step * pairs);
            BDSP_LAUNCH_CHECK();
            BDSP_TRY(kernel_lds(rows, lds_tile));
            hipLaunchKernelGGL(rows, dim3((unsigned)(pairs * 2 * nb)), dim3(JE_THREADS), lds_tile, s, wk, vw, N, nb, step, (const T*)jt);
            BDSP_LAUNCH_CHECK();
            BDSP_TRY(kernel_lds(cols, lds_tile));
            hipLaunchKernelGGL(cols, dim3((unsigned)(pairs * nb)), dim3(JE_THREADS), lds_tile, s, wk, N, nb, step, (const T*)jt);
            BDSP_LAUNCH_CHECK();
        }
        // one small copy per outer sweep: the flag and every pair's first-inner-sweep count
        BDSP_HIP_TRY(hipMemcpyAsync(host_counts, counts, sizeof(unsigned) * words, hipMemcpyDeviceToHost, s));
        BDSP_HIP_TRY(hipStreamSynchronize(s));
        if (host_counts[0]) return BDSP_OK; // not finite: *sweeps stays 0
        unsigned any = 0;
        for (size_t i = 1; i < words; ++i) any |= host_counts[i];
        if (!any) { *sweeps = (unsigned)sweep; break; }
    }
    if (!*sweeps) { *sweeps = JE_STATUS_NOT_CONVERGED; return BDSP_OK; }
    hipLaunchKernelGGL((k_je_sorted<T, CPLX>), dim3((unsigned)N), dim3(JE_THREADS), 0, s, (const T*)wk, (const T*)vw, w, v, N);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// *sweeps: the sweeps taken, JE_STATUS_NOT_FINITE or JE_STATUS_NOT_CONVERGED
template <typename T>
int je_eigh(const T* a, T* w, T* v, size_t N, bool is_complex, T* scratch, T* thr, unsigned* counts, unsigned* host_counts,
            unsigned* sweeps, hipStream_t s)
{
    *sweeps = 1;
    if (!N) return BDSP_OK;
    if (je_dispatch(N) == JE_PATH_SMALL) {
        BDSP_TRY(is_complex ? (je_run_small<T, true>(a, w, v, N, counts, s)) : (je_run_small<T, false>(a, w, v, N, counts, s)));
        // the call's only synchronisation: one word
        BDSP_HIP_TRY(hipMemcpyAsync(sweeps, counts, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        BDSP_HIP_TRY(hipStreamSynchronize(s));
        return BDSP_OK;
    }
    if (!scratch) return BDSP_ERR_UNSUPPORTED;
    if (is_complex) return je_run_blocked<T, true>(a, w, v, N, scratch, thr, counts, host_counts, sweeps, s);
    return je_run_blocked<T, false>(a, w, v, N, scratch, thr, counts, host_counts, sweeps, s);
}

template int je_eigh<float>(const float*, float*, float*, size_t, bool, float*, float*, unsigned*, unsigned*, unsigned*, hipStream_t);
template int je_eigh<double>(const double*, double*, double*, size_t, bool, double*, double*, unsigned*, unsigned*, unsigned*, hipStream_t);

} // namespace bdsp
