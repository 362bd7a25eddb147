// mat_reduce.hip -- per-row statistics, sums and dot products of a matrix (matrix/src/general/statistics.rs,
// matrix/src/general/mod.rs:9-241): ONE batched pass over all rows, one result per row (or per row and bucket for
// statistics_split).  The element and merge rules are reduce.hip's (reduce_common.h), so count, min, max and their
// indices equal the vector path's bit for bit whatever the mapping; sums add in double in another order.  Indices are
// within the row.  No float atomics: every fold has a fixed shape, repeated calls give identical bits.
//
// The mapping follows the row length (thresholds checked by the sweep in profiles/r07_mat_reduce.txt):
//   short  (<= MR_SHORT_MAX_PK packets): G = 4..64 lanes per row, 256 / G rows per workgroup, folded with
//          cross-lane shuffles, no LDS, results written straight to their slot
//   medium: one 256-lane workgroup per row, folded in the wave, then across the 4 waves through LDS
//   long, few rows: `chunks` workgroups per row write partials [row][chunk]; k_mr_fold folds each row's partials
// The result is finished on the device (k_mr_* write the header's Statistics / sum structs; stat_emit mirrors
// capi.cpp's stat_fill_real / stat_fill_complex), so the host only copies it out.
#include "bdsp_internal.h"
#include "reduce_common.h"

namespace bdsp {

// ------------------------------------------------------------------------------------------ finishing step
template <typename R, bool CPLX> struct StatsOf;
template <> struct StatsOf<float, false> { using type = Statistics32; };
template <> struct StatsOf<double, false> { using type = Statistics64; };
template <> struct StatsOf<float, true> { using type = ComplexStatistics32; };
template <> struct StatsOf<double, true> { using type = ComplexStatistics64; };

template <typename R, bool CPLX>
__device__ __forceinline__ void stat_fill(void* out, size_t i, const StatPartial& p)
{
    typename StatsOf<R, CPLX>::type& o = reinterpret_cast<typename StatsOf<R, CPLX>::type*>(out)[i];
    const double n = (double)p.cnt;
    if constexpr (CPLX) {
        // sqrt of the COMPLEX mean of z*z (principal branch), as stat_fill_complex
        const double qr = p.qr / n, qi = p.qi / n;
        const double r = hypot(qr, qi);
        double rr, ri;
        if (r != r) { rr = ri = __builtin_nan(""); }
        else if (qi == 0.0 && qr >= 0.0) { rr = sqrt(qr); ri = qi; }
        else if (qi == 0.0) { rr = 0.0; ri = signbit(qi) ? -sqrt(-qr) : sqrt(-qr); }
        else { const double th = atan2(qi, qr) / 2; rr = sqrt(r) * cos(th); ri = sqrt(r) * sin(th); }
        o.sum.re = (R)p.sr; o.sum.im = (R)p.si; o.count = (size_t)p.cnt;
        o.average.re = (R)(p.sr / n); o.average.im = (R)(p.si / n);
        o.rms.re = (R)rr; o.rms.im = (R)ri;
        o.min.re = (R)p.mnr; o.min.im = (R)p.mni; o.min_index = (size_t)p.imn;
        o.max.re = (R)p.mxr; o.max.im = (R)p.mxi; o.max_index = (size_t)p.imx;
    } else {
        o.sum = (R)p.sr; o.count = (size_t)p.cnt;
        o.average = (R)(p.sr / n); o.rms = (R)sqrt(p.qr / n);
        o.min = (R)p.mnr; o.min_index = (size_t)p.imn; o.max = (R)p.mxr; o.max_index = (size_t)p.imx;
    }
}

template <typename R, bool CPLX>
__device__ __forceinline__ void sum_fill(void* out, size_t i, double re, double im)
{
    R* o = reinterpret_cast<R*>(out);
    if (CPLX) { o[2 * i] = (R)re; o[2 * i + 1] = (R)im; } else o[i] = (R)re;
}

// result i of a launch: the raw partial (long rows), the header's struct, or one (complex) sum in T or double
template <typename T, bool CPLX>
__device__ __forceinline__ void stat_emit(int kind, void* out, size_t i, const StatPartial& p)
{
    switch (kind) {
    case MR_OUT_PARTIAL: reinterpret_cast<StatPartial*>(out)[i] = p; break;
    case MR_OUT_STATS: stat_fill<T, CPLX>(out, i, p); break;
    case MR_OUT_STATS_PREC: stat_fill<double, CPLX>(out, i, p); break;
    case MR_OUT_SUM: sum_fill<T, CPLX>(out, i, p.sr, p.si); break;
    case MR_OUT_SUM_PREC: sum_fill<double, CPLX>(out, i, p.sr, p.si); break;
    case MR_OUT_SUM_SQ: sum_fill<T, CPLX>(out, i, p.qr, p.qi); break;
    default: sum_fill<double, CPLX>(out, i, p.qr, p.qi); break;
    }
}

// ------------------------------------------------------------------------------------------ folds
template <bool MINMAX>
__device__ __forceinline__ void stat_fold_xor(StatPartial& p, int m)
{
    StatPartial q = p;
    q.sr = __shfl_xor(p.sr, m); q.si = __shfl_xor(p.si, m);
    q.qr = __shfl_xor(p.qr, m); q.qi = __shfl_xor(p.qi, m);
    q.cnt = __shfl_xor(p.cnt, m);
    if (MINMAX) {
        q.mn_key = __shfl_xor(p.mn_key, m); q.mnr = __shfl_xor(p.mnr, m); q.mni = __shfl_xor(p.mni, m);
        q.imn = __shfl_xor(p.imn, m);
        q.mx_key = __shfl_xor(p.mx_key, m); q.mxr = __shfl_xor(p.mxr, m); q.mxi = __shfl_xor(p.mxi, m);
        q.imx = __shfl_xor(p.imx, m);
    }
    // the butterfly gives every lane of the group the same bits: a + b == b + a, and the (key, index) order of
    // stat_merge_ordered is total
    stat_merge_ordered(p, q);
}

// G lanes (a power of two <= 64, aligned within the wave) end holding the fold of their partials
template <int G, bool MINMAX>
__device__ __forceinline__ void stat_fold_group(StatPartial& p)
{
#pragma unroll
    for (int m = (G > 64 ? 64 : G) / 2; m > 0; m >>= 1) stat_fold_xor<MINMAX>(p, m);
}

// a 256-lane workgroup: in the wave, then the 4 wave results through LDS in wave order; lane 0 holds the result
template <bool MINMAX>
__device__ __forceinline__ void stat_fold_block(StatPartial& p)
{
    __shared__ StatPartial sh[4];
    stat_fold_group<64, MINMAX>(p);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) stat_merge_ordered(p, sh[w]);
}

// ------------------------------------------------------------------------------------------ segment walks
// Elements [e0, e1) of one row (element j at row[j * SPE]), lane `lane` of G: elements in front of the first 16-byte
// boundary and behind the last whole packet one by one, the rest as 16-byte packets, four in flight per lane.  A lane
// meets its elements in ascending order, which is what the strict comparisons of stat_take need.
template <typename T, bool CPLX, int G, class F>
__device__ __forceinline__ void seg_walk(const T* __restrict__ row, size_t e0, size_t e1, unsigned lane, F&& take)
{
    constexpr int SPE = CPLX ? 2 : 1;
    constexpr int TPP = 16 / sizeof(T);
    constexpr int EPP = TPP / SPE;
    struct alignas(16) Pk { T v[TPP]; };
    const uintptr_t a = (uintptr_t)(row + e0 * SPE);
    size_t head = e1 - e0; // pairs at an odd scalar never reach a packet boundary: all one by one
    if (a % (sizeof(T) * SPE) == 0) {
        const size_t h = (16 - a % 16) % 16 / (sizeof(T) * SPE);
        if (h < head) head = h;
    }
    const size_t pb = e0 + head, npk = (e1 - pb) / EPP, pe = pb + npk * EPP;
    for (size_t j = e0 + lane; j < pb; j += G) take(row[j * SPE], CPLX ? row[j * SPE + 1] : T(0), j);
    const Pk* __restrict__ xp = reinterpret_cast<const Pk*>(row + pb * SPE);
    for (size_t q = lane; q < npk; q += 4 * G) {
        Pk pk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q + G * u < npk) pk[u] = xp[q + G * u];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q + G * u < npk) {
#pragma unroll
                for (int k = 0; k < EPP; ++k)
                    take(pk[u].v[CPLX ? 2 * k : k], CPLX ? pk[u].v[2 * k + 1] : T(0), pb + (q + G * u) * EPP + k);
            }
    }
    for (size_t j = pe + lane; j < e1; j += G) take(row[j * SPE], CPLX ? row[j * SPE + 1] : T(0), j);
}

// which (segment, chunk, element range) lane group `unit` owns; a segment is a row (nb == 1) or one bucket of a row
struct MrUnit {
    size_t seg, row, e0, e1;
    unsigned b;
};
__device__ __forceinline__ MrUnit mr_unit(const MrGeom& g, size_t unit)
{
    MrUnit u;
    u.seg = unit / g.chunks;
    const size_t c = unit % g.chunks;
    u.row = u.seg / g.nb;
    u.b = (unsigned)(u.seg % g.nb);
    const size_t cnt = g.n > u.b ? (g.n - u.b + g.nb - 1) / g.nb : 0; // elements of this bucket
    u.e0 = c * g.per < cnt ? c * g.per : cnt;
    u.e1 = u.e0 + g.per < cnt ? u.e0 + g.per : cnt;
    return u;
}

// ------------------------------------------------------------------------------------------ kernels
// G <= 64: 256 / G lane groups per workgroup, one unit each; G == 256: one unit per workgroup
template <typename T, bool CPLX, bool MINMAX, int G>
__global__ __launch_bounds__(256) void k_mr_stats(const T* __restrict__ x, MrGeom g)
{
    constexpr int SPE = CPLX ? 2 : 1;
    const size_t unit = G == 256 ? (size_t)blockIdx.x : (size_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const unsigned lane = threadIdx.x % G;
    StatPartial p;
    stat_init(p, CPLX);
    const bool live = unit < g.units; // (the last workgroup's surplus groups still join no fold but their own)
    if (live) {
        const MrUnit u = mr_unit(g, unit);
        const T* row = x + u.row * g.stride;
        auto take = [&](T re, T im, size_t j) { stat_take<T, CPLX, MINMAX>(p, re, im, j); };
        if (g.nb == 1) {
            seg_walk<T, CPLX, G>(row, u.e0, u.e1, lane, take);
        } else { // statistics_split: element b + k*nb is element k of bucket b
            for (size_t k = u.e0 + lane; k < u.e1; k += G) {
                const size_t j = (u.b + k * g.nb) * SPE;
                take(row[j], CPLX ? row[j + 1] : T(0), k);
            }
        }
    }
    if (G == 256) stat_fold_block<MINMAX>(p);
    else stat_fold_group<G, MINMAX>(p);
    if (live && lane == 0) stat_emit<T, CPLX>(g.kind, g.out, unit, p);
}

// dot products: row r of x with row r of y (ystride = its row length) or with one vector (ystride = 0), both read
// through the cache; complex products without conjugation, as k_dot.  x as 16-byte packets from its first boundary on,
// y's matching scalars as element-aligned 16-byte loads (gfx950 takes dword-aligned global_load_dwordx4: a broadcast
// vector against odd-length rows keeps the packet path).
template <typename T, bool CPLX, int G>
__global__ __launch_bounds__(256) void k_mr_dot(const T* __restrict__ x, const T* __restrict__ y, size_t ystride,
                                                MrGeom g)
{
    constexpr int SPE = CPLX ? 2 : 1;
    constexpr int TPP = 16 / sizeof(T);
    constexpr int EPP = TPP / SPE;
    struct alignas(16) Pk { T v[TPP]; };
    struct alignas(sizeof(T)) Pu { T v[TPP]; }; // y's packets: element-aligned
    const size_t unit = G == 256 ? (size_t)blockIdx.x : (size_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const unsigned lane = threadIdx.x % G;
    StatPartial p;
    stat_init(p, CPLX);
    const bool live = unit < g.units;
    if (live) {
        const MrUnit u = mr_unit(g, unit);
        const T* xr = x + u.row * g.stride;
        const T* yr = y + u.row * ystride;
        double a = 0.0, b = 0.0;
        auto take = [&](T ar, T ai, T br, T bi) {
            if (CPLX) {
                a += (double)ar * (double)br - (double)ai * (double)bi;
                b += (double)ar * (double)bi + (double)ai * (double)br;
            } else {
                a += (double)ar * (double)br;
            }
        };
        const uintptr_t ax = (uintptr_t)(xr + u.e0 * SPE), ay = (uintptr_t)(yr + u.e0 * SPE);
        size_t head = u.e1 - u.e0;
        if (ax % (sizeof(T) * SPE) == 0 && ay % (sizeof(T) * SPE) == 0) {
            const size_t h = (16 - ax % 16) % 16 / (sizeof(T) * SPE);
            if (h < head) head = h;
        }
        const size_t pb = u.e0 + head, npk = (u.e1 - pb) / EPP, pe = pb + npk * EPP;
        auto one = [&](size_t j) {
            take(xr[j * SPE], CPLX ? xr[j * SPE + 1] : T(0), yr[j * SPE], CPLX ? yr[j * SPE + 1] : T(0));
        };
        for (size_t j = u.e0 + lane; j < pb; j += G) one(j);
        const Pk* __restrict__ xp = reinterpret_cast<const Pk*>(xr + pb * SPE);
        const Pu* __restrict__ yp = reinterpret_cast<const Pu*>(yr + pb * SPE);
        for (size_t q = lane; q < npk; q += 2 * G) {
            Pk px[2];
            Pu py[2];
#pragma unroll
            for (int v = 0; v < 2; ++v)
                if (q + G * v < npk) { px[v] = xp[q + G * v]; py[v] = yp[q + G * v]; }
#pragma unroll
            for (int v = 0; v < 2; ++v)
                if (q + G * v < npk) {
#pragma unroll
                    for (int k = 0; k < EPP; ++k)
                        take(px[v].v[CPLX ? 2 * k : k], CPLX ? px[v].v[2 * k + 1] : T(0), py[v].v[CPLX ? 2 * k : k],
                             CPLX ? py[v].v[2 * k + 1] : T(0));
                }
        }
        for (size_t j = pe + lane; j < u.e1; j += G) one(j);
        p.sr = a; p.si = b;
    }
    if (G == 256) stat_fold_block<false>(p);
    else stat_fold_group<G, false>(p);
    if (live && lane == 0) stat_emit<T, CPLX>(g.kind, g.out, unit, p);
}

// long rows: one workgroup per segment folds its `chunks` partials [seg][chunk] (k_stats_final with a partial stride)
template <typename T, bool CPLX>
__global__ __launch_bounds__(256) void k_mr_fold(const StatPartial* __restrict__ partials, unsigned chunks, int kind,
                                                 void* out)
{
    StatPartial p;
    stat_init(p, CPLX);
    partials += (size_t)blockIdx.x * chunks;
    for (unsigned i = threadIdx.x; i < chunks; i += 256) stat_merge_ordered(p, partials[i]);
    stat_fold_block<true>(p);
    if (threadIdx.x == 0) stat_emit<T, CPLX>(kind, out, blockIdx.x, p);
}

// ------------------------------------------------------------------------------------------ mapping + launch
// Thresholds in 16-byte packets of one segment (profiles/r07_mat_reduce.txt, row-length sweep):
// The fold of a lane group costs log2(G) shuffle rounds of the 104-byte partial per lane: with 4 packets per lane it
// cost as much as the data (first sweep: 65 536 x 128 complex f64 1.74x, 16 384 x 1000 complex f32 3.6x the flat kernel),
// with 16 it is a fraction of it.
constexpr size_t MR_PK_PER_LANE = 16;     // a short row's lane group is sized for ~16 packets per lane
constexpr size_t MR_SHORT_MAX_PK = 1024;  // up to 64 lanes x 16 packets (16 KiB) per row: lane groups; above, workgroups
constexpr size_t MR_CHUNK_MIN_PK = 4096;  // a long row's chunk keeps >= 64 KiB per workgroup (16 packets per lane)
constexpr size_t MR_MAX_CHUNKS = 1024;
static size_t mr_wg_target() { return (size_t)num_cus() * 4; } // workgroups that fill the CUs (red_grid's cap)

struct MrPlan {
    int G;
    unsigned chunks;
};
static MrPlan mr_plan(size_t segs, size_t seg_elems, size_t epp)
{
    const size_t npk = (seg_elems + epp - 1) / epp;
    MrPlan pl{256, 1};
    if (npk <= MR_SHORT_MAX_PK) {
        const size_t want = (npk + MR_PK_PER_LANE - 1) / MR_PK_PER_LANE;
        pl.G = 4;
        while ((size_t)pl.G < want) pl.G *= 2;
        return pl;
    }
    const size_t target = mr_wg_target();
    if (segs < target && npk >= 2 * MR_CHUNK_MIN_PK) {
        size_t c = (target + segs - 1) / segs, cmax = npk / MR_CHUNK_MIN_PK;
        if (c > cmax) c = cmax;
        if (c > MR_MAX_CHUNKS) c = MR_MAX_CHUNKS;
        pl.chunks = (unsigned)c;
    }
    return pl;
}

static MrGeom mr_geom(size_t rows, size_t n, size_t stride, size_t nb, unsigned chunks, size_t epp)
{
    MrGeom g;
    g.n = n; g.stride = stride; g.nb = nb; g.chunks = chunks;
    const size_t seg_elems = (n + nb - 1) / nb;
    size_t per = (seg_elems + chunks - 1) / chunks;
    if (chunks > 1) per = (per + 64 * epp - 1) / (64 * epp) * (64 * epp); // chunk starts on a packet boundary
    g.per = per ? per : 1;
    g.units = rows * nb * chunks;
    return g;
}

static unsigned mr_blocks(size_t units, int G) { return (unsigned)(G == 256 ? units : (units + 256 / G - 1) / (256 / G)); }

template <typename T, bool CPLX, bool MINMAX>
static void mr_launch_stats(const T* x, const MrGeom& g, int G, hipStream_t s)
{
    const dim3 grid(mr_blocks(g.units, G)), block(256);
    switch (G) {
    case 4: hipLaunchKernelGGL((k_mr_stats<T, CPLX, MINMAX, 4>), grid, block, 0, s, x, g); break;
    case 8: hipLaunchKernelGGL((k_mr_stats<T, CPLX, MINMAX, 8>), grid, block, 0, s, x, g); break;
    case 16: hipLaunchKernelGGL((k_mr_stats<T, CPLX, MINMAX, 16>), grid, block, 0, s, x, g); break;
    case 32: hipLaunchKernelGGL((k_mr_stats<T, CPLX, MINMAX, 32>), grid, block, 0, s, x, g); break;
    case 64: hipLaunchKernelGGL((k_mr_stats<T, CPLX, MINMAX, 64>), grid, block, 0, s, x, g); break;
    default: hipLaunchKernelGGL((k_mr_stats<T, CPLX, MINMAX, 256>), grid, block, 0, s, x, g); break;
    }
}

template <typename T, bool CPLX>
static void mr_launch_dot(const T* x, const T* y, size_t ystride, const MrGeom& g, int G, hipStream_t s)
{
    const dim3 grid(mr_blocks(g.units, G)), block(256);
    switch (G) {
    case 4: hipLaunchKernelGGL((k_mr_dot<T, CPLX, 4>), grid, block, 0, s, x, y, ystride, g); break;
    case 8: hipLaunchKernelGGL((k_mr_dot<T, CPLX, 8>), grid, block, 0, s, x, y, ystride, g); break;
    case 16: hipLaunchKernelGGL((k_mr_dot<T, CPLX, 16>), grid, block, 0, s, x, y, ystride, g); break;
    case 32: hipLaunchKernelGGL((k_mr_dot<T, CPLX, 32>), grid, block, 0, s, x, y, ystride, g); break;
    case 64: hipLaunchKernelGGL((k_mr_dot<T, CPLX, 64>), grid, block, 0, s, x, y, ystride, g); break;
    default: hipLaunchKernelGGL((k_mr_dot<T, CPLX, 256>), grid, block, 0, s, x, y, ystride, g); break;
    }
}

// the second launch of the long-row mapping: partials (rows * nb * chunks) -> out
template <typename T>
static int mr_fold(const StatPartial* partials, size_t segs, unsigned chunks, bool cplx, int kind, void* out,
                   hipStream_t s)
{
    if (cplx) hipLaunchKernelGGL((k_mr_fold<T, true>), dim3((unsigned)segs), dim3(256), 0, s, partials, chunks, kind, out);
    else hipLaunchKernelGGL((k_mr_fold<T, false>), dim3((unsigned)segs), dim3(256), 0, s, partials, chunks, kind, out);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T>
int mr_stats(const T* x, size_t rows, size_t n, size_t stride, size_t nb, bool cplx, bool minmax, int kind, void* out,
             hipStream_t s)
{
    if (rows == 0 || nb == 0) return BDSP_OK;
    const size_t epp = 16 / sizeof(T) / (cplx ? 2 : 1);
    const MrPlan pl = mr_plan(rows * nb, (n + nb - 1) / nb, epp);
    MrGeom g = mr_geom(rows, n, stride, nb, pl.chunks, epp);
    WsBlock pb;
    if (pl.chunks > 1) {
        BDSP_TRY(pb.alloc(sizeof(StatPartial) * g.units, s));
        g.kind = MR_OUT_PARTIAL; g.out = pb.p;
    } else {
        g.kind = kind; g.out = out;
    }
    if (cplx) {
        if (minmax) mr_launch_stats<T, true, true>(x, g, pl.G, s); else mr_launch_stats<T, true, false>(x, g, pl.G, s);
    } else {
        if (minmax) mr_launch_stats<T, false, true>(x, g, pl.G, s); else mr_launch_stats<T, false, false>(x, g, pl.G, s);
    }
    BDSP_LAUNCH_CHECK();
    if (pl.chunks > 1) BDSP_TRY(mr_fold<T>(pb.as<StatPartial>(), rows * nb, pl.chunks, cplx, kind, out, s));
    return BDSP_OK;
}

template <typename T>
int mr_dot(const T* x, size_t xstride, const T* y, size_t ystride, size_t rows, size_t n, bool cplx, int kind,
           void* out, hipStream_t s)
{
    if (rows == 0) return BDSP_OK;
    const size_t epp = 16 / sizeof(T) / (cplx ? 2 : 1);
    const MrPlan pl = mr_plan(rows, n, epp);
    MrGeom g = mr_geom(rows, n, xstride, 1, pl.chunks, epp);
    WsBlock pb;
    if (pl.chunks > 1) {
        BDSP_TRY(pb.alloc(sizeof(StatPartial) * g.units, s));
        g.kind = MR_OUT_PARTIAL; g.out = pb.p;
    } else {
        g.kind = kind; g.out = out;
    }
    if (cplx) mr_launch_dot<T, true>(x, y, ystride, g, pl.G, s);
    else mr_launch_dot<T, false>(x, y, ystride, g, pl.G, s);
    BDSP_LAUNCH_CHECK();
    if (pl.chunks > 1) BDSP_TRY(mr_fold<T>(pb.as<StatPartial>(), rows, pl.chunks, cplx, kind, out, s));
    return BDSP_OK;
}

template int mr_stats<float>(const float*, size_t, size_t, size_t, size_t, bool, bool, int, void*, hipStream_t);
template int mr_stats<double>(const double*, size_t, size_t, size_t, size_t, bool, bool, int, void*, hipStream_t);
template int mr_dot<float>(const float*, size_t, const float*, size_t, size_t, size_t, bool, int, void*, hipStream_t);
template int mr_dot<double>(const double*, size_t, const double*, size_t, size_t, size_t, bool, int, void*, hipStream_t);

} // namespace bdsp
