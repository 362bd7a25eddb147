// reduce_common.h -- per-element and merge rules of the statistics reductions, shared by the vector kernels
// (reduce.hip) and the per-row matrix kernels (mat_reduce.hip) so that both produce the same min / max / indices /
// counts bit for bit: accumulation in double, norms computed in T then widened, strict comparisons (first occurrence
// wins, NaN never wins), complex values ordered by norm().
#pragma once

#include "bdsp_internal.h"

namespace bdsp {

template <typename T> __device__ __forceinline__ T dev_norm(T a, T b);
template <> __device__ __forceinline__ float dev_norm<float>(float a, float b) { return hypotf(a, b); }
template <> __device__ __forceinline__ double dev_norm<double>(double a, double b) { return hypot(a, b); }

__device__ __forceinline__ void stat_init(StatPartial& p, bool cplx)
{
    p.sr = p.si = p.qr = p.qi = 0.0;
    p.cnt = 0; p.imn = 0; p.imx = 0;
    if (cplx) { // Statistics<Complex>::empty(): min = (inf, inf), max = (0, 0)   (statistics.rs:270-283)
        p.mnr = p.mni = INFINITY; p.mn_key = INFINITY; p.mxr = p.mxi = 0.0; p.mx_key = 0.0;
    } else {    // min = +inf, max = -inf   (:185-196)
        p.mnr = INFINITY; p.mni = 0.0; p.mn_key = INFINITY; p.mxr = -INFINITY; p.mxi = 0.0; p.mx_key = -INFINITY;
    }
}

// fold b into a: the larger (smaller) key wins the maximum (minimum), equal keys keep the earlier element --
// exactly what one sequential walk with strict comparisons produces (statistics.rs:251-263, 341-353)
__device__ __forceinline__ void stat_merge_ordered(StatPartial& a, const StatPartial& b)
{
    a.sr += b.sr; a.si += b.si; a.qr += b.qr; a.qi += b.qi; a.cnt += b.cnt;
    if (b.mx_key > a.mx_key || (b.mx_key == a.mx_key && b.imx < a.imx)) {
        a.mx_key = b.mx_key; a.mxr = b.mxr; a.mxi = b.mxi; a.imx = b.imx;
    }
    if (b.mn_key < a.mn_key || (b.mn_key == a.mn_key && b.imn < a.imn)) {
        a.mn_key = b.mn_key; a.mnr = b.mnr; a.mni = b.mni; a.imn = b.imn;
    }
}

template <typename T, bool CPLX, bool MINMAX>
__device__ __forceinline__ void stat_take(StatPartial& p, T re, T im, size_t j)
{
    if (CPLX) {
        p.sr += (double)re; p.si += (double)im;
        p.qr += (double)re * (double)re - (double)im * (double)im;
        p.qi += 2.0 * (double)re * (double)im;
        if (MINMAX) {
            const double key = (double)dev_norm<T>(re, im);
            if (key > p.mx_key) { p.mx_key = key; p.mxr = re; p.mxi = im; p.imx = j; }
            if (key < p.mn_key) { p.mn_key = key; p.mnr = re; p.mni = im; p.imn = j; }
        }
    } else {
        p.sr += (double)re; p.qr += (double)re * (double)re;
        if (MINMAX) {
            if ((double)re > p.mx_key) { p.mx_key = re; p.mxr = re; p.imx = j; }
            if ((double)re < p.mn_key) { p.mn_key = re; p.mnr = re; p.imn = j; }
        }
    }
    p.cnt += 1;
}

} // namespace bdsp
