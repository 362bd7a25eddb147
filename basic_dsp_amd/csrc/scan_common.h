// scan_common.h -- what the vector unit (vecmath.hip) and the matrix unit (mat_scan.hip) of diff / cum_sum / unwrap
// share: the scan chunk size and the exact remainder of unwrap's serial chain.  Also compiled by the host simulation
// (tests/host_sim/sim_mat_scan.cpp), where the device qualifiers fall away.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define BDSP_SCAN_FN __device__ __forceinline__
#else
#define BDSP_SCAN_FN inline
#endif

namespace bdsp {

constexpr int SCAN_PER_THREAD = 16;
constexpr int SCAN_CHUNK = 256 * SCAN_PER_THREAD; // elements per workgroup

// fmod on the serial critical path: the remainder a - trunc(a/b)*b is exactly representable, so one fma returns it
// exactly when the quotient is right; a quotient off by one (a/b rounded across an integer) shows as a remainder
// outside [0, |b|) and is redone.  Huge quotients, infinities and NaNs go to the library function.
template <typename T>
BDSP_SCAN_FN T fmod_exact(T a, T b, T inv_abs_b)
{
    const T A = fabs(a), Bv = fabs(b);
    T q = trunc(A * inv_abs_b); // a guess within one of trunc(A / Bv): the checks below settle it
    if (!(q < (T)(sizeof(T) == 4 ? 4194304.0 : 2251799813685248.0))) return fmod(a, b);
    T r = fma(-q, Bv, A);
    if (r < T(0)) r = fma(-(q - T(1)), Bv, A);
    else if (r >= Bv) r = fma(-(q + T(1)), Bv, A);
    return copysign(r, a);
}

} // namespace bdsp
