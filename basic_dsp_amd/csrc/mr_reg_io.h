// mr_reg_io.h -- the register-resident mixed-radix transforms (k_mr_reg3, k_mr_reg2) as mixed_radix.hip sees them: the I/O
// descriptor of their kernels and the two launchers of mixed_radix_reg3_f32.hip / _f64.hip.  The only definition of either.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace bdsp {

// What the kernels fuse besides the transform: input rotation (ifft_shift), input scale, a window on the input or divided out of
// the output, real input, output rotation (fft_shift), real-part / magnitude output -- every option k_mr_wg has.  `plain` = none of them: stage 0 loads
// from HBM and stage 2 stores to it straight from registers.  Otherwise the workgroup stages its transforms' inputs and outputs
// through the two LDS buffers in natural order, in rolled loops that carry the index arithmetic (with it in the unrolled
// register code the plain path's f32 kernels went from 84 to 139 VGPRs and the f64 ones lost a wave per SIMD): three more
// barriers and two more LDS trips per transform for the calls that use an option, nothing for the ones that do not.
template <typename T>
struct MrReg3Io {
    const T* in;
    T* out;
    unsigned rot_in, rot_out; // input element i is x[(i + rot_in) mod n]; output element i is X[(i + rot_out) mod n]
    T in_scale;
    int in_real;              // the input holds n reals per vector
    int out_kind;             // 0 complex, 1 real part, 2 magnitude
    int plain;
    int window_id;            // >= 0: multiply the input by the window (evaluated like the reference, symmetrically) ...
    int window_div;           // ... or divide the output by it (windowed_ifft)
    T alpha;
};

constexpr int MR_REG3_NOT_BUILT = 1 << 20; // what both launchers return for a length without instantiation (-> k_mr_wg)
template <typename T> int mr_reg3_launch(const MrReg3Io<T>& io, size_t n, size_t batch, bool inverse, hipStream_t s); // 300 <= n
template <typename T> int mr_reg2_launch(const MrReg3Io<T>& io, size_t n, size_t batch, bool inverse, hipStream_t s); // n < 300

} // namespace bdsp
