/*
 * basic_dsp_hip.h -- C ABI of libbasic_dsp_hip.so, the MI355X (gfx950) backend for basic_dsp's
 * time/frequency-domain vector operations.
 *
 * Three layers, all plain C (pointers + sizes, no C++/torch types):
 *
 *   B1  bdsp_hip_*_f32/_f64       the five functions of the reference's GPU plug-in trait
 *                                 `GpuSupport<T>` (vector/src/gpu_support/mod.rs:18-46); HOST
 *                                 pointers, synchronous, thread-safe.  This is what a Rust shim
 *                                 `impl GpuSupport<T> for T` binds.
 *   B2  new32, plain_fft32, ...   the subset of the reference's C facade
 *                                 (interop/src/facade32.rs, facade64.rs) that covers the hot path,
 *                                 with IDENTICAL names, argument order and result codes, but the
 *                                 vector lives in HBM.  Handles are opaque.
 *   B3  bdsp_hip_dev_*            the same kernels on caller-owned DEVICE pointers and a caller
 *                                 stream (used by bench.py and the multi-GPU batch driver, which
 *                                 hold memory in torch tensors and communicate through RCCL).
 *
 * All citations are relative to the reference tree (liebharc/basic_dsp v0.10.0).
 * Conventions: complex data is interleaved [re0, im0, re1, im1, ...];
 * every `len` counts SCALARS; `points` = len/2 for complex vectors.
 */
#ifndef BASIC_DSP_HIP_H
#define BASIC_DSP_HIP_H

#include <stddef.h>
#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Result codes.  0 = ok; 1..14 = the reference's ErrorReason numbering
 * (interop/src/lib.rs:125-142, translate_error); -1 = vector is poisoned
 * (interop/src/lib.rs:145-151); <= -100 = backend failure (no reference counterpart: the OpenCL
 * backend panics instead, vector/src/gpu_support/ocl/mod.rs:167,188,208).
 * ---------------------------------------------------------------------------------------- */
#define BDSP_OK 0
#define BDSP_ERR_SAME_SIZE 1             /* InputMustHaveTheSameSize */
#define BDSP_ERR_META_DATA 2             /* InputMetaDataMustAgree */
#define BDSP_ERR_MUST_BE_COMPLEX 3       /* InputMustBeComplex */
#define BDSP_ERR_MUST_BE_REAL 4          /* InputMustBeReal */
#define BDSP_ERR_MUST_BE_TIME 5          /* InputMustBeInTimeDomain */
#define BDSP_ERR_MUST_BE_FREQ 6          /* InputMustBeInFrequencyDomain */
#define BDSP_ERR_ARG_LENGTH 7            /* InvalidArgumentLength */
#define BDSP_ERR_CONJ_SYMMETRIC 8        /* InputMustBeConjSymmetric */
#define BDSP_ERR_ODD_LENGTH 9            /* InputMustHaveAnOddLength */
#define BDSP_ERR_FN_SYMMETRIC 10         /* ArgumentFunctionMustBeSymmetric */
#define BDSP_ERR_COMBINED_ARGS 11        /* InvalidNumberOfArgumentsForCombinedOp */
#define BDSP_ERR_NOT_EMPTY 12            /* InputMustNotBeEmpty */
#define BDSP_ERR_EVEN_LENGTH 13          /* InputMustHaveAnEvenLength */
#define BDSP_ERR_CANNOT_RESIZE 14        /* TypeCanNotResize */
#define BDSP_ERR_POISONED (-1)
#define BDSP_ERR_NO_DEVICE (-100)        /* no usable gfx950 device / HIP runtime failure */
#define BDSP_ERR_HIP (-101)              /* a HIP call failed; see bdsp_hip_last_error() */
#define BDSP_ERR_UNSUPPORTED (-102)      /* argument combination this backend does not implement */

/* Human-readable text of the last backend failure on the calling thread ("" if none). */
const char *bdsp_hip_last_error(void);
/* Library version string, e.g. "basic_dsp_hip 0.1.0 (gfx950)". */
const char *bdsp_hip_version(void);

/* ==========================================================================================
 * B1 -- GpuSupport<T> (vector/src/gpu_support/mod.rs:18-46).  HOST pointers.
 * ======================================================================================== */

/* fn has_gpu_support() -> bool            (gpu_support/mod.rs:21)
 * 1 if a gfx950 device is usable (for _f64: always the same answer, MI355X has native fp64). */
int bdsp_hip_has_gpu_support_f32(void);
int bdsp_hip_has_gpu_support_f64(void);

/* fn is_supported_fft_len(is_complex, len) -> bool      (gpu_support/mod.rs:32)
 * `len` in scalars.  Like the OpenCL backend (ocl/mod.rs:277-299) real input is refused; unlike
 * it, EVERY complex length is supported (powers of two and 2,3,5,7-smooth lengths natively, all other
 * lengths through Bluestein on the same kernels), matching what rustfft accepts on the CPU path --
 * from the B1 size policy's FFT_MIN_LEN (below) up: shorter vectors are answered 0 so that the caller
 * keeps them on rustfft, which is faster than a host round trip there. */
int bdsp_hip_is_supported_fft_len_f32(int is_complex, size_t len);
int bdsp_hip_is_supported_fft_len_f64(int is_complex, size_t len);

/* The size policy of B1.  Every B1 call is a host round trip (upload, kernels, download, one synchronisation); below some
 * length the CPU code the reference runs when the plug-in declines is faster.  The reference's OpenCL backend picked its
 * device by data length for the same reason (gpu_support/ocl/mod.rs:69-80).  The trait offers two ways to decline:
 *   is_supported_fft_len -> false   sends fft() to rustfft          (time_freq/mod.rs:41-44)
 *   gpu_convolve_vector  -> None    sends convolve_signal on       (convolution.rs:504-541)
 * and this library uses them below these thresholds:
 *   FFT_MIN_LEN   is_supported_fft_len answers 0 for len (scalars) below it.  bdsp_hip_fft_* itself still transforms ANY
 *                 length it is handed.
 *   CONV_MIN_WORK gpu_convolve_vector answers 0 (None) when points x taps is below it AND the reference's next choice is
 *                 its direct form convolve_signal_scalar (real data, imp_len <= 15 scalars, or src_len <= 10 imp_len); a
 *                 complex vector the reference would send into its own overlap_discard is never declined.
 * Defaults: the crossovers measured on an MI355X box against one host core (profiles/r06_b1_crossover.txt,
 * tools/b1_crossover.py -- which a deployment can rerun on its own host).  0 = never decline.  Process-wide, thread-safe. */
#define BDSP_B1_FFT_MIN_LEN_F32 0
#define BDSP_B1_FFT_MIN_LEN_F64 1
#define BDSP_B1_CONV_MIN_WORK_F32 2
#define BDSP_B1_CONV_MIN_WORK_F64 3
size_t bdsp_hip_b1_policy_get(int key);
int bdsp_hip_b1_policy_set(int key, size_t value); /* BDSP_OK, or BDSP_ERR_UNSUPPORTED for an unknown key */

/* fn fft(is_complex, signal: &mut [T], direction)       (gpu_support/mod.rs:35)
 * In place on `len` scalars (= len/2 complex points), UNNORMALISED in both directions
 * (time_freq/mod.rs:47-58 contract).  inverse = 0 forward, 1 inverse.  Returns BDSP_OK or a
 * negative backend code (the Rust shim panics on != 0, as the OpenCL impl does). */
int bdsp_hip_fft_f32(int is_complex, float *signal, size_t len, int inverse);
int bdsp_hip_fft_f64(int is_complex, double *signal, size_t len, int inverse);

/* fn gpu_convolve_vector(is_complex, source, target, imp_resp) -> Option<Range<usize>>
 *                                                        (gpu_support/mod.rs:24-29)
 * Computes the reference's centred circular convolution (time_freq/mod.rs:455-473)
 *     y[i] = sum_k x[(i + ceil(M/2) - 1 - k) mod N] * h[k]
 * for EVERY output including the wrap-around head and tail (the OpenCL backend leaves those to
 * the CPU and never fills the tail, convolution.rs:509-527).  Returns 1 and sets
 * [*range_start, *range_end) = [0, src_len) for Some(range); returns 0 for None (declined:
 * empty input or taps longer than the signal); negative on backend failure. */
int bdsp_hip_convolve_vector_f32(int is_complex, const float *src, size_t src_len, float *dst,
                                 size_t dst_len, const float *imp, size_t imp_len,
                                 size_t *range_start, size_t *range_end);
int bdsp_hip_convolve_vector_f64(int is_complex, const double *src, size_t src_len, double *dst,
                                 size_t dst_len, const double *imp, size_t imp_len,
                                 size_t *range_start, size_t *range_end);

/* fn overlap_discard(x_time, tmp, x_freq, h_freq, imp_len, step_size) -> usize
 *                                                        (gpu_support/mod.rs:38-45)
 * All lengths in scalars (factor 2 against the caller's complex view, convolution.rs:401-412).
 * fft_len = h_len.  Blocks start at scalar position 0 and advance by step_size while
 * pos + fft_len < x_len; each block's valid part tmp[imp_len-2 .. fft_len] lands at
 * x_time[pos + imp_len/2 ..]; the LAST block's full time-domain result is left in `tmp` and the
 * final position is returned (ocl/mod.rs:426-520).  tmp[0 .. imp_len/2] (the caller's scalar
 * head, convolution.rs:376-385) is copied to x_time[0 .. imp_len/2] first, as the OpenCL impl
 * does.  The 1/fft_len scaling is applied here (h_freq arrives unscaled).  x_freq is scratch the
 * reference passes along; it is not touched.  The return value is a POSITION; failure is reported out of band:
 * the call clears the calling thread's bdsp_hip_last_error() on entry and leaves a message there (and returns 0)
 * if the backend failed -- check the message, not the position. */
size_t bdsp_hip_overlap_discard_f32(float *x_time, size_t x_len, float *tmp, size_t tmp_len,
                                    float *x_freq, size_t x_freq_len, const float *h_freq,
                                    size_t h_len, size_t imp_len, size_t step_size);
size_t bdsp_hip_overlap_discard_f64(double *x_time, size_t x_len, double *tmp, size_t tmp_len,
                                    double *x_freq, size_t x_freq_len, const double *h_freq,
                                    size_t h_len, size_t imp_len, size_t step_size);

/* ==========================================================================================
 * B2 -- device-resident vectors behind the reference's C facade names
 *       (interop/src/facade32.rs; facade64.rs is generated from it by facade64_create.pl).
 * Ownership follows the facade: operations take the handle BY VALUE (it moves in) and hand it
 * back inside the result struct; borrowed operands are const pointers.
 * ======================================================================================== */
typedef struct VecBuf32 VecBuf32; /* InteropVec<f32>, interop/src/lib.rs:16-22 */
typedef struct VecBuf64 VecBuf64;

/* #[repr(C)] VectorInteropResult<T> { result_code: i32, vector: Box<T> }  (lib.rs:203-212) */
typedef struct { int32_t result_code; VecBuf32 *vector; } VectorInteropResult32;
typedef struct { int32_t result_code; VecBuf64 *vector; } VectorInteropResult64;

/* domain: 0 = time, otherwise frequency (facade32.rs:24-28).  Window ids (lib.rs:153-164):
 * 0 triangular, 1 Hamming(0.54), 2 Blackman-Harris, 3 rectangular; 4 = Hann (generalised
 * Hamming alpha 0.5) is an ADDITION so windowed_fft(Hann) needs no host callback.
 * Conv function ids (lib.rs:166-192): 0 sinc, otherwise raised cosine(rolloff).
 * Padding option ids (lib.rs:194-200): 0 End, 1 Surround, otherwise Center. */

VecBuf32 *new32(int32_t is_complex, int32_t domain, float init_value, size_t length,
                float delta);                                  /* facade32.rs:22-41 */
VecBuf32 *new_with_performance_options32(int32_t is_complex, int32_t domain, float init_value,
                                         size_t length, float delta, size_t core_limit,
                                         int early_temp_allocation); /* :43-70 (options ignored) */
void delete_vector32(VecBuf32 *vector);                        /* facade32.rs:17-19 */
VecBuf32 *clone32(VecBuf32 *vector); /* facade32.rs:687-692; consumes its argument like the reference (Box by value) */
VecBuf32 *bdsp_hip_vec_clone32(const VecBuf32 *vector); /* non-consuming copy (addition) */
float get_value32(const VecBuf32 *vector, size_t index);     /* facade32.rs:105-107 (one-element download) */
size_t get_len32(const VecBuf32 *vector);                      /* facade32.rs:138-140 */
size_t get_points32(const VecBuf32 *vector);                   /* facade32.rs:148-150 */
float get_delta32(const VecBuf32 *vector);                     /* facade32.rs:153-155 */
int32_t is_complex32(const VecBuf32 *vector);                  /* facade32.rs:115-121 */
int32_t get_domain32(const VecBuf32 *vector);                  /* facade32.rs:130-135 */
/* data32 (facade32.rs:158-160) returns a pointer into host memory in the reference.  Here the
 * data lives in HBM: data32 downloads into a host mirror owned by the handle (valid until the
 * next call on that handle) and returns it. */
const float *data32(VecBuf32 *vector);
/* overwrite_data32 (facade32.rs:827-846): uploads `len` scalars into the front of the vector.
 * The reference rejects len >= vector.len() (strict `<`, :834); we accept len <= vector.len()
 * and return code 7 (InvalidArgumentLength) beyond that. */
VectorInteropResult32 overwrite_data32(VecBuf32 *vector, const float *data, size_t len);
void set_len32(VecBuf32 *vector, size_t len);               /* facade32.rs:143-145 */

VectorInteropResult32 real_offset32(VecBuf32 *vector, float value);          /* facade32.rs:363-365 */
VectorInteropResult32 real_scale32(VecBuf32 *vector, float value);           /* facade32.rs:368-370 */
VectorInteropResult32 complex_offset32(VecBuf32 *vector, float re, float im);/* facade32.rs:532-538 */
VectorInteropResult32 complex_scale32(VecBuf32 *vector, float re, float im); /* facade32.rs:541-547 */
VectorInteropResult32 add32(VecBuf32 *vector, const VecBuf32 *operand);      /* facade32.rs:173-175 */
VectorInteropResult32 sub32(VecBuf32 *vector, const VecBuf32 *operand);      /* facade32.rs:178-180 */
VectorInteropResult32 mul32(VecBuf32 *vector, const VecBuf32 *operand);      /* facade32.rs:188-190 */
VectorInteropResult32 div32(VecBuf32 *vector, const VecBuf32 *operand);      /* facade32.rs:183-185 */
VectorInteropResult32 conj32(VecBuf32 *vector);                              /* facade32.rs:579-581 */
VectorInteropResult32 multiply_complex_exponential32(VecBuf32 *vector, float a, float b); /* facade32.rs:695-701 */
VectorInteropResult32 magnitude32(VecBuf32 *vector);                         /* facade32.rs:559-561 */
VectorInteropResult32 magnitude_squared32(VecBuf32 *vector);                 /* facade32.rs:574-576 */
VectorInteropResult32 to_real32(VecBuf32 *vector);                           /* facade32.rs:584-586 */
VectorInteropResult32 to_imag32(VecBuf32 *vector);                           /* facade32.rs:589-591 */
VectorInteropResult32 phase32(VecBuf32 *vector);                             /* facade32.rs:662-664 */
VectorInteropResult32 to_complex32(VecBuf32 *vector);                        /* facade32.rs:418-420 */
VectorInteropResult32 reverse32(VecBuf32 *vector);                           /* facade32.rs:1142-1144 */
VectorInteropResult32 swap_halves32(VecBuf32 *vector);                       /* facade32.rs:527-529 */
VectorInteropResult32 zero_pad32(VecBuf32 *vector, size_t points, int32_t padding_option); /* facade32.rs:330-338 */
VectorInteropResult32 zero_interleave32(VecBuf32 *vector, int32_t factor);   /* facade32.rs:340-345 */
VectorInteropResult32 fft_shift32(VecBuf32 *vector);                         /* facade32.rs:963-965 */
VectorInteropResult32 ifft_shift32(VecBuf32 *vector);                        /* facade32.rs:967-969 */
VectorInteropResult32 mirror32(VecBuf32 *vector);                            /* facade32.rs:959-961 */
VectorInteropResult32 apply_window32(VecBuf32 *vector, int32_t window);      /* facade32.rs:980-983 */
VectorInteropResult32 unapply_window32(VecBuf32 *vector, int32_t window);    /* facade32.rs:987-994 */
VectorInteropResult32 plain_fft32(VecBuf32 *vector);                         /* facade32.rs:672-674 */
VectorInteropResult32 plain_ifft32(VecBuf32 *vector);                        /* facade32.rs:682-684 */
VectorInteropResult32 fft32(VecBuf32 *vector);                               /* facade32.rs:934-936 */
VectorInteropResult32 ifft32(VecBuf32 *vector);                              /* facade32.rs:944-946 */
VectorInteropResult32 windowed_fft32(VecBuf32 *vector, int32_t window);      /* facade32.rs:997-1000 */
VectorInteropResult32 windowed_ifft32(VecBuf32 *vector, int32_t window);     /* facade32.rs:1011-1014 */
VectorInteropResult32 convolve_signal32(VecBuf32 *vector, const VecBuf32 *impulse_response); /* facade32.rs:1171-1176 */
VectorInteropResult32 interpolatef32(VecBuf32 *vector, int32_t impulse_response, float rolloff,
                                     float interpolation_factor, float delay, size_t conv_len); /* :1334-1348 */

/* FFT-domain interpolation family and the symmetric (real, odd-length) transforms */
VectorInteropResult32 interpolatei32(VecBuf32 *vector, int32_t frequency_response, float rolloff,
                                     int32_t interpolation_factor);            /* facade32.rs:1426-1434 */
VectorInteropResult32 interpolate32(VecBuf32 *vector, int32_t frequency_response, float rolloff,
                                    size_t dest_points, float delay);          /* facade32.rs:1378-1387 */
VectorInteropResult32 interpft32(VecBuf32 *vector, size_t dest_points);        /* facade32.rs:1390-1395 */
VectorInteropResult32 decimatei32(VecBuf32 *vector, uint32_t decimation_factor, uint32_t delay); /* facade32.rs:1147-1153 */
VectorInteropResult32 multiply_frequency_response32(VecBuf32 *vector, int32_t frequency_response,
                                                    float rolloff, float ratio); /* facade32.rs:1293-1301 */
VectorInteropResult32 plain_sfft32(VecBuf32 *vector);                          /* facade32.rs:677-679 */
VectorInteropResult32 sfft32(VecBuf32 *vector);                                /* facade32.rs:939-941 */
VectorInteropResult32 windowed_sfft32(VecBuf32 *vector, int32_t window);       /* facade32.rs:1004-1007 */
VectorInteropResult32 plain_sifft32(VecBuf32 *vector);                         /* facade32.rs:949-951 */
VectorInteropResult32 sifft32(VecBuf32 *vector);                               /* facade32.rs:954-956 */
VectorInteropResult32 windowed_sifft32(VecBuf32 *vector, int32_t window);      /* facade32.rs:1018-1024 */

/* Correlation, function convolution, real interpolation, wrap-around binary ops, callback variants.
 * Callbacks (interop/src/lib.rs:245-377) cannot run on the device: the host samples them once into a
 * table (window: every point, or the first half mirrored when is_symmetric; convolution: 2*len+1
 * weights; frequency response: one value per bin) and a device kernel applies the table. */
typedef float (*bdsp_window_fn32)(const void *window_data, size_t n, size_t length);   /* lib.rs:306-311 */
typedef float (*bdsp_real_fn32)(const void *function_data, float x);                     /* lib.rs:245-250 */
VecBuf32 *new_with_detailed_performance_options32(int32_t is_complex, int32_t domain, float init_value,
        size_t length, float delta, size_t core_limit, size_t med_dual_core_threshold,
        size_t med_multi_core_threshold, size_t large_dual_core_threshold,
        size_t large_multi_core_threshold);                                         /* facade32.rs:70-102 (options ignored) */
void set_value32(VecBuf32 *vector, size_t index, float value);                        /* facade32.rs:110-112 */
size_t get_allocated_len32(const VecBuf32 *vector);                                 /* facade32.rs:168-170 */
const float *complex_data32(VecBuf32 *vector);  /* facade32.rs:163-165; interleaved pairs, host mirror like data32 */
VectorInteropResult32 complex_divide32(VecBuf32 *vector, float re, float im);           /* facade32.rs:550-556 */
VectorInteropResult32 add_vector32(VecBuf32 *vector, const VecBuf32 *operand);      /* facade32.rs:704-709 */
VectorInteropResult32 sub_vector32(VecBuf32 *vector, const VecBuf32 *operand);      /* facade32.rs:712-717 */
VectorInteropResult32 div_vector32(VecBuf32 *vector, const VecBuf32 *operand);      /* facade32.rs:720-725 */
VectorInteropResult32 mul_vector32(VecBuf32 *vector, const VecBuf32 *operand);      /* facade32.rs:728-733 */
VectorInteropResult32 add_smaller_vector32(VecBuf32 *vector, const VecBuf32 *operand); /* facade32.rs:736-741 */
VectorInteropResult32 sub_smaller_vector32(VecBuf32 *vector, const VecBuf32 *operand); /* facade32.rs:744-749 */
VectorInteropResult32 div_smaller_vector32(VecBuf32 *vector, const VecBuf32 *operand); /* facade32.rs:752-757 */
VectorInteropResult32 mul_smaller_vector32(VecBuf32 *vector, const VecBuf32 *operand); /* facade32.rs:760-765 */
VectorInteropResult32 prepare_argument32(VecBuf32 *vector);                         /* facade32.rs:1156-1158 */
VectorInteropResult32 prepare_argument_padded32(VecBuf32 *vector);                  /* facade32.rs:1161-1163 */
VectorInteropResult32 correlate32(VecBuf32 *vector, const VecBuf32 *other);         /* facade32.rs:1166-1168 */
VectorInteropResult32 convolve32(VecBuf32 *vector, int32_t impulse_response, float rolloff, float ratio,
                                 size_t len);                                       /* facade32.rs:1231-1240 */
VectorInteropResult32 convolve_real32(VecBuf32 *vector, bdsp_real_fn32 impulse_response,
                                      const void *impulse_response_data, bool is_symmetric, float ratio,
                                      size_t len);                                  /* facade32.rs:1183-1203 */
VectorInteropResult32 multiply_frequency_response_real32(VecBuf32 *vector, bdsp_real_fn32 frequency_response,
                                      const void *frequency_response_data, bool is_symmetric,
                                      float ratio);                                   /* facade32.rs:1247-1262 */
/* Getters into a second vector (facade32.rs:564-668).  The source handle is CONSUMED (the reference takes it
 * by value), the destination is resized to `points` reals; like the reference these return 9 on success
 * (convert_void, interop/src/lib.rs:100-105) -- a quirk kept for link compatibility. */
int32_t get_real32(VecBuf32 *vector, VecBuf32 *destination);              /* facade32.rs:652-654 */
int32_t get_imag32(VecBuf32 *vector, VecBuf32 *destination);              /* facade32.rs:657-659 */
int32_t get_magnitude32(VecBuf32 *vector, VecBuf32 *destination);         /* facade32.rs:564-566 */
int32_t get_magnitude_squared32(VecBuf32 *vector, VecBuf32 *destination); /* facade32.rs:569-571 */
int32_t get_phase32(VecBuf32 *vector, VecBuf32 *destination);             /* facade32.rs:667-669 */
VectorInteropResult32 interpolate_lin32(VecBuf32 *vector, float interpolation_factor, float delay);     /* facade32.rs:1437-1443 */
VectorInteropResult32 interpolate_hermite32(VecBuf32 *vector, float interpolation_factor, float delay); /* facade32.rs:1446-1452 */
VectorInteropResult32 apply_custom_window32(VecBuf32 *vector, bdsp_window_fn32 window, const void *window_data,
                                            bool is_symmetric);                     /* facade32.rs:1030-1044 */
VectorInteropResult32 unapply_custom_window32(VecBuf32 *vector, bdsp_window_fn32 window, const void *window_data,
                                              bool is_symmetric);                   /* facade32.rs:1049-1063 */
VectorInteropResult32 windowed_custom_fft32(VecBuf32 *vector, bdsp_window_fn32 window, const void *window_data,
                                            bool is_symmetric);                     /* facade32.rs:1068-1082 */
VectorInteropResult32 windowed_custom_sfft32(VecBuf32 *vector, bdsp_window_fn32 window, const void *window_data,
                                             bool is_symmetric);                    /* facade32.rs:1087-1101 */
VectorInteropResult32 windowed_custom_ifft32(VecBuf32 *vector, bdsp_window_fn32 window, const void *window_data,
                                             bool is_symmetric);                    /* facade32.rs:1106-1120 */
VectorInteropResult32 windowed_custom_sifft32(VecBuf32 *vector, bdsp_window_fn32 window, const void *window_data,
                                              bool is_symmetric);                   /* facade32.rs:1125-1139 */

VecBuf64 *new64(int32_t is_complex, int32_t domain, double init_value, size_t length, double delta);
VecBuf64 *new_with_performance_options64(int32_t is_complex, int32_t domain, double init_value,
                                         size_t length, double delta, size_t core_limit,
                                         int early_temp_allocation);
void delete_vector64(VecBuf64 *vector);
VecBuf64 *clone64(VecBuf64 *vector);
VecBuf64 *bdsp_hip_vec_clone64(const VecBuf64 *vector);
double get_value64(const VecBuf64 *vector, size_t index);
size_t get_len64(const VecBuf64 *vector);
size_t get_points64(const VecBuf64 *vector);
double get_delta64(const VecBuf64 *vector);
int32_t is_complex64(const VecBuf64 *vector);
int32_t get_domain64(const VecBuf64 *vector);
const double *data64(VecBuf64 *vector);
VectorInteropResult64 overwrite_data64(VecBuf64 *vector, const double *data, size_t len);
void set_len64(VecBuf64 *vector, size_t len);
VectorInteropResult64 real_offset64(VecBuf64 *vector, double value);
VectorInteropResult64 real_scale64(VecBuf64 *vector, double value);
VectorInteropResult64 complex_offset64(VecBuf64 *vector, double re, double im);
VectorInteropResult64 complex_scale64(VecBuf64 *vector, double re, double im);
VectorInteropResult64 add64(VecBuf64 *vector, const VecBuf64 *operand);
VectorInteropResult64 sub64(VecBuf64 *vector, const VecBuf64 *operand);
VectorInteropResult64 mul64(VecBuf64 *vector, const VecBuf64 *operand);
VectorInteropResult64 div64(VecBuf64 *vector, const VecBuf64 *operand);
VectorInteropResult64 conj64(VecBuf64 *vector);
VectorInteropResult64 multiply_complex_exponential64(VecBuf64 *vector, double a, double b);
VectorInteropResult64 magnitude64(VecBuf64 *vector);
VectorInteropResult64 magnitude_squared64(VecBuf64 *vector);
VectorInteropResult64 to_real64(VecBuf64 *vector);
VectorInteropResult64 to_imag64(VecBuf64 *vector);
VectorInteropResult64 phase64(VecBuf64 *vector);
VectorInteropResult64 to_complex64(VecBuf64 *vector);
VectorInteropResult64 reverse64(VecBuf64 *vector);
VectorInteropResult64 swap_halves64(VecBuf64 *vector);
VectorInteropResult64 zero_pad64(VecBuf64 *vector, size_t points, int32_t padding_option);
VectorInteropResult64 zero_interleave64(VecBuf64 *vector, int32_t factor);
VectorInteropResult64 fft_shift64(VecBuf64 *vector);
VectorInteropResult64 ifft_shift64(VecBuf64 *vector);
VectorInteropResult64 mirror64(VecBuf64 *vector);
VectorInteropResult64 apply_window64(VecBuf64 *vector, int32_t window);
VectorInteropResult64 unapply_window64(VecBuf64 *vector, int32_t window);
VectorInteropResult64 plain_fft64(VecBuf64 *vector);
VectorInteropResult64 plain_ifft64(VecBuf64 *vector);
VectorInteropResult64 fft64(VecBuf64 *vector);
VectorInteropResult64 ifft64(VecBuf64 *vector);
VectorInteropResult64 windowed_fft64(VecBuf64 *vector, int32_t window);
VectorInteropResult64 windowed_ifft64(VecBuf64 *vector, int32_t window);
VectorInteropResult64 convolve_signal64(VecBuf64 *vector, const VecBuf64 *impulse_response);
VectorInteropResult64 interpolatef64(VecBuf64 *vector, int32_t impulse_response, double rolloff,
                                     double interpolation_factor, double delay, size_t conv_len);

VectorInteropResult64 interpolatei64(VecBuf64 *vector, int32_t frequency_response, double rolloff,
                                     int32_t interpolation_factor);
VectorInteropResult64 interpolate64(VecBuf64 *vector, int32_t frequency_response, double rolloff,
                                    size_t dest_points, double delay);
VectorInteropResult64 interpft64(VecBuf64 *vector, size_t dest_points);
VectorInteropResult64 decimatei64(VecBuf64 *vector, uint32_t decimation_factor, uint32_t delay);
VectorInteropResult64 multiply_frequency_response64(VecBuf64 *vector, int32_t frequency_response,
                                                    double rolloff, double ratio);
VectorInteropResult64 plain_sfft64(VecBuf64 *vector);
VectorInteropResult64 sfft64(VecBuf64 *vector);
VectorInteropResult64 windowed_sfft64(VecBuf64 *vector, int32_t window);
VectorInteropResult64 plain_sifft64(VecBuf64 *vector);
VectorInteropResult64 sifft64(VecBuf64 *vector);
VectorInteropResult64 windowed_sifft64(VecBuf64 *vector, int32_t window);

/* Correlation, function convolution, real interpolation, wrap-around binary ops, callback variants.
 * Callbacks (interop/src/lib.rs:245-377) cannot run on the device: the host samples them once into a
 * table (window: every point, or the first half mirrored when is_symmetric; convolution: 2*len+1
 * weights; frequency response: one value per bin) and a device kernel applies the table. */
typedef double (*bdsp_window_fn64)(const void *window_data, size_t n, size_t length);   /* lib.rs:306-311 */
typedef double (*bdsp_real_fn64)(const void *function_data, double x);                     /* lib.rs:245-250 */
VecBuf64 *new_with_detailed_performance_options64(int32_t is_complex, int32_t domain, double init_value,
        size_t length, double delta, size_t core_limit, size_t med_dual_core_threshold,
        size_t med_multi_core_threshold, size_t large_dual_core_threshold,
        size_t large_multi_core_threshold);                                         /* facade32.rs:70-102 (options ignored) */
void set_value64(VecBuf64 *vector, size_t index, double value);                        /* facade32.rs:110-112 */
size_t get_allocated_len64(const VecBuf64 *vector);                                 /* facade32.rs:168-170 */
const double *complex_data64(VecBuf64 *vector);  /* facade32.rs:163-165; interleaved pairs, host mirror like data64 */
VectorInteropResult64 complex_divide64(VecBuf64 *vector, double re, double im);           /* facade32.rs:550-556 */
VectorInteropResult64 add_vector64(VecBuf64 *vector, const VecBuf64 *operand);      /* facade32.rs:704-709 */
VectorInteropResult64 sub_vector64(VecBuf64 *vector, const VecBuf64 *operand);      /* facade32.rs:712-717 */
VectorInteropResult64 div_vector64(VecBuf64 *vector, const VecBuf64 *operand);      /* facade32.rs:720-725 */
VectorInteropResult64 mul_vector64(VecBuf64 *vector, const VecBuf64 *operand);      /* facade32.rs:728-733 */
VectorInteropResult64 add_smaller_vector64(VecBuf64 *vector, const VecBuf64 *operand); /* facade32.rs:736-741 */
VectorInteropResult64 sub_smaller_vector64(VecBuf64 *vector, const VecBuf64 *operand); /* facade32.rs:744-749 */
VectorInteropResult64 div_smaller_vector64(VecBuf64 *vector, const VecBuf64 *operand); /* facade32.rs:752-757 */
VectorInteropResult64 mul_smaller_vector64(VecBuf64 *vector, const VecBuf64 *operand); /* facade32.rs:760-765 */
VectorInteropResult64 prepare_argument64(VecBuf64 *vector);                         /* facade32.rs:1156-1158 */
VectorInteropResult64 prepare_argument_padded64(VecBuf64 *vector);                  /* facade32.rs:1161-1163 */
VectorInteropResult64 correlate64(VecBuf64 *vector, const VecBuf64 *other);         /* facade32.rs:1166-1168 */
VectorInteropResult64 convolve64(VecBuf64 *vector, int32_t impulse_response, double rolloff, double ratio,
                                 size_t len);                                       /* facade32.rs:1231-1240 */
VectorInteropResult64 convolve_real64(VecBuf64 *vector, bdsp_real_fn64 impulse_response,
                                      const void *impulse_response_data, bool is_symmetric, double ratio,
                                      size_t len);                                  /* facade32.rs:1183-1203 */
VectorInteropResult64 multiply_frequency_response_real64(VecBuf64 *vector, bdsp_real_fn64 frequency_response,
                                      const void *frequency_response_data, bool is_symmetric,
                                      double ratio);                                   /* facade32.rs:1247-1262 */
/* Getters into a second vector (facade32.rs:564-668).  The source handle is CONSUMED (the reference takes it
 * by value), the destination is resized to `points` reals; like the reference these return 9 on success
 * (convert_void, interop/src/lib.rs:100-105) -- a quirk kept for link compatibility. */
int32_t get_real64(VecBuf64 *vector, VecBuf64 *destination);              /* facade32.rs:652-654 */
int32_t get_imag64(VecBuf64 *vector, VecBuf64 *destination);              /* facade32.rs:657-659 */
int32_t get_magnitude64(VecBuf64 *vector, VecBuf64 *destination);         /* facade32.rs:564-566 */
int32_t get_magnitude_squared64(VecBuf64 *vector, VecBuf64 *destination); /* facade32.rs:569-571 */
int32_t get_phase64(VecBuf64 *vector, VecBuf64 *destination);             /* facade32.rs:667-669 */
VectorInteropResult64 interpolate_lin64(VecBuf64 *vector, double interpolation_factor, double delay);     /* facade32.rs:1437-1443 */
VectorInteropResult64 interpolate_hermite64(VecBuf64 *vector, double interpolation_factor, double delay); /* facade32.rs:1446-1452 */
VectorInteropResult64 apply_custom_window64(VecBuf64 *vector, bdsp_window_fn64 window, const void *window_data,
                                            bool is_symmetric);                     /* facade32.rs:1030-1044 */
VectorInteropResult64 unapply_custom_window64(VecBuf64 *vector, bdsp_window_fn64 window, const void *window_data,
                                              bool is_symmetric);                   /* facade32.rs:1049-1063 */
VectorInteropResult64 windowed_custom_fft64(VecBuf64 *vector, bdsp_window_fn64 window, const void *window_data,
                                            bool is_symmetric);                     /* facade32.rs:1068-1082 */
VectorInteropResult64 windowed_custom_sfft64(VecBuf64 *vector, bdsp_window_fn64 window, const void *window_data,
                                             bool is_symmetric);                    /* facade32.rs:1087-1101 */
VectorInteropResult64 windowed_custom_ifft64(VecBuf64 *vector, bdsp_window_fn64 window, const void *window_data,
                                             bool is_symmetric);                    /* facade32.rs:1106-1120 */
VectorInteropResult64 windowed_custom_sifft64(VecBuf64 *vector, bdsp_window_fn64 window, const void *window_data,
                                              bool is_symmetric);                   /* facade32.rs:1125-1139 */

/* Device pointer of the handle's live buffer (valid until the next mutating call); lets the
 * batch driver feed RCCL without a host round trip.  No reference counterpart. */
void *bdsp_hip_vec_device_ptr32(VecBuf32 *vector);
void *bdsp_hip_vec_device_ptr64(VecBuf64 *vector);

/* Statistics, sums and dot products (interop/src/facade32.rs:193-327, 846-931; vector/src/vector_types/general/
 * statistics.rs, dot_products.rs).  One pass over the vector on the device (sums accumulate in double), the small
 * result comes back by value.  Minimum / maximum: first occurrence, complex values ordered by norm(); the complex
 * `rms` is sqrt(sum(z*z)/n) -- a complex number, as in the reference (statistics.rs:331, 344).  The `real_*` entry
 * points walk all interleaved scalars of a complex vector, the `complex_*` ones walk pairs.  `*_prec*` variants
 * return double-precision results (the reference uses compensated summation there). */
typedef struct { float re, im; } bdsp_complex32;   /* num_complex::Complex32, #[repr(C)] */
typedef struct { double re, im; } bdsp_complex64;
/* #[repr(C)] Statistics<T>  (statistics.rs:11-31) */
typedef struct { float sum; size_t count; float average, rms, min; size_t min_index; float max; size_t max_index; } Statistics32;
typedef struct { double sum; size_t count; double average, rms, min; size_t min_index; double max; size_t max_index; } Statistics64;
typedef struct { bdsp_complex32 sum; size_t count; bdsp_complex32 average, rms, min; size_t min_index; bdsp_complex32 max; size_t max_index; } ComplexStatistics32;
typedef struct { bdsp_complex64 sum; size_t count; bdsp_complex64 average, rms, min; size_t min_index; bdsp_complex64 max; size_t max_index; } ComplexStatistics64;
/* #[repr(C)] ScalarInteropResult<T> { result_code, result }  (interop/src/lib.rs:229-242) */
typedef struct { int32_t result_code; float result; } ScalarInteropResult32;
typedef struct { int32_t result_code; double result; } ScalarInteropResult64;
typedef struct { int32_t result_code; bdsp_complex32 result; } ComplexScalarInteropResult32;
typedef struct { int32_t result_code; bdsp_complex64 result; } ComplexScalarInteropResult64;
Statistics32 real_statistics32(const VecBuf32 *vector);                          /* facade32.rs:223-226 */
ComplexStatistics32 complex_statistics32(const VecBuf32 *vector);                /* facade32.rs:229-232 */
float real_sum32(const VecBuf32 *vector);                                          /* facade32.rs:235-237 */
float real_sum_sq32(const VecBuf32 *vector);                                       /* facade32.rs:240-242 */
bdsp_complex32 complex_sum32(const VecBuf32 *vector);                            /* facade32.rs:245-247 */
bdsp_complex32 complex_sum_sq32(const VecBuf32 *vector);                         /* facade32.rs:250-252 */
ScalarInteropResult32 real_dot_product32(const VecBuf32 *vector, const VecBuf32 *operand);             /* facade32.rs:193-201 */
ComplexScalarInteropResult32 complex_dot_product32(const VecBuf32 *vector, const VecBuf32 *operand);   /* facade32.rs:204-220 */
Statistics64 real_statistics_prec32(const VecBuf32 *vector);                     /* facade32.rs:292-295 */
ComplexStatistics64 complex_statistics_prec32(const VecBuf32 *vector);           /* facade32.rs:298-301 */
double real_sum_prec32(const VecBuf32 *vector);                                  /* facade32.rs:304-306 */
double real_sum_sq_prec32(const VecBuf32 *vector);                               /* facade32.rs:309-311 */
bdsp_complex64 complex_sum_prec32(const VecBuf32 *vector);                       /* facade32.rs:314-316 */
bdsp_complex64 complex_sum_sq_prec32(const VecBuf32 *vector);                    /* facade32.rs:319-321 */
ScalarInteropResult64 real_dot_product_prec32(const VecBuf32 *vector, const VecBuf32 *operand);            /* facade32.rs:254-270 */
ComplexScalarInteropResult64 complex_dot_product_prec32(const VecBuf32 *vector, const VecBuf32 *operand);  /* facade32.rs:273-289 */
/* statistics_split (statistics.rs:389-426): element j goes to bucket j % len with index j / len; len <= 16, else code 7 */
int32_t real_statistics_split32(const VecBuf32 *vector, Statistics32 *data, size_t len);               /* facade32.rs:848-864 */
int32_t complex_statistics_split32(const VecBuf32 *vector, ComplexStatistics32 *data, size_t len);     /* facade32.rs:867-886 */
int32_t real_statistics_split_prec32(const VecBuf32 *vector, Statistics64 *data, size_t len);          /* facade32.rs:889-907 */
int32_t complex_statistics_split_prec32(const VecBuf32 *vector, ComplexStatistics64 *data, size_t len);/* facade32.rs:910-931 */

Statistics64 real_statistics64(const VecBuf64 *vector);                          /* facade32.rs:223-226 */
ComplexStatistics64 complex_statistics64(const VecBuf64 *vector);                /* facade32.rs:229-232 */
double real_sum64(const VecBuf64 *vector);                                          /* facade32.rs:235-237 */
double real_sum_sq64(const VecBuf64 *vector);                                       /* facade32.rs:240-242 */
bdsp_complex64 complex_sum64(const VecBuf64 *vector);                            /* facade32.rs:245-247 */
bdsp_complex64 complex_sum_sq64(const VecBuf64 *vector);                         /* facade32.rs:250-252 */
ScalarInteropResult64 real_dot_product64(const VecBuf64 *vector, const VecBuf64 *operand);             /* facade32.rs:193-201 */
ComplexScalarInteropResult64 complex_dot_product64(const VecBuf64 *vector, const VecBuf64 *operand);   /* facade32.rs:204-220 */
Statistics64 real_statistics_prec64(const VecBuf64 *vector);                     /* facade32.rs:292-295 */
ComplexStatistics64 complex_statistics_prec64(const VecBuf64 *vector);           /* facade32.rs:298-301 */
double real_sum_prec64(const VecBuf64 *vector);                                  /* facade32.rs:304-306 */
double real_sum_sq_prec64(const VecBuf64 *vector);                               /* facade32.rs:309-311 */
bdsp_complex64 complex_sum_prec64(const VecBuf64 *vector);                       /* facade32.rs:314-316 */
bdsp_complex64 complex_sum_sq_prec64(const VecBuf64 *vector);                    /* facade32.rs:319-321 */
ScalarInteropResult64 real_dot_product_prec64(const VecBuf64 *vector, const VecBuf64 *operand);            /* facade32.rs:254-270 */
ComplexScalarInteropResult64 complex_dot_product_prec64(const VecBuf64 *vector, const VecBuf64 *operand);  /* facade32.rs:273-289 */
/* statistics_split (statistics.rs:389-426): element j goes to bucket j % len with index j / len; len <= 16, else code 7 */
int32_t real_statistics_split64(const VecBuf64 *vector, Statistics64 *data, size_t len);               /* facade32.rs:848-864 */
int32_t complex_statistics_split64(const VecBuf64 *vector, ComplexStatistics64 *data, size_t len);     /* facade32.rs:867-886 */
int32_t real_statistics_split_prec64(const VecBuf64 *vector, Statistics64 *data, size_t len);          /* facade32.rs:889-907 */
int32_t complex_statistics_split_prec64(const VecBuf64 *vector, ComplexStatistics64 *data, size_t len);/* facade32.rs:910-931 */

/* ----------------------------------------------------------------------------------------
 * Per-element math family, differences / running sums, phase wrapping, real<->complex pairs, split / merge,
 * host callbacks (trigonometry_and_powers.rs, real_ops.rs, diff_sum.rs, complex_to_real.rs:674-770,
 * data_reorganization.rs:484-555, mapping.rs).  TrigOps / PowerOps work on real and complex vectors (complex
 * functions as in num-complex 0.4); abs / wrap / unwrap / the *_approx family poison a complex vector.  The
 * "approximated" functions are the standard ones, as in the reference's build without explicit SIMD
 * (simd_extensions/approx_fallback.rs).  cum_sum carries the running sum in double.
 * glibc's <math.h> declares powf32 / expf32 / powf64 / expf64 itself (the _Float32 / _Float64 functions of
 * ISO/IEC TS 18661-3) and the reference's facade uses the very same names for different functions: the C
 * declarations below carry a bdsp_ prefix and bind to the facade's symbol name, so the library still exports
 * `powf32` etc. for ctypes / Rust callers and this header can be included next to <math.h>.
 * -------------------------------------------------------------------------------------- */
#define BDSP_FACADE_SYMBOL(name) __asm__(#name)
VectorInteropResult32 diff32(VecBuf32 *vector);                        /* facade32.rs:348-350 */
VectorInteropResult32 diff_with_start32(VecBuf32 *vector);             /* facade32.rs:353-355 */
VectorInteropResult32 cum_sum32(VecBuf32 *vector);                     /* facade32.rs:358-360 */
VectorInteropResult32 abs32(VecBuf32 *vector);                         /* facade32.rs:373-375 */
VectorInteropResult32 sqrt32(VecBuf32 *vector);                        /* facade32.rs:378-380 */
VectorInteropResult32 square32(VecBuf32 *vector);                      /* facade32.rs:383-385 */
VectorInteropResult32 root32(VecBuf32 *vector, float value);           /* facade32.rs:388-390 */
VectorInteropResult32 bdsp_powf32(VecBuf32 *vector, float value) BDSP_FACADE_SYMBOL(powf32);           /* facade32.rs:393-395 */
VectorInteropResult32 ln32(VecBuf32 *vector);                          /* facade32.rs:398-400 */
VectorInteropResult32 exp32(VecBuf32 *vector);                         /* facade32.rs:403-405 */
VectorInteropResult32 log32(VecBuf32 *vector, float value);            /* facade32.rs:408-410 */
VectorInteropResult32 bdsp_expf32(VecBuf32 *vector, float value) BDSP_FACADE_SYMBOL(expf32);           /* facade32.rs:413-415 */
VectorInteropResult32 sin32(VecBuf32 *vector);                         /* facade32.rs:423-425 */
VectorInteropResult32 cos32(VecBuf32 *vector);                         /* facade32.rs:428-430 */
VectorInteropResult32 tan32(VecBuf32 *vector);
VectorInteropResult32 asin32(VecBuf32 *vector);
VectorInteropResult32 acos32(VecBuf32 *vector);
VectorInteropResult32 atan32(VecBuf32 *vector);
VectorInteropResult32 sinh32(VecBuf32 *vector);
VectorInteropResult32 cosh32(VecBuf32 *vector);
VectorInteropResult32 tanh32(VecBuf32 *vector);
VectorInteropResult32 asinh32(VecBuf32 *vector);
VectorInteropResult32 acosh32(VecBuf32 *vector);
VectorInteropResult32 atanh32(VecBuf32 *vector);                       /* facade32.rs:433-479 */
VectorInteropResult32 ln_approx32(VecBuf32 *vector);                   /* facade32.rs:482-484 */
VectorInteropResult32 exp_approx32(VecBuf32 *vector);
VectorInteropResult32 sin_approx32(VecBuf32 *vector);
VectorInteropResult32 cos_approx32(VecBuf32 *vector);
VectorInteropResult32 log_approx32(VecBuf32 *vector, float value);
VectorInteropResult32 expf_approx32(VecBuf32 *vector, float value);
VectorInteropResult32 powf_approx32(VecBuf32 *vector, float value);    /* facade32.rs:487-514 */
VectorInteropResult32 wrap32(VecBuf32 *vector, float value);           /* facade32.rs:517-519 */
VectorInteropResult32 unwrap32(VecBuf32 *vector, float value);         /* facade32.rs:522-524; sequential recurrence */
/* callbacks are host code: the vector makes one host round trip, one call per element in index order */
VectorInteropResult32 map_inplace_real32(VecBuf32 *vector, float (*map)(float, size_t));                  /* facade32.rs:594-600 */
VectorInteropResult32 map_inplace_complex32(VecBuf32 *vector, bdsp_complex32 (*map)(bdsp_complex32, size_t)); /* facade32.rs:603-609 */
typedef struct { int32_t result_code; const void *result; } PointerInteropResult;  /* ScalarInteropResult<*const c_void> */
PointerInteropResult map_aggregate_real32(const VecBuf32 *vector, const void *(*map)(float, size_t),
                                          const void *(*aggregate)(const void *, const void *));       /* facade32.rs:614-629 */
PointerInteropResult map_aggregate_complex32(const VecBuf32 *vector, const void *(*map)(bdsp_complex32, size_t),
                                             const void *(*aggregate)(const void *, const void *));    /* facade32.rs:634-649 */
/* the source handle is CONSUMED, the answer is convert_void(Ok) = 9 (interop/src/lib.rs:100-105) */
int32_t get_real_imag32(VecBuf32 *vector, VecBuf32 *real, VecBuf32 *imag);                              /* facade32.rs:768-774 */
int32_t get_mag_phase32(VecBuf32 *vector, VecBuf32 *mag, VecBuf32 *phase);                              /* facade32.rs:777-783 */
VectorInteropResult32 set_real_imag32(VecBuf32 *vector, const VecBuf32 *real, const VecBuf32 *imag);    /* facade32.rs:786-792 */
VectorInteropResult32 set_mag_phase32(VecBuf32 *vector, const VecBuf32 *mag, const VecBuf32 *phase);    /* facade32.rs:795-801 */
int32_t split_into32(const VecBuf32 *vector, VecBuf32 **targets, size_t len);                           /* facade32.rs:804-811; 9 = ok */
VectorInteropResult32 merge32(VecBuf32 *vector, VecBuf32 *const *sources, size_t len);                  /* facade32.rs:814-824 */
typedef bdsp_complex32 (*bdsp_complex_fn32)(const void *function_data, float x);                        /* lib.rs:279-284 */
VectorInteropResult32 convolve_complex32(VecBuf32 *vector, bdsp_complex_fn32 impulse_response,
                                         const void *impulse_response_data, bool is_symmetric, float ratio,
                                         size_t len);                                                   /* facade32.rs:1206-1222 */
VectorInteropResult32 multiply_frequency_response_complex32(VecBuf32 *vector, bdsp_complex_fn32 frequency_response,
                                         const void *frequency_response_data, bool is_symmetric,
                                         float ratio);                                                  /* facade32.rs:1269-1284 */
VectorInteropResult32 interpolatef_custom32(VecBuf32 *vector, bdsp_real_fn32 impulse_response,
                                            const void *impulse_response_data, bool is_symmetric,
                                            float interpolation_factor, float delay, size_t len);       /* facade32.rs:1308-1326 */
VectorInteropResult32 interpolate_custom32(VecBuf32 *vector, bdsp_real_fn32 frequency_response,
                                           const void *frequency_response_data, bool is_symmetric,
                                           size_t dest_points, float delay);                            /* facade32.rs:1353-1369 */
VectorInteropResult32 interpolatei_custom32(VecBuf32 *vector, bdsp_real_fn32 frequency_response,
                                            const void *frequency_response_data, bool is_symmetric,
                                            int32_t interpolation_factor);                              /* facade32.rs:1402-1417 */

VectorInteropResult64 diff64(VecBuf64 *vector);                        /* facade32.rs:348-350 */
VectorInteropResult64 diff_with_start64(VecBuf64 *vector);             /* facade32.rs:353-355 */
VectorInteropResult64 cum_sum64(VecBuf64 *vector);                     /* facade32.rs:358-360 */
VectorInteropResult64 abs64(VecBuf64 *vector);                         /* facade32.rs:373-375 */
VectorInteropResult64 sqrt64(VecBuf64 *vector);                        /* facade32.rs:378-380 */
VectorInteropResult64 square64(VecBuf64 *vector);                      /* facade32.rs:383-385 */
VectorInteropResult64 root64(VecBuf64 *vector, double value);           /* facade32.rs:388-390 */
VectorInteropResult64 bdsp_powf64(VecBuf64 *vector, double value) BDSP_FACADE_SYMBOL(powf64);           /* facade32.rs:393-395 */
VectorInteropResult64 ln64(VecBuf64 *vector);                          /* facade32.rs:398-400 */
VectorInteropResult64 exp64(VecBuf64 *vector);                         /* facade32.rs:403-405 */
VectorInteropResult64 log64(VecBuf64 *vector, double value);            /* facade32.rs:408-410 */
VectorInteropResult64 bdsp_expf64(VecBuf64 *vector, double value) BDSP_FACADE_SYMBOL(expf64);           /* facade32.rs:413-415 */
VectorInteropResult64 sin64(VecBuf64 *vector);                         /* facade32.rs:423-425 */
VectorInteropResult64 cos64(VecBuf64 *vector);                         /* facade32.rs:428-430 */
VectorInteropResult64 tan64(VecBuf64 *vector);
VectorInteropResult64 asin64(VecBuf64 *vector);
VectorInteropResult64 acos64(VecBuf64 *vector);
VectorInteropResult64 atan64(VecBuf64 *vector);
VectorInteropResult64 sinh64(VecBuf64 *vector);
VectorInteropResult64 cosh64(VecBuf64 *vector);
VectorInteropResult64 tanh64(VecBuf64 *vector);
VectorInteropResult64 asinh64(VecBuf64 *vector);
VectorInteropResult64 acosh64(VecBuf64 *vector);
VectorInteropResult64 atanh64(VecBuf64 *vector);                       /* facade32.rs:433-479 */
VectorInteropResult64 ln_approx64(VecBuf64 *vector);                   /* facade32.rs:482-484 */
VectorInteropResult64 exp_approx64(VecBuf64 *vector);
VectorInteropResult64 sin_approx64(VecBuf64 *vector);
VectorInteropResult64 cos_approx64(VecBuf64 *vector);
VectorInteropResult64 log_approx64(VecBuf64 *vector, double value);
VectorInteropResult64 expf_approx64(VecBuf64 *vector, double value);
VectorInteropResult64 powf_approx64(VecBuf64 *vector, double value);    /* facade32.rs:487-514 */
VectorInteropResult64 wrap64(VecBuf64 *vector, double value);           /* facade32.rs:517-519 */
VectorInteropResult64 unwrap64(VecBuf64 *vector, double value);         /* facade32.rs:522-524; sequential recurrence */
/* callbacks are host code: the vector makes one host round trip, one call per element in index order */
VectorInteropResult64 map_inplace_real64(VecBuf64 *vector, double (*map)(double, size_t));                  /* facade32.rs:594-600 */
VectorInteropResult64 map_inplace_complex64(VecBuf64 *vector, bdsp_complex64 (*map)(bdsp_complex64, size_t)); /* facade32.rs:603-609 */
PointerInteropResult map_aggregate_real64(const VecBuf64 *vector, const void *(*map)(double, size_t),
                                          const void *(*aggregate)(const void *, const void *));       /* facade32.rs:614-629 */
PointerInteropResult map_aggregate_complex64(const VecBuf64 *vector, const void *(*map)(bdsp_complex64, size_t),
                                             const void *(*aggregate)(const void *, const void *));    /* facade32.rs:634-649 */
/* the source handle is CONSUMED, the answer is convert_void(Ok) = 9 (interop/src/lib.rs:100-105) */
int32_t get_real_imag64(VecBuf64 *vector, VecBuf64 *real, VecBuf64 *imag);                              /* facade32.rs:768-774 */
int32_t get_mag_phase64(VecBuf64 *vector, VecBuf64 *mag, VecBuf64 *phase);                              /* facade32.rs:777-783 */
VectorInteropResult64 set_real_imag64(VecBuf64 *vector, const VecBuf64 *real, const VecBuf64 *imag);    /* facade32.rs:786-792 */
VectorInteropResult64 set_mag_phase64(VecBuf64 *vector, const VecBuf64 *mag, const VecBuf64 *phase);    /* facade32.rs:795-801 */
int32_t split_into64(const VecBuf64 *vector, VecBuf64 **targets, size_t len);                           /* facade32.rs:804-811; 9 = ok */
VectorInteropResult64 merge64(VecBuf64 *vector, VecBuf64 *const *sources, size_t len);                  /* facade32.rs:814-824 */
typedef bdsp_complex64 (*bdsp_complex_fn64)(const void *function_data, double x);                        /* lib.rs:279-284 */
VectorInteropResult64 convolve_complex64(VecBuf64 *vector, bdsp_complex_fn64 impulse_response,
                                         const void *impulse_response_data, bool is_symmetric, double ratio,
                                         size_t len);                                                   /* facade32.rs:1206-1222 */
VectorInteropResult64 multiply_frequency_response_complex64(VecBuf64 *vector, bdsp_complex_fn64 frequency_response,
                                         const void *frequency_response_data, bool is_symmetric,
                                         double ratio);                                                  /* facade32.rs:1269-1284 */
VectorInteropResult64 interpolatef_custom64(VecBuf64 *vector, bdsp_real_fn64 impulse_response,
                                            const void *impulse_response_data, bool is_symmetric,
                                            double interpolation_factor, double delay, size_t len);       /* facade32.rs:1308-1326 */
VectorInteropResult64 interpolate_custom64(VecBuf64 *vector, bdsp_real_fn64 frequency_response,
                                           const void *frequency_response_data, bool is_symmetric,
                                           size_t dest_points, double delay);                            /* facade32.rs:1353-1369 */
VectorInteropResult64 interpolatei_custom64(VecBuf64 *vector, bdsp_real_fn64 frequency_response,
                                            const void *frequency_response_data, bool is_symmetric,
                                            int32_t interpolation_factor);                              /* facade32.rs:1402-1417 */

/* Bridges for foreign-function layers that cannot describe callbacks RETURNING structs (Python ctypes): these
 * functions have the facade's callback signatures and forward to a pointer-style callback.  Pass
 * bdsp_hip_complex_fn_bridge32 as the `bdsp_complex_fn32` and a bdsp_complex_bridge32 as its function_data; for
 * map_inplace_complex32 (no data argument) register the target for the calling thread first. */
typedef struct { void (*fn)(void *ctx, float x, float *re_im_out); void *ctx; } bdsp_complex_bridge32;
typedef struct { void (*fn)(void *ctx, double x, double *re_im_out); void *ctx; } bdsp_complex_bridge64;
bdsp_complex32 bdsp_hip_complex_fn_bridge32(const void *bridge, float x);
bdsp_complex64 bdsp_hip_complex_fn_bridge64(const void *bridge, double x);
void bdsp_hip_set_map_complex_bridge32(void (*fn)(float re, float im, size_t index, float *re_im_out));
void bdsp_hip_set_map_complex_bridge64(void (*fn)(double re, double im, size_t index, double *re_im_out));
bdsp_complex32 bdsp_hip_map_complex_bridge32(bdsp_complex32 value, size_t index);
bdsp_complex64 bdsp_hip_map_complex_bridge64(bdsp_complex64 value, size_t index);

/* ========================================================================================
 * B2m -- matrix / batch API: `rows` equally long vectors in one allocation, every operation a
 *        batched launch.  The reference's matrix crate has no C facade; these entry points mirror
 *        its Rust API (matrix/src/lib.rs:195-208 row loop, matrix/src/time_freq.rs:49-530 trait
 *        forwarding, MatrixMxN::convolve_signal with a matrix of impulse responses :439-483 ->
 *        DspVec::convolve_mat, vector/src/vector_types/time_freq/mod.rs:365-453).
 *        Operations return the facade result codes (0, -1 poisoned, 1..14, <= -100 backend).
 * ======================================================================================== */
typedef struct MatBuf32 MatBuf32;
typedef struct MatBuf64 MatBuf64;
MatBuf32 *bdsp_hip_mat_new32(int32_t is_complex, int32_t domain, size_t rows, size_t row_len, float delta); /* row_len in scalars; zero filled */
void bdsp_hip_mat_delete32(MatBuf32 *m);
size_t bdsp_hip_mat_rows32(const MatBuf32 *m);        /* col_len() of the reference (number of row vectors) */
size_t bdsp_hip_mat_row_len32(const MatBuf32 *m);     /* row_len(): scalars per row */
size_t bdsp_hip_mat_row_points32(const MatBuf32 *m);
int32_t bdsp_hip_mat_is_complex32(const MatBuf32 *m);
int32_t bdsp_hip_mat_get_domain32(const MatBuf32 *m);
float bdsp_hip_mat_get_delta32(const MatBuf32 *m);
void *bdsp_hip_mat_device_ptr32(MatBuf32 *m);         /* [rows][row_len] contiguous */
int32_t bdsp_hip_mat_upload32(MatBuf32 *m, const float *data, size_t len);   /* len == rows*row_len */
int32_t bdsp_hip_mat_download32(MatBuf32 *m, float *out, size_t len);
VecBuf32 *bdsp_hip_mat_get_row32(const MatBuf32 *m, size_t row);           /* copy of one row as a vector handle */
int32_t bdsp_hip_mat_set_row32(MatBuf32 *m, size_t row, const VecBuf32 *vector);
int32_t bdsp_hip_mat_real_scale32(MatBuf32 *m, float factor);
int32_t bdsp_hip_mat_real_offset32(MatBuf32 *m, float offset);
int32_t bdsp_hip_mat_complex_scale32(MatBuf32 *m, float re, float im);
int32_t bdsp_hip_mat_conj32(MatBuf32 *m);
int32_t bdsp_hip_mat_add32(MatBuf32 *m, const MatBuf32 *other);            /* matrix (.) matrix */
int32_t bdsp_hip_mat_sub32(MatBuf32 *m, const MatBuf32 *other);
int32_t bdsp_hip_mat_mul32(MatBuf32 *m, const MatBuf32 *other);
int32_t bdsp_hip_mat_div32(MatBuf32 *m, const MatBuf32 *other);
int32_t bdsp_hip_mat_add_vector32(MatBuf32 *m, const VecBuf32 *operand);   /* every row (.) the same vector */
int32_t bdsp_hip_mat_sub_vector32(MatBuf32 *m, const VecBuf32 *operand);
int32_t bdsp_hip_mat_mul_vector32(MatBuf32 *m, const VecBuf32 *operand);
int32_t bdsp_hip_mat_div_vector32(MatBuf32 *m, const VecBuf32 *operand);
int32_t bdsp_hip_mat_magnitude32(MatBuf32 *m);
int32_t bdsp_hip_mat_magnitude_squared32(MatBuf32 *m);
int32_t bdsp_hip_mat_to_real32(MatBuf32 *m);
int32_t bdsp_hip_mat_to_imag32(MatBuf32 *m);
int32_t bdsp_hip_mat_phase32(MatBuf32 *m);
int32_t bdsp_hip_mat_plain_fft32(MatBuf32 *m);                             /* matrix/src/time_freq.rs:53-61 */
int32_t bdsp_hip_mat_fft32(MatBuf32 *m);                                   /* :63-71 */
int32_t bdsp_hip_mat_windowed_fft32(MatBuf32 *m, int32_t window);          /* :73-81 */
int32_t bdsp_hip_mat_plain_ifft32(MatBuf32 *m);                            /* :120-128 */
int32_t bdsp_hip_mat_ifft32(MatBuf32 *m);                                  /* :130-138 */
int32_t bdsp_hip_mat_windowed_ifft32(MatBuf32 *m, int32_t window);         /* :140-148 */
int32_t bdsp_hip_mat_apply_window32(MatBuf32 *m, int32_t window);
int32_t bdsp_hip_mat_unapply_window32(MatBuf32 *m, int32_t window);
int32_t bdsp_hip_mat_swap_halves32(MatBuf32 *m);
int32_t bdsp_hip_mat_fft_shift32(MatBuf32 *m);
int32_t bdsp_hip_mat_ifft_shift32(MatBuf32 *m);
int32_t bdsp_hip_mat_zero_pad32(MatBuf32 *m, size_t points, int32_t padding_option);
int32_t bdsp_hip_mat_convolve_signal32(MatBuf32 *m, const VecBuf32 *impulse_response);      /* :421-431, one filter for all rows */
int32_t bdsp_hip_mat_convolve_signal_mat32(MatBuf32 *m, const VecBuf32 *const *impulse_responses,
                                           size_t count); /* :439-483: count == rows*rows, row-major [out][in] */
int32_t bdsp_hip_mat_interpolatef32(MatBuf32 *m, int32_t impulse_response, float rolloff,
                                    float interpolation_factor, float delay, size_t conv_len);
/* interpolatef with one delay per row: row r as bdsp_hip_interpolatef on it with delays[r] (each divided by the
 * matrix's delta, as the vector call divides its delay); delta is left alone.  The launches do not depend on the row
 * count.  Codes: 7 when count is not the row count or delays is null with count > 0 (the matrix is untouched); -1 for a
 * poisoned matrix; 0 otherwise, a matrix with no rows or empty rows included.  The call uploads the delays, so it
 * cannot be captured into a HIP graph (bdsp_hip_mat_interpolatef can, once its tap table is cached). */
int32_t bdsp_hip_mat_interpolatef_delays32(MatBuf32 *m, int32_t impulse_response, float rolloff,
                                           float interpolation_factor, const float *delays, size_t count,
                                           size_t conv_len);
int32_t bdsp_hip_mat_multiply_frequency_response32(MatBuf32 *m, int32_t frequency_response, float rolloff, float ratio);
/* Per-row statistics, sums and dot products: one result per row in out[0 .. rows) (split: out[r*len + b], bucket b of
 * row r), one batched device pass.  `len` (split: `out_len`) must equal rows (rows * len), else 7; split len > 16 gives 7,
 * len 0 gives 0 and writes nothing.  Indices are within the row.  real_* walks every scalar of a row, complex_* its
 * pairs, as the vector facade.  Dot products: 4 (real_* on a complex matrix), 3 (complex_* on a real one), 2 (complex
 * operand not complex or in another domain), 7 for matrices with unequal row counts (stricter than the reference's
 * zip, as bdsp_hip_mat_add), per-row count min(row length, operand length), complex products not conjugated.
 * -1 for a poisoned matrix, results written as the vector path writes them. */
int32_t bdsp_hip_mat_real_statistics32(const MatBuf32 *m, Statistics32 *out, size_t len);                 /* matrix/src/general/statistics.rs:4-19 */
int32_t bdsp_hip_mat_complex_statistics32(const MatBuf32 *m, ComplexStatistics32 *out, size_t len);
int32_t bdsp_hip_mat_real_statistics_prec32(const MatBuf32 *m, Statistics64 *out, size_t len);             /* :240-255 */
int32_t bdsp_hip_mat_complex_statistics_prec32(const MatBuf32 *m, ComplexStatistics64 *out, size_t len);
int32_t bdsp_hip_mat_real_statistics_split32(const MatBuf32 *m, Statistics32 *out, size_t out_len, size_t len);       /* :21-36 */
int32_t bdsp_hip_mat_complex_statistics_split32(const MatBuf32 *m, ComplexStatistics32 *out, size_t out_len, size_t len);
int32_t bdsp_hip_mat_real_statistics_split_prec32(const MatBuf32 *m, Statistics64 *out, size_t out_len, size_t len);   /* :257-272 */
int32_t bdsp_hip_mat_complex_statistics_split_prec32(const MatBuf32 *m, ComplexStatistics64 *out, size_t out_len, size_t len);
int32_t bdsp_hip_mat_real_sum32(const MatBuf32 *m, float *out, size_t len);                                     /* :140-163 */
int32_t bdsp_hip_mat_real_sum_sq32(const MatBuf32 *m, float *out, size_t len);
int32_t bdsp_hip_mat_complex_sum32(const MatBuf32 *m, bdsp_complex32 *out, size_t len);
int32_t bdsp_hip_mat_complex_sum_sq32(const MatBuf32 *m, bdsp_complex32 *out, size_t len);
int32_t bdsp_hip_mat_real_sum_prec32(const MatBuf32 *m, double *out, size_t len);                           /* :376-400 */
int32_t bdsp_hip_mat_real_sum_sq_prec32(const MatBuf32 *m, double *out, size_t len);
int32_t bdsp_hip_mat_complex_sum_prec32(const MatBuf32 *m, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_complex_sum_sq_prec32(const MatBuf32 *m, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_real_dot_product32(const MatBuf32 *m, const MatBuf32 *factor, float *out, size_t len);   /* matrix/src/general/mod.rs:9-25 */
int32_t bdsp_hip_mat_complex_dot_product32(const MatBuf32 *m, const MatBuf32 *factor, bdsp_complex32 *out, size_t len);
int32_t bdsp_hip_mat_real_dot_product_prec32(const MatBuf32 *m, const MatBuf32 *factor, double *out, size_t len);    /* :153-169 */
int32_t bdsp_hip_mat_complex_dot_product_prec32(const MatBuf32 *m, const MatBuf32 *factor, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_real_dot_product_vector32(const MatBuf32 *m, const VecBuf32 *factor, float *out, size_t len);     /* :81-97 */
int32_t bdsp_hip_mat_complex_dot_product_vector32(const MatBuf32 *m, const VecBuf32 *factor, bdsp_complex32 *out, size_t len);
int32_t bdsp_hip_mat_real_dot_product_vector_prec32(const MatBuf32 *m, const VecBuf32 *factor, double *out, size_t len);   /* :225-241 */
int32_t bdsp_hip_mat_complex_dot_product_vector_prec32(const MatBuf32 *m, const VecBuf32 *factor, bdsp_complex64 *out, size_t len);
/* Cross correlation of the rows (matrix/src/time_freq.rs:208-264; correlation.rs:96-160 per row): every row behaves as
 * the vector function of the same name on that row.  prepare_argument: plain_fft of all rows, conjugated (real rows
 * become complex, delta <- points * delta; a frequency-domain matrix is poisoned, -1).  prepare_argument_padded: every
 * row Surround-padded to 2p-1 points first; 7 for p <= 1, matrix untouched.  correlate: `m` complex / time and `other`
 * complex / frequency, else `m` is poisoned and the code is 5; `other`'s row points L must exceed m's, else 7, and the
 * row counts must agree, else 7 (m unchanged both times).  Afterwards every row holds L complex points in the time
 * domain -- zero_pad(L, Surround), plain_fft, x other, plain_ifft, 1/L, swap_halves -- delta as before; `other` is
 * not modified; zero rows: 0.  One launch for L a power of two in [16, 4096], else a number of launches that does not
 * depend on the row count.  _vector: every row with ONE prepared vector (not in the reference: time_freq.rs:233-239). */
int32_t bdsp_hip_mat_prepare_argument32(MatBuf32 *m);                      /* matrix/src/time_freq.rs:208-229 */
int32_t bdsp_hip_mat_prepare_argument_padded32(MatBuf32 *m);
int32_t bdsp_hip_mat_correlate32(MatBuf32 *m, const MatBuf32 *other);        /* :241-264, row r with row r of other */
int32_t bdsp_hip_mat_correlate_vector32(MatBuf32 *m, const VecBuf32 *other); /* every row with one prepared vector */
/* Differences, running sums and phase wrapping of the rows (matrix/src/general/elementary.rs:206-225 DiffSumOps,
 * matrix/src/real.rs:69-83 ModuloOps): every row behaves as the vector function OF THE SAME NAME on that row.  (The
 * reference's matrix diff_with_start and cum_sum both forward to v.diff(), elementary.rs:214-224 -- a slip there, not
 * reproduced here.)  diff shortens every row by one point, rows that are empty stay empty; cum_sum carries the running
 * sum in double and rounds once per element, as cum_sum32/64; wrap / unwrap on a complex matrix poison it, -1, with no
 * launch (real_ops.rs:222-233).  Zero rows or empty rows: 0, no launch; -1 for a poisoned matrix.  Domain, delta and
 * number space stay.  One launch each (cum_sum: three for rows of more than 4096 points), whatever the row count. */
int32_t bdsp_hip_mat_diff32(MatBuf32 *m);
int32_t bdsp_hip_mat_diff_with_start32(MatBuf32 *m);
int32_t bdsp_hip_mat_cum_sum32(MatBuf32 *m);
int32_t bdsp_hip_mat_wrap32(MatBuf32 *m, float divisor);
int32_t bdsp_hip_mat_unwrap32(MatBuf32 *m, float divisor);
/* FFT-domain resampling and decimation of the rows (matrix/src/time_freq.rs:266-327 InterpolationOps; interpolation.rs:
 * 484-633 per row): every row behaves as the vector function OF THE SAME NAME on that row, and the arguments are the
 * vector facade's (frequency_response 0 = sinc, anything else = raised cosine(rolloff)).  Real rows stay real, complex
 * rows complex; every row gets the same new length: points * interpolation_factor, dest_points, or
 * ceil((points - delay) / decimation_factor) (0 for delay >= points).  interpolate / interpft set
 * delta <- delta / (dest_points / points), computed in the matrix's precision; interpolatei and decimatei leave delta
 * alone; domain and number space are neither checked nor changed, as in the vector functions.  Codes: interpolatei with
 * a factor <= 1: 0, matrix untouched; interpolate / interpft with dest_points == 0 or rows of zero points: 7, matrix
 * untouched; decimatei with factor 0: 7; zero rows: 0, no launch; -1 for a poisoned matrix.
 * Launches, whatever the row count: ONE when the new length is an integer multiple (>= 2) of the row length and a power
 * of two in [16, 4096] (the row is read once and written once); otherwise batched forward transform -> one spectrum
 * pass over all rows -> batched inverse transform, as many launches as those transforms take for ONE row length
 * (three for power-of-two lengths up to 4096; interpolate to the same length with delay 0 skips the spectrum pass).
 * decimatei: one launch.  Memory: the general path grows both device buffers of the matrix to
 * rows * 2 * max(points, new points) scalars before its first launch (real rows too: their spectra are complex); the
 * one-launch path and decimatei to rows * new row length.  Custom (callback) responses are not offered for matrices. */
int32_t bdsp_hip_mat_interpolatei32(MatBuf32 *m, int32_t frequency_response, float rolloff,
                                    int32_t interpolation_factor);            /* matrix/src/time_freq.rs:282-293 */
int32_t bdsp_hip_mat_interpolate32(MatBuf32 *m, int32_t frequency_response, float rolloff,
                                   size_t dest_points, float delay);          /* :295-307 */
int32_t bdsp_hip_mat_interpft32(MatBuf32 *m, size_t dest_points);             /* :309-317 */
int32_t bdsp_hip_mat_decimatei32(MatBuf32 *m, uint32_t decimation_factor, uint32_t delay); /* :319-326 */
/* Symmetric real-signal transforms of the rows, mirror and to_complex (matrix/src/time_freq.rs:83-107
 * SymmetricTimeToFrequencyDomainOperations, :144-168 SymmetricFrequencyToTimeDomainOperations, :173-177
 * FrequencyDomainOperations::mirror; time_to_freq.rs:188-298, freq_to_time.rs:180-248, freq.rs:52-83 per row): every row
 * behaves as the vector function OF THE SAME NAME on that row.  N = real points of a row, p = N/2 + 1.
 * plain_sfft / sfft / windowed_sfft: a real time matrix with odd N becomes complex / frequency with p points per row,
 * densely packed: the first p bins of what plain_fft / fft / windowed_fft leave (of the shifted forms: the negative half
 * plus DC, as sfft32), delta <- N * delta.  Not real or not time: poisoned, 5; N even or rows without points: poisoned,
 * 9; zero rows: 0, complex / frequency with no data.
 * plain_sifft / sifft / windowed_sifft: a complex frequency matrix with p points per row becomes real / time with
 * 2p - 1 points per row, delta <- (2p - 1) * delta; plain_sifft is unnormalised, sifft and windowed_sifft scale by 1/p
 * (the HALF spectrum's point count, as sifft32) and rotate the half spectrum by p/2 first, windowed_sifft divides by the
 * window last.  Not complex or not frequency: poisoned, 6.  The first bin of EVERY row (after scale and rotation) must
 * be real: a row fails if |im0| > 1e-10 and |im0| > 1e-3 * (|re0| + |re1| + |im1|) (re1 = im1 = 0 for p == 1); if any
 * row fails the whole matrix is poisoned, 8.  Zero rows or rows without points: 0, real / time with no data.
 * mirror: every row grows from p to 2p - 1 complex points, out[g] = in[g] for g < p, conj(in[2p - 1 - g]) above;
 * bit-exact; a real time-domain matrix is poisoned (-1); domain and delta stay; rows with p == 0 stay as they are (a
 * real frequency-domain matrix is read as pairs, as mirror32 reads it: 7 for rows of an odd number of scalars).
 * to_complex: every real scalar becomes (x, 0), rows double their length; a complex matrix is poisoned (-1).
 * Launches, whatever the row count: the forward forms the batched transform of ONE row length plus one crop; the
 * inverse forms one mirror launch, one 4-byte read-back of the symmetry flag (the call's only synchronisation), the
 * batched inverse transform (+ one for windowed_sifft); mirror and to_complex one.  Memory: both device buffers of the
 * matrix grow to rows * 2 * (2p - 1) scalars before the first launch. */
int32_t bdsp_hip_mat_plain_sfft32(MatBuf32 *m);                            /* matrix/src/time_freq.rs:87-91 */
int32_t bdsp_hip_mat_sfft32(MatBuf32 *m);                                  /* :93-97 */
int32_t bdsp_hip_mat_windowed_sfft32(MatBuf32 *m, int32_t window);         /* :99-106 */
int32_t bdsp_hip_mat_plain_sifft32(MatBuf32 *m);                           /* :148-152 */
int32_t bdsp_hip_mat_sifft32(MatBuf32 *m);                                 /* :154-158 */
int32_t bdsp_hip_mat_windowed_sifft32(MatBuf32 *m, int32_t window);        /* :160-167 */
int32_t bdsp_hip_mat_mirror32(MatBuf32 *m);                                /* :173-177 */
int32_t bdsp_hip_mat_to_complex32(MatBuf32 *m);                            /* matrix/src/real.rs:34-54 */
/* Convolution with an impulse-response function and interpolation between the samples of real rows
 * (matrix/src/time_freq.rs:355-387 Convolution::convolve with a real / complex function, :329-353 RealInterpolationOps;
 * convolution.rs:136-254 and real_interpolation.rs:33-176 per row): every row behaves as the vector function OF THE SAME
 * NAME on that row, and the arguments are the vector facade's (impulse_response 0 = sinc, anything else = raised
 * cosine(rolloff); callbacks as bdsp_real_fn / bdsp_complex_fn, is_symmetric is accepted and not used, as there).
 * convolve / convolve_real / convolve_complex: y[i] = sum_{k=0}^{2L} x[(i - L + k) mod N] * f(-(k - L) * ratio) per row,
 * L = len clipped to the row's points N, accumulated over ascending k in the matrix's precision.  The callback forms
 * sample the 2L + 1 weights on the host ONCE for all rows.  A frequency-domain matrix is poisoned (-1) by every form, a
 * real matrix by convolve_complex; zero rows or empty rows: 0, matrix as it is; delta and domain stay.
 * interpolate_lin / interpolate_hermite: real rows of n scalars become rows of round((n - 1) * factor) + 1 scalars,
 * densely packed, bit-equal to interpolate_lin32/64 and interpolate_hermite32/64 on the row; a complex matrix is
 * poisoned (-1); zero rows or empty rows: 0; delta and domain stay.
 * Launches, whatever the row count: the interpolations one; convolve one for the weight table (none for the callback
 * forms) plus one direct kernel when 2L + 1 exceeds N or is at most 33 taps, else the batched block convolution
 * bdsp_hip_mat_convolve_signal uses.  Memory: the interpolations grow both device buffers of the matrix to
 * rows * max(old, new row length) scalars before the launch. */
int32_t bdsp_hip_mat_convolve32(MatBuf32 *m, int32_t impulse_response, float rolloff, float ratio, size_t len); /* matrix/src/time_freq.rs:355-370 */
int32_t bdsp_hip_mat_convolve_ex32(MatBuf32 *m, int32_t impulse_response, float rolloff, float ratio, size_t len,
                                   int32_t path); /* path < 0: as bdsp_hip_mat_convolve; 0: the block convolution whatever the tap count (7 if 2L + 1 exceeds the row's points); else: the direct kernel.  For measuring the crossover. */
int32_t bdsp_hip_mat_convolve_real32(MatBuf32 *m, bdsp_real_fn32 impulse_response, const void *impulse_response_data,
                                     bool is_symmetric, float ratio, size_t len);                   /* :355-370 */
int32_t bdsp_hip_mat_convolve_complex32(MatBuf32 *m, bdsp_complex_fn32 impulse_response, const void *impulse_response_data,
                                        bool is_symmetric, float ratio, size_t len);                /* :372-387 */
int32_t bdsp_hip_mat_interpolate_lin32(MatBuf32 *m, float interpolation_factor, float delay);     /* :343-352 */
int32_t bdsp_hip_mat_interpolate_hermite32(MatBuf32 *m, float interpolation_factor, float delay); /* :333-342 */
/* Math family, reverse, mixer, wrap-around binary operations and the part getters / setters of the rows
 * (matrix/src/general/elementary.rs:226-350 TrigOps / PowerOps, real.rs:58-130 RealOps / ApproximatedOps,
 * general/elementary.rs:190-198 ReorganizeDataOps::reverse, complex.rs:203-211 multiply_complex_exponential,
 * general/elementary.rs:117-188 ElementaryWrapAroundOps, complex.rs:119-201 getters and setters): every row behaves as
 * the vector function OF THE SAME NAME on that row, bit for bit.
 * sqrt .. atanh, root, powf, log, expf: real and complex matrices; root(d) is powf(1 / d), as root32.  abs and the
 * *_approx functions poison a complex matrix (-1).
 * reverse: out[r][i] = in[r][points - 1 - i], bit-exact, real or complex; domain and delta stay.
 * multiply_complex_exponential(a, b): z[r][k] *= exp(j (a delta k + b delta)) with k counted from 0 in EVERY row; a * delta
 * and b * delta are formed in the matrix's precision, the phase in double, the phasor rounded to the matrix's precision
 * (as multiply_complex_exponential32/64); a real matrix is poisoned (-1).
 * add / sub / mul / div_smaller: x[r][i] (.)= y[r][i mod ypoints], row r around row r of `other`: 7 if the row counts
 * differ, then 7 if other's rows are empty or their length does not divide the row length of m, then the meta data check
 * of bdsp_hip_mat_add (2); two matrices without rows: 0.  *_smaller_vector: one period for all rows; the operand's
 * length must divide the ROW length (2 rows of 3 scalars and a 2-scalar operand: 7, although 6 % 2 == 0), 7 also for an
 * empty operand.  The matrix is untouched after an error.
 * get_real / get_imag / get_magnitude / get_magnitude_squared / get_phase, get_real_imag / get_mag_phase: the source is
 * NOT consumed (the vector facade consumes it and answers 9; that is a link-compatibility artefact there).  Every
 * destination becomes rows(m) rows of `points` real scalars and keeps its own domain and delta; a real source or a
 * complex destination leaves the destination(s) with rows(m) rows of length 0.  0; -1 if the source is poisoned, the
 * destinations untouched.  (The reference's matrix get_magnitude, get_magnitude_squared and get_phase all forward to
 * v.get_imag, complex.rs:135-151: a slip there, not reproduced, like diff_with_start above.)
 * set_real_imag / set_mag_phase: 7 unless the two arguments have equal row counts and row lengths; m becomes complex
 * with the shape of the first argument, delta and domain stay; set_mag_phase builds mag * (cos phase, sin phase).
 * Everywhere: zero rows or empty rows: 0, no launch; a poisoned matrix: -1; an argument error (7) comes before the
 * poison check.  Launches: ONE per call, whatever the row count, no synchronisation.  Memory: reverse writes the
 * matrix's second buffer and trades; the getters grow the destinations' buffers to rows * points scalars, the setters
 * the matrix's to rows * 2 * points; everything else works in place. */
int32_t bdsp_hip_mat_sqrt32(MatBuf32 *m);  /* matrix/src/general/elementary.rs:302-350 PowerOps */
int32_t bdsp_hip_mat_square32(MatBuf32 *m);
int32_t bdsp_hip_mat_ln32(MatBuf32 *m);
int32_t bdsp_hip_mat_exp32(MatBuf32 *m);
int32_t bdsp_hip_mat_sin32(MatBuf32 *m);  /* :226-300 TrigOps */
int32_t bdsp_hip_mat_cos32(MatBuf32 *m);
int32_t bdsp_hip_mat_tan32(MatBuf32 *m);
int32_t bdsp_hip_mat_asin32(MatBuf32 *m);
int32_t bdsp_hip_mat_acos32(MatBuf32 *m);
int32_t bdsp_hip_mat_atan32(MatBuf32 *m);
int32_t bdsp_hip_mat_sinh32(MatBuf32 *m);
int32_t bdsp_hip_mat_cosh32(MatBuf32 *m);
int32_t bdsp_hip_mat_tanh32(MatBuf32 *m);
int32_t bdsp_hip_mat_asinh32(MatBuf32 *m);
int32_t bdsp_hip_mat_acosh32(MatBuf32 *m);
int32_t bdsp_hip_mat_atanh32(MatBuf32 *m);
int32_t bdsp_hip_mat_abs32(MatBuf32 *m);  /* matrix/src/real.rs:58-76 */
int32_t bdsp_hip_mat_ln_approx32(MatBuf32 *m);  /* :78-130 */
int32_t bdsp_hip_mat_exp_approx32(MatBuf32 *m);
int32_t bdsp_hip_mat_sin_approx32(MatBuf32 *m);
int32_t bdsp_hip_mat_cos_approx32(MatBuf32 *m);
int32_t bdsp_hip_mat_root32(MatBuf32 *m, float value);
int32_t bdsp_hip_mat_powf32(MatBuf32 *m, float value);
int32_t bdsp_hip_mat_log32(MatBuf32 *m, float value);
int32_t bdsp_hip_mat_expf32(MatBuf32 *m, float value);
int32_t bdsp_hip_mat_log_approx32(MatBuf32 *m, float value);
int32_t bdsp_hip_mat_expf_approx32(MatBuf32 *m, float value);
int32_t bdsp_hip_mat_powf_approx32(MatBuf32 *m, float value);
int32_t bdsp_hip_mat_reverse32(MatBuf32 *m);  /* matrix/src/general/elementary.rs:190-198 */
int32_t bdsp_hip_mat_multiply_complex_exponential32(MatBuf32 *m, float a, float b);  /* matrix/src/complex.rs:203-211 */
int32_t bdsp_hip_mat_add_smaller32(MatBuf32 *m, const MatBuf32 *other);  /* matrix/src/general/elementary.rs:117-188, row r around row r */
int32_t bdsp_hip_mat_sub_smaller32(MatBuf32 *m, const MatBuf32 *other);
int32_t bdsp_hip_mat_mul_smaller32(MatBuf32 *m, const MatBuf32 *other);
int32_t bdsp_hip_mat_div_smaller32(MatBuf32 *m, const MatBuf32 *other);
int32_t bdsp_hip_mat_add_smaller_vector32(MatBuf32 *m, const VecBuf32 *operand);  /* every row around the same vector */
int32_t bdsp_hip_mat_sub_smaller_vector32(MatBuf32 *m, const VecBuf32 *operand);
int32_t bdsp_hip_mat_mul_smaller_vector32(MatBuf32 *m, const VecBuf32 *operand);
int32_t bdsp_hip_mat_div_smaller_vector32(MatBuf32 *m, const VecBuf32 *operand);
int32_t bdsp_hip_mat_get_real32(const MatBuf32 *m, MatBuf32 *destination);  /* matrix/src/complex.rs:119-151 */
int32_t bdsp_hip_mat_get_imag32(const MatBuf32 *m, MatBuf32 *destination);
int32_t bdsp_hip_mat_get_magnitude32(const MatBuf32 *m, MatBuf32 *destination);
int32_t bdsp_hip_mat_get_magnitude_squared32(const MatBuf32 *m, MatBuf32 *destination);
int32_t bdsp_hip_mat_get_phase32(const MatBuf32 *m, MatBuf32 *destination);
int32_t bdsp_hip_mat_get_real_imag32(const MatBuf32 *m, MatBuf32 *real, MatBuf32 *imag);  /* :153-175 */
int32_t bdsp_hip_mat_get_mag_phase32(const MatBuf32 *m, MatBuf32 *mag, MatBuf32 *phase);
int32_t bdsp_hip_mat_set_real_imag32(MatBuf32 *m, const MatBuf32 *real, const MatBuf32 *imag);  /* :177-201 */
int32_t bdsp_hip_mat_set_mag_phase32(MatBuf32 *m, const MatBuf32 *mag, const MatBuf32 *phase);
/* Vector <-> matrix without a host round trip (the reference builds matrices from vectors with to_mat,
 * matrix/src/to_from_mat_conversions.rs; from_frames and overlap_add are the analysis and synthesis steps of an STFT on
 * a signal that stays in HBM).  P, F, H in POINTS (a complex point is two scalars).  Each call allocates its result,
 * hands it back through *out (to be deleted by the caller with bdsp_hip_mat_delete / delete_vector) and launches ONCE,
 * whatever the row count; because they allocate, none of them can be captured into a graph.  All three are bit-exact.
 * from_frames(vector, F, H, pad_tail): row r, point j = x[r * H + j]; positions at or past P read as zero.  Rows:
 * pad_tail == 0: P >= F ? (P - F) / H + 1 : 0 (whole frames only); otherwise P == 0 ? 0 : (P > F ? ceil((P - F) / H) + 1
 * : 1) (every point lies in a frame, the last one zero-extended).  Number space, domain and delta are the vector's, which
 * stays as it is.  F == 0 or H == 0: 7, *out = NULL.
 * overlap_add(m, H): a vector of rows ? (rows - 1) * H + F : 0 points, y[i] = sum of m[r][i - r * H] over the rows with
 * 0 <= i - r * H < F, added in ascending r from +0 by the one lane that owns y[i] -- no atomics, so deterministic and
 * bit-equal to the row loop y[r * H .. r * H + F) += m[r] in the matrix's precision.  H > F leaves zero gaps, H == F
 * flattens the matrix.  Number space, domain and delta are the matrix's, which stays as it is.  H == 0: 7, *out = NULL;
 * a matrix without rows: an empty vector, 0.
 * from_vectors(vectors, count): row r = a copy of vectors[r]; number space, domain and delta of vectors[0].  count == 0:
 * a real time-domain matrix without rows, 0.  Any poisoned vector: a poisoned matrix, -1; else unequal lengths: 7;
 * else unequal number space or domain: 2 (*out = NULL after 7 and 2).  One upload of the pointer table (the call's only
 * synchronisation) and one launch, whatever `count`.  The other direction is bdsp_hip_mat_get_row, or
 * overlap_add(H = row points) for the flat vector.
 * Everywhere: a poisoned source gives a poisoned result (no rows or points, NaN delta) and -1; a failed allocation or a
 * result too long for the address space returns the backend code (<= -100) with *out = NULL. */
int32_t bdsp_hip_mat_from_frames32(const VecBuf32 *vector, size_t frame_points, size_t hop, int32_t pad_tail, MatBuf32 **out);
int32_t bdsp_hip_mat_overlap_add32(const MatBuf32 *m, size_t hop, VecBuf32 **out);
int32_t bdsp_hip_mat_from_vectors32(const VecBuf32 *const *vectors, size_t count, MatBuf32 **out);
/* Across the rows: one tiled transpose of whole elements (a real scalar or a complex pair stays together) serves
 * transpose, from_interleaved and to_interleaved -- the reference's split_into and merge
 * (vector/src/vector_types/general/data_reorganization.rs:477-555) with the rows of ONE matrix as targets and sources,
 * so no pointer table and no synchronisation; zero_interleave is the same file's zero_interleave on every row.  One launch each, bit-exact.
 * transpose(m): in place through the trade buffer, rows <- the old row points, row points <- the old rows; nothing is
 * allocated, so it can be captured into a graph like swap_halves.  Number space, domain and delta stay: delta belongs to
 * the row axis, the axis across the rows has none, and what delta means after a transpose is the caller's business.  A
 * matrix without rows or with empty rows becomes a matrix WITHOUT ROWS, 0 -- so transposing an empty matrix twice does
 * not bring its row count back.  A poisoned matrix: -1, untouched, still poisoned.
 * from_interleaved(vector, channels): a new matrix of `channels` rows x P / channels points, row c, point j =
 * x[j * channels + c] (in points), every row bit-equal to target c of split_into with `channels` targets.  Number space,
 * domain and delta are the vector's, which stays as it is.  channels == 0 or P % channels != 0: 7, *out = NULL.  An
 * empty vector: `channels` empty rows, 0.
 * to_interleaved(m): the inverse -- a new vector of rows * row points points, y[j * rows + r] = m[r][j], bit-equal to
 * merge of the rows; the matrix stays as it is.  A matrix without rows: an empty vector, 0.
 * Both allocate their result, hand it back through *out (to be deleted by the caller with bdsp_hip_mat_delete /
 * delete_vector) and cannot be captured into a graph; a poisoned source gives a poisoned result and -1; a failed
 * allocation or a result too long for the address space returns the backend code (<= -100) with *out = NULL.
 * zero_interleave(m, factor): every point of every row is followed by factor - 1 zeros, as zero_interleave on every row;
 * row points grow by `factor`.  factor <= 1: nothing happens, 0.  -1 for a poisoned matrix.  It grows the buffers, so a
 * captured graph must not contain the first call at a size. */
int32_t bdsp_hip_mat_transpose32(MatBuf32 *m);
int32_t bdsp_hip_mat_from_interleaved32(const VecBuf32 *vector, size_t channels, MatBuf32 **out);
int32_t bdsp_hip_mat_to_interleaved32(const MatBuf32 *m, VecBuf32 **out);
int32_t bdsp_hip_mat_zero_interleave32(MatBuf32 *m, int32_t factor);
/* zoom_fft: chirp-z transform of a frequency band (nothing of it is in the reference).  For every row x[0..N) of a
 * time-domain vector or matrix (complex, or real read with a zero imaginary part)
 *     X[k] = sum_{n<N} x[n] exp(-2 pi i (start + k step) n),   k = 0 .. bins-1
 * start and step in cycles per sample, double in both precisions; unscaled, as plain_fft; step may be 0 or negative and
 * bins may exceed N.  The result is complex, in the frequency domain, `bins` points per row, dense; delta becomes
 * step / delta.  start = 0, step = 1/N, bins = N is plain_fft.  _starts takes one start per row (count == rows).
 * Codes: 7 for bins == 0, a start or step that is not finite, count != rows or a null starts with count > 0 (the data
 * are untouched); 5 for frequency-domain input; -1 for a poisoned vector or matrix; BDSP_ERR_UNSUPPORTED where
 * rows * bins does not fit the address space or the convolution length -- the power of two >= N + bins - 1 -- is above
 * 2^30.  No rows, or rows of no points: as plain_fft leaves them.  Convolution lengths up to 4096 are one launch.  The
 * chirp tables are cached per (N, bins, start, step) with the chirp-z plans of the any-length transforms: inside a HIP
 * graph capture a missing plan is BDSP_ERR_UNSUPPORTED (run the call once before), and _starts uploads its argument, so
 * it cannot be captured at all. */
int32_t bdsp_hip_zoom_fft32(VecBuf32 *v, double start, double step, size_t bins);
int32_t bdsp_hip_mat_zoom_fft32(MatBuf32 *m, double start, double step, size_t bins);
int32_t bdsp_hip_mat_zoom_fft_starts32(MatBuf32 *m, const double *starts, size_t count, double step, size_t bins);
/* matmul: the product of two matrices on the device (nothing of it is in the reference).  Sizes in POINTS.
 *     b_conj_transposed == 0:  a: M x K, b: K x N  ->  out: M x N,  out[i][n] = sum_k a[i][k] * b[k][n]
 *     b_conj_transposed != 0:  a: M x K, b: N x K  ->  out: M x N,  out[i][j] = sum_k a[i][k] * conj(b[j][k])
 * a and b may be the same object (the Gram / covariance matrix of its rows); both stay untouched.  Both operands are
 * real or both are complex (convert real weights with to_complex first); the result has their number space, and for real
 * operands conj is the identity.  Domains and deltas need not agree: the result takes domain and delta from the operand
 * whose row axis survives, b in the plain form and a in the transposed one.  A complex product is four real products.
 * Codes: -1 for a poisoned a or b, with a poisoned result in *out; else 2 for a real and a complex operand; else 7
 * unless a's row points equal b's rows (plain) or b's row points (transposed); after 2 and 7 *out = NULL.  Empty shapes
 * return 0: K == 0 gives an M x N matrix of +0, M == 0 a matrix without rows, N == 0 M empty rows.  A failed allocation
 * (BDSP_ERR_HIP) or a result or temporary too long for the address space (BDSP_ERR_UNSUPPORTED) returns that backend code
 * with *out = NULL.  The call allocates its result (to be deleted by the caller with bdsp_hip_mat_delete), so it cannot
 * be captured into a graph.  Rows of either operand may start on any element boundary.
 * Deterministic: every output element is one sum over ascending k from +0 with one rounding per product; for K >= 256
 * and at most 64 tiles of 64 x 64 outputs, K is cut into chunks whose sums are added in ascending chunk order.  The
 * path and the order are a function of (M, N, K, number kind, precision, form) only, never of the device's CU count or
 * of timing: the same call gives the same bits on every run.  With a == b in the transposed form the result is Hermitian
 * to the bit and its diagonal has imaginary part +0.  Every element is within (2 K + 4) eps sum_k |a[i][k]| |b[k][n]| of
 * the exact product.  One launch, or two where K is cut, whatever the shape. */
int32_t bdsp_hip_mat_matmul32(const MatBuf32 *a, const MatBuf32 *b, int32_t b_conj_transposed, MatBuf32 **out);
/* cholesky / cholesky_solve: Hermitian positive-definite systems on the device (nothing of them is in the reference).
 * bdsp_hip_mat_cholesky: a is N x N, real (symmetric) or complex (Hermitian).  Only the lower triangle is read, and of
 * the diagonal only the real part; the upper triangle and the diagonal's imaginary parts may hold anything, NaN included.
 * loading is rounded once to the matrix's precision and added to every diagonal element as it is read, with one rounding
 * (diagonal loading, a + loading I); a stays untouched.  *out is a new N x N matrix L with a = L L^H: lower triangular,
 * the diagonal real and > 0 with imaginary part +0, every element above the diagonal +0, domain and delta from a.
 * Codes: 0; -1 for a poisoned a, with a poisoned result in *out; else 7 unless a's rows equal its row points, *out =
 * NULL; 8 when a pivot is <= 0 or not finite (a is not Hermitian positive definite), *out = NULL: one 4-byte read-back
 * after the last launch, the call's only synchronisation.  N == 0 gives 0 and an empty matrix.  A failed allocation
 * (BDSP_ERR_HIP) or a size too long for the address space (BDSP_ERR_UNSUPPORTED) returns that backend code with *out = NULL.
 * bdsp_hip_mat_cholesky_solve: l is N x N, a factor as bdsp_hip_mat_cholesky returns it (only its lower triangle is read,
 * of its diagonal the real part); b is N x P; *out is a new N x P matrix with domain and delta from b; both operands stay
 * untouched.  part: 0 both (forward, then backward: a^-1 b), 1 forward (L x = b: L^-1 b, whitening), 2 backward
 * (L^H x = b); any other value BDSP_ERR_UNSUPPORTED.  Codes: -1 for a poisoned l or b, with a poisoned result; else 2 for
 * a real and a complex operand; else 7 unless l is square and l's rows equal b's rows; after 2 and 7 *out = NULL.  P == 0
 * gives N empty rows, N == 0 a matrix without rows.  A zero on l's diagonal gives inf / NaN in the result and code 0;
 * nothing is tested, nothing is read back: this call does not synchronise.
 * Both calls allocate their results (to be deleted with bdsp_hip_mat_delete), so they cannot be captured into a graph.
 * N <= 64: one launch (per triangular pass); larger N: blocks of 64, at most 3 ceil(N / 64) launches for the
 * factorisation and 2 ceil(N / 64) per triangular pass, whatever P.  No atomics.  Deterministic: the path and the order
 * of operations are a function of (N, P, number kind, precision, part) only, never of the device's CU count or of
 * timing: the same call gives the same bits on every run.  Element-wise, with A the loaded matrix and c(N) = 2 N + 4:
 * |A - L L^H| <= c(N) eps |L| |L|^H;  |b - L x| <= c(N) eps |L| |x| (forward; backward with L^H);
 * |b - L L^H x| <= 3 c(N) eps |L| |L|^H |x| (both). */
int32_t bdsp_hip_mat_cholesky32(const MatBuf32 *a, double loading, MatBuf32 **out);
int32_t bdsp_hip_mat_cholesky_solve32(const MatBuf32 *l, const MatBuf32 *b, int32_t part, MatBuf32 **out);
/* eigh: the eigendecomposition of a Hermitian matrix on the device (nothing of it is in the reference).  a is N x N,
 * real (symmetric) or complex (Hermitian).  Only the lower triangle is read, and of the diagonal only the real part; the
 * upper triangle and the diagonal's imaginary parts may hold anything, NaN included; a stays untouched.  *w is a new real
 * matrix of 1 row x N points, the eigenvalues in ascending order, ties in the order of the index a value had before
 * sorting; *v a new N x N matrix of a's number kind; both take domain and delta from a.  Row k of v is the k-th
 * eigenvector conjugate-transposed: v a v^H = diag(w) and v v^H = I, so matmul(v, x) is the transform to the principal
 * components of the rows of x and a subspace is a set of rows.  The phase of a row is arbitrary but reproducible.
 * *sweeps (sweeps may be NULL) is the number of sweeps taken, the last one, which rotated nothing, included: 1 for the
 * identity, a diagonal matrix and the zero matrix, whose v is a permutation matrix to the bit.
 * Codes: 0; -1 for a poisoned a, with poisoned results in *w and *v; else 7 unless a's rows equal its row points, *w =
 * *v = NULL; 8 when the Frobenius norm of the matrix as read is not finite (a NaN or an infinity in what is read, or
 * squares that overflow) or when the iteration has not converged after 30 sweeps, *w = *v = NULL.  N == 0 gives 0 and two
 * empty matrices.  A failed allocation (BDSP_ERR_HIP) or a size too long for the address space (BDSP_ERR_UNSUPPORTED)
 * returns that backend code with *w = *v = NULL.  The call allocates its results (to be deleted with
 * bdsp_hip_mat_delete), so it cannot be captured into a graph.
 * Method: cyclic two-sided Jacobi in the round-robin ordering; a pair (p, q) is rotated iff |a_pq| > eps |a|_F / N, by
 * the small angle; every product-sum is one fma, a complex product four real ones, divisions and square roots correctly
 * rounded.  N <= 64: one launch of one workgroup with the matrix in LDS, then one 4-byte read-back, the call's only
 * synchronisation.  Larger N: blocks of 32 columns in the same ordering; 3 launches per block step (the pivot problem
 * of a block pair, its rows, its columns), so 3 B launches per sweep with B = ceil(N / 32) (3 (B - 1) for even B), plus 3
 * for the whole call; the call synchronises once per sweep on one small read-back of the rotation counts.  No atomics.
 * Deterministic: the path, the ordering and the order of operations are a function of (N, number kind, precision) only,
 * never of the device's CU count or of timing: the same call gives the same bits on every run.  In Frobenius norms, with
 * S = *sweeps: |a - v^H diag(w) v| <= c_res(N, S) eps |a| and |v v^H - I| <= c_orth(N, S) eps, c_orth = 2 K S sqrt(N),
 * c_res = 2 K S (1 + sqrt(N)) + 1, K = rho N for N <= 64 and 8 (128 rho + 132) times the block steps of a sweep above,
 * rho = 24 (real), 40 (complex). */
int32_t bdsp_hip_mat_eigh32(const MatBuf32 *a, MatBuf32 **w, MatBuf32 **v, int32_t *sweeps);
/* sosfilt: recursive (IIR) filtering with a cascade of second-order sections along a vector or along every row of a
 * matrix, in place (nothing of it is in the reference).  sos holds `sections` rows of six doubles b0 b1 b2 a0 a1 a2, the
 * layout of scipy's output='sos'; every section is divided by its a0 in double and rounded once to the data's precision.
 * A section is direct form II transposed, y = b0 x + s1, s1 <- b1 x - a1 y + s2, s2 <- b2 x - a2 y, the form and state
 * convention of scipy.signal.sosfilt; the sections are applied in order.  The data are real or complex in the time domain;
 * complex data are filtered as two independent real signals (the coefficients are real).  Length, domain, delta and
 * number kind stay.  state (may be NULL: zero initial state, the final state is dropped) is a vector of 2 * sections
 * points, for a matrix a matrix of rows x 2 * sections points, of the data's number kind: s1, s2 of section 0, then of
 * section 1, ...; it is read as the initial state and overwritten with the state after the last point, so a recording can
 * be filtered block after block.
 * Codes: 0; 7, with the data untouched, for sections > 0 with a NULL sos, a coefficient that is not finite, a0 == 0,
 * sections above 16 (IIR_MAX_SECTIONS) or a state of the wrong shape; -1 for a poisoned vector, matrix or state; 5 for
 * frequency-domain data; 2 for a state of the other number kind.  sections == 0, no rows, or rows of no points: 0 and
 * nothing changes.  An unstable filter gives inf or NaN as the recurrence would, with code 0: nothing is tested.  A failed
 * allocation (BDSP_ERR_HIP) or rows x tiles above 2^31 (BDSP_ERR_UNSUPPORTED) returns that backend code.  The call
 * uploads its coefficient tables, so it cannot be captured into a graph.
 * Method: a row is cut into tiles of 4096 points, a tile into 256 chunks of 16; every lane runs its chunk from a zero
 * state, the chunk end states are combined by a fixed tree of the maps s -> A^16 s + e with host tables A^(16 * 2^k), and
 * every lane runs its chunk again from its true state.  Rows of one tile: one launch.  Longer rows: three launches (end
 * states of the tiles from zero, the carry along the row in double, the tiles from their true states), whatever the row
 * count.  No atomics, no workgroup waits for another.  Deterministic: the result is a function of (row length, sos,
 * number kind, precision, incoming state) only, never of the row count, the device's CU count or of timing: row r of the
 * matrix call is bit-equal to the vector call on that row. */
int32_t bdsp_hip_sosfilt32(VecBuf32 *v, const double *sos, size_t sections, VecBuf32 *state /* may be NULL */);
int32_t bdsp_hip_mat_sosfilt32(MatBuf32 *m, const double *sos, size_t sections, MatBuf32 *state /* may be NULL */);
/* rank_filter: a sliding order statistic along a vector or along every row of a matrix, in place (nothing of it is in
 * the reference).  The data are real, in any domain; length, domain, delta and number kind stay.  For point i of a row of
 * n points the window is the multiset x[i + d], guard < |d| <= half; with guard == -1 (none) it is all |d| <= half, the
 * centre included: W = 2 half + 1 values without a guard, 2 (half - guard) with one.  The result is the window's element
 * of rank `rank`, 0 the smallest and W - 1 the largest; every result is computed from the row as it was on entry.  The
 * median filter of an odd kernel size k is half = rank = (k - 1) / 2; rank 0 and W - 1 are the running minimum and
 * maximum; a guard gives the ordered-statistic CFAR floor of the training cells around every cell.
 * boundary says how positions outside the row are read: 0 (zero) as +0.0, scipy.signal.medfilt's rule; 1 (wrap) index
 * mod n, also where half >= n and the window wraps more than once; 2 (nearest) the row's first or last point.
 * Order: IEEE totalOrder on the bit patterns, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN: the kernel compares the
 * keys bits ^ (sign ? all ones : sign bit) as unsigned integers.  The output carries exactly the bits of the selected
 * input, NaN payloads and denormals included: no flush and no arithmetic touches a value.
 * Codes: 0; 7, with the data untouched, for rank >= W, guard >= half (or below -1) or an unknown boundary; then -1 for a
 * poisoned vector or matrix; then 4 (BDSP_ERR_MUST_BE_REAL) for complex data; then BDSP_ERR_UNSUPPORTED for half above
 * 1024 (RANK_MAX_HALF) and for rows x tiles above 2^31.  No rows, or rows of no points: 0 and nothing changes.
 * Method: one launch whatever the row count, rows x tiles of 1024 outputs; a workgroup holds its tile and a halo of half
 * on each side in LDS as integer keys and writes to the trade buffer, which is then swapped in.  Short windows count,
 * for every candidate, the window keys below it and at or below it (W^2 reads); long windows build the answer key bit
 * by bit from the top (32 or 64 passes over the window); the choice depends on W and the precision alone.  No atomics,
 * no early exit, no workgroup waits for another.  Deterministic: the result is a function of the row and the arguments
 * only, never of the row count, the device's CU count or of timing: row r of the matrix call is bit-equal to the vector
 * call on that row. */
int32_t bdsp_hip_rank_filter32(VecBuf32 *v, size_t half, size_t rank, int64_t guard /* -1: none */, int32_t boundary);
int32_t bdsp_hip_mat_rank_filter32(MatBuf32 *m, size_t half, size_t rank, int64_t guard /* -1: none */, int32_t boundary);
/* detect: the detections of a vector, or of every row of a matrix, as a compact list (nothing of it is in the reference).
 * The data are real, in any domain, and are not modified.  Cell j of a row of n points is a detection iff it is above the
 * threshold and a strict local maximum of order `order`.
 * Threshold, by kind: 0 none (threshold NULL); 1 one value, double(x[j]) > t (const double * to one value); 2 one value
 * per row, double(x[r][j]) > t[r] (const double * to rows values; on a vector it means one value); 3 one profile for all
 * rows, x[r][j] > t[j] (const VecBuf * of n points of the same precision); 4 one value per cell, x[r][j] > t[r][j] (const
 * MatBuf * of rows x n).  Every comparison is IEEE >: a NaN on either side is never a detection, -0 is not above +0,
 * denormals compare by value, +inf > t holds for finite t.
 * Strict local maximum: for every d with 0 < |d| <= order, x[j] > x[j + d]; order 0 is no condition.  boundary says how
 * positions outside the row are read: 0 (open) the comparison is skipped, so an end point can be a peak and with n = 1
 * every cell passes; 1 (wrap) index mod n, any number of turns, so order >= n compares a cell with itself and detects
 * nothing; 2 (nearest) the end point repeated, scipy.signal.argrelmax's mode "clip": an end point is never a peak for
 * order >= 1.  Plateaus yield no peak; a NaN neighbour blocks a peak.
 * Outputs: counts[r] is always the true number of detections of row r (one entry for a vector); index and value receive
 * the first min(total, capacity) detections in row-major order, rows ascending and index ascending within a row; value
 * holds exactly the bits of the detected input.  The row of an entry follows from counts.  With capacity 0 the two lists
 * may be NULL and the write launch is skipped.
 * Codes: 0; 7, with nothing written, for an unknown kind or boundary, a NULL counts, a NULL threshold of a kind that has
 * one, NULL lists with capacity > 0, or kind 4 on a vector; then -1 for a poisoned x or operand; then 4
 * (BDSP_ERR_MUST_BE_REAL) for a complex x or operand; then, for kinds 3 and 4, the size and meta-data checks of add with
 * its codes (7 for another row count, 1, 2); then BDSP_ERR_UNSUPPORTED for order above 1024 (DETECT_MAX_ORDER) and for
 * rows x tiles above 2^31.  No rows, or rows of no points: 0 with counts zeroed.
 * Method: four launches whatever the row count: the count of every tile of 1024 cells (a workgroup holds its tile and a
 * halo of order on each side in LDS; a wave's 64-bit ballot counts 64 consecutive cells), the prefix over the tiles of
 * each row, the prefix over the rows (both 64-bit), and the tile launch again, which stores every detection at its slot.
 * x is read twice; only counts and the listed entries are copied to the host.  No atomics, no workgroup waits for
 * another.  Deterministic: the list is a function of the data and the arguments only, never of the row count, the
 * device's CU count or of timing: row r of the matrix call equals the vector call on that row. */
int32_t bdsp_hip_detect32(const VecBuf32 *v, int32_t kind, const void *threshold, size_t order, int32_t boundary,
                          size_t capacity, int64_t *counts /* 1 */, int64_t *index /* capacity */, float *value /* capacity */);
int32_t bdsp_hip_mat_detect32(const MatBuf32 *m, int32_t kind, const void *threshold, size_t order, int32_t boundary,
                              size_t capacity, int64_t *counts /* rows */, int64_t *index, float *value);
/* sort, order_select: the order statistics of a vector, or of every row of a matrix (nothing of it is in the reference).
 * The data are real, in any domain; n is the points of a row.
 * Order: ascending is IEEE totalOrder on the bit patterns, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, realised as the
 * unsigned keys k = bits ^ (sign ? all ones : sign bit); ties are broken by ascending index.  Descending is the stable
 * ascending sort of the complemented key ~k: largest first, and among equal bit patterns the lower index first; it is not
 * the reverse of the ascending permutation.  Every output carries exactly the bits of the selected input, NaN payloads and
 * denormals included: no flush and no arithmetic touches a value.
 * sort sorts every row in place; length, domain, delta and number kind stay.  order_select leaves x as it is and writes, for
 * every row, the elements of the sorted ranks ranks[0 .. count): index (the position in the row) and value (its bits, float
 * or double), rows x count row-major entries each, to host arrays.  argsort is count = n, top_k is count = k, a quantile
 * selects its one or two ranks; a top_k is the full sort and a crop.
 * Codes: 0; 7, with the data untouched and nothing written, for a descending that is not 0 or 1, a rank at or above n, or
 * count above n without ranks; then -1 for a poisoned x; then 4 (BDSP_ERR_MUST_BE_REAL) for complex data; then
 * BDSP_ERR_UNSUPPORTED for n at or above 2^32 and for rows x tiles above 2^31.  No rows, or rows of no points: 0, nothing
 * changes and nothing is written; count 0 likewise.
 * Method: a tile launch, in which a workgroup of 256 lanes sorts 4096 elements (SORT_TILE: one tile of a long row, or
 * 4096 / p rows of at most p points, p a power of two <= 2048) with a bitonic network, 16 elements per lane in registers and
 * the longer compare distances through LDS; then P = ceil(log2(ceil(n / 4096))) merge launches, each merging neighbouring
 * runs by the merge path (ties to the left run) and a bitonic merge of 4096 outputs per workgroup.  sort: 1 + P launches
 * between the live and the trade buffer, keys travel as keys and the last launch turns them back into bits.  order_select:
 * 2 + P launches (the last gathers the ranks), (key, 32-bit index) pairs in two workspaces of rows x n x (4 + 4) or (8 + 4)
 * bytes (one where n <= 4096), one synchronisation, and only the rows x count entries are copied to the host.  No atomics,
 * no workgroup waits for another, no loop leaves early: launch count and work depend on (rows, n, precision, with or
 * without index) only.  Deterministic: the result is a function of the input bits alone, never of the row count, the
 * device's CU count or of timing: row r of the matrix call equals the vector call on that row. */
int32_t bdsp_hip_sort32(VecBuf32 *v, int32_t descending);
int32_t bdsp_hip_mat_sort32(MatBuf32 *m, int32_t descending);
/* the elements of sorted ranks ranks[0..count) of every row, as rows x count row-major entries; ranks: a host array, each
 * < n, any order, repeats allowed; NULL: 0 .. count - 1 (count <= n).  index and value may each be NULL.  x is not modified. */
int32_t bdsp_hip_order_select32(const VecBuf32 *v, int32_t descending, size_t count, const uint64_t *ranks, int64_t *index, void *value);
int32_t bdsp_hip_mat_order_select32(const MatBuf32 *m, int32_t descending, size_t count, const uint64_t *ranks, int64_t *index, void *value);

MatBuf64 *bdsp_hip_mat_new64(int32_t is_complex, int32_t domain, size_t rows, size_t row_len, double delta); /* row_len in scalars; zero filled */
void bdsp_hip_mat_delete64(MatBuf64 *m);
size_t bdsp_hip_mat_rows64(const MatBuf64 *m);        /* col_len() of the reference (number of row vectors) */
size_t bdsp_hip_mat_row_len64(const MatBuf64 *m);     /* row_len(): scalars per row */
size_t bdsp_hip_mat_row_points64(const MatBuf64 *m);
int32_t bdsp_hip_mat_is_complex64(const MatBuf64 *m);
int32_t bdsp_hip_mat_get_domain64(const MatBuf64 *m);
double bdsp_hip_mat_get_delta64(const MatBuf64 *m);
void *bdsp_hip_mat_device_ptr64(MatBuf64 *m);         /* [rows][row_len] contiguous */
int32_t bdsp_hip_mat_upload64(MatBuf64 *m, const double *data, size_t len);   /* len == rows*row_len */
int32_t bdsp_hip_mat_download64(MatBuf64 *m, double *out, size_t len);
VecBuf64 *bdsp_hip_mat_get_row64(const MatBuf64 *m, size_t row);           /* copy of one row as a vector handle */
int32_t bdsp_hip_mat_set_row64(MatBuf64 *m, size_t row, const VecBuf64 *vector);
int32_t bdsp_hip_mat_real_scale64(MatBuf64 *m, double factor);
int32_t bdsp_hip_mat_real_offset64(MatBuf64 *m, double offset);
int32_t bdsp_hip_mat_complex_scale64(MatBuf64 *m, double re, double im);
int32_t bdsp_hip_mat_conj64(MatBuf64 *m);
int32_t bdsp_hip_mat_add64(MatBuf64 *m, const MatBuf64 *other);            /* matrix (.) matrix */
int32_t bdsp_hip_mat_sub64(MatBuf64 *m, const MatBuf64 *other);
int32_t bdsp_hip_mat_mul64(MatBuf64 *m, const MatBuf64 *other);
int32_t bdsp_hip_mat_div64(MatBuf64 *m, const MatBuf64 *other);
int32_t bdsp_hip_mat_add_vector64(MatBuf64 *m, const VecBuf64 *operand);   /* every row (.) the same vector */
int32_t bdsp_hip_mat_sub_vector64(MatBuf64 *m, const VecBuf64 *operand);
int32_t bdsp_hip_mat_mul_vector64(MatBuf64 *m, const VecBuf64 *operand);
int32_t bdsp_hip_mat_div_vector64(MatBuf64 *m, const VecBuf64 *operand);
int32_t bdsp_hip_mat_magnitude64(MatBuf64 *m);
int32_t bdsp_hip_mat_magnitude_squared64(MatBuf64 *m);
int32_t bdsp_hip_mat_to_real64(MatBuf64 *m);
int32_t bdsp_hip_mat_to_imag64(MatBuf64 *m);
int32_t bdsp_hip_mat_phase64(MatBuf64 *m);
int32_t bdsp_hip_mat_plain_fft64(MatBuf64 *m);                             /* matrix/src/time_freq.rs:53-61 */
int32_t bdsp_hip_mat_fft64(MatBuf64 *m);                                   /* :63-71 */
int32_t bdsp_hip_mat_windowed_fft64(MatBuf64 *m, int32_t window);          /* :73-81 */
int32_t bdsp_hip_mat_plain_ifft64(MatBuf64 *m);                            /* :120-128 */
int32_t bdsp_hip_mat_ifft64(MatBuf64 *m);                                  /* :130-138 */
int32_t bdsp_hip_mat_windowed_ifft64(MatBuf64 *m, int32_t window);         /* :140-148 */
int32_t bdsp_hip_mat_apply_window64(MatBuf64 *m, int32_t window);
int32_t bdsp_hip_mat_unapply_window64(MatBuf64 *m, int32_t window);
int32_t bdsp_hip_mat_swap_halves64(MatBuf64 *m);
int32_t bdsp_hip_mat_fft_shift64(MatBuf64 *m);
int32_t bdsp_hip_mat_ifft_shift64(MatBuf64 *m);
int32_t bdsp_hip_mat_zero_pad64(MatBuf64 *m, size_t points, int32_t padding_option);
int32_t bdsp_hip_mat_convolve_signal64(MatBuf64 *m, const VecBuf64 *impulse_response);      /* :421-431, one filter for all rows */
int32_t bdsp_hip_mat_convolve_signal_mat64(MatBuf64 *m, const VecBuf64 *const *impulse_responses,
                                           size_t count); /* :439-483: count == rows*rows, row-major [out][in] */
int32_t bdsp_hip_mat_interpolatef64(MatBuf64 *m, int32_t impulse_response, double rolloff,
                                    double interpolation_factor, double delay, size_t conv_len);
int32_t bdsp_hip_mat_interpolatef_delays64(MatBuf64 *m, int32_t impulse_response, double rolloff,
                                           double interpolation_factor, const double *delays, size_t count,
                                           size_t conv_len);
int32_t bdsp_hip_mat_multiply_frequency_response64(MatBuf64 *m, int32_t frequency_response, double rolloff, double ratio);
/* per-row statistics, sums and dot products: as the f32 set above */
int32_t bdsp_hip_mat_real_statistics64(const MatBuf64 *m, Statistics64 *out, size_t len);                 /* matrix/src/general/statistics.rs:4-19 */
int32_t bdsp_hip_mat_complex_statistics64(const MatBuf64 *m, ComplexStatistics64 *out, size_t len);
int32_t bdsp_hip_mat_real_statistics_prec64(const MatBuf64 *m, Statistics64 *out, size_t len);             /* :240-255 */
int32_t bdsp_hip_mat_complex_statistics_prec64(const MatBuf64 *m, ComplexStatistics64 *out, size_t len);
int32_t bdsp_hip_mat_real_statistics_split64(const MatBuf64 *m, Statistics64 *out, size_t out_len, size_t len);       /* :21-36 */
int32_t bdsp_hip_mat_complex_statistics_split64(const MatBuf64 *m, ComplexStatistics64 *out, size_t out_len, size_t len);
int32_t bdsp_hip_mat_real_statistics_split_prec64(const MatBuf64 *m, Statistics64 *out, size_t out_len, size_t len);   /* :257-272 */
int32_t bdsp_hip_mat_complex_statistics_split_prec64(const MatBuf64 *m, ComplexStatistics64 *out, size_t out_len, size_t len);
int32_t bdsp_hip_mat_real_sum64(const MatBuf64 *m, double *out, size_t len);                                     /* :140-163 */
int32_t bdsp_hip_mat_real_sum_sq64(const MatBuf64 *m, double *out, size_t len);
int32_t bdsp_hip_mat_complex_sum64(const MatBuf64 *m, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_complex_sum_sq64(const MatBuf64 *m, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_real_sum_prec64(const MatBuf64 *m, double *out, size_t len);                           /* :376-400 */
int32_t bdsp_hip_mat_real_sum_sq_prec64(const MatBuf64 *m, double *out, size_t len);
int32_t bdsp_hip_mat_complex_sum_prec64(const MatBuf64 *m, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_complex_sum_sq_prec64(const MatBuf64 *m, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_real_dot_product64(const MatBuf64 *m, const MatBuf64 *factor, double *out, size_t len);   /* matrix/src/general/mod.rs:9-25 */
int32_t bdsp_hip_mat_complex_dot_product64(const MatBuf64 *m, const MatBuf64 *factor, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_real_dot_product_prec64(const MatBuf64 *m, const MatBuf64 *factor, double *out, size_t len);    /* :153-169 */
int32_t bdsp_hip_mat_complex_dot_product_prec64(const MatBuf64 *m, const MatBuf64 *factor, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_real_dot_product_vector64(const MatBuf64 *m, const VecBuf64 *factor, double *out, size_t len);     /* :81-97 */
int32_t bdsp_hip_mat_complex_dot_product_vector64(const MatBuf64 *m, const VecBuf64 *factor, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_real_dot_product_vector_prec64(const MatBuf64 *m, const VecBuf64 *factor, double *out, size_t len);   /* :225-241 */
int32_t bdsp_hip_mat_complex_dot_product_vector_prec64(const MatBuf64 *m, const VecBuf64 *factor, bdsp_complex64 *out, size_t len);
int32_t bdsp_hip_mat_prepare_argument64(MatBuf64 *m);                      /* matrix/src/time_freq.rs:208-229 */
int32_t bdsp_hip_mat_prepare_argument_padded64(MatBuf64 *m);
int32_t bdsp_hip_mat_correlate64(MatBuf64 *m, const MatBuf64 *other);        /* :241-264, row r with row r of other */
int32_t bdsp_hip_mat_correlate_vector64(MatBuf64 *m, const VecBuf64 *other); /* every row with one prepared vector */
/* differences, running sums, wrap / unwrap of the rows: as the f32 set above */
int32_t bdsp_hip_mat_diff64(MatBuf64 *m);
int32_t bdsp_hip_mat_diff_with_start64(MatBuf64 *m);
int32_t bdsp_hip_mat_cum_sum64(MatBuf64 *m);
int32_t bdsp_hip_mat_wrap64(MatBuf64 *m, double divisor);
int32_t bdsp_hip_mat_unwrap64(MatBuf64 *m, double divisor);
/* FFT-domain resampling and decimation of the rows: as the f32 set above */
int32_t bdsp_hip_mat_interpolatei64(MatBuf64 *m, int32_t frequency_response, double rolloff,
                                    int32_t interpolation_factor);
int32_t bdsp_hip_mat_interpolate64(MatBuf64 *m, int32_t frequency_response, double rolloff,
                                   size_t dest_points, double delay);
int32_t bdsp_hip_mat_interpft64(MatBuf64 *m, size_t dest_points);
int32_t bdsp_hip_mat_decimatei64(MatBuf64 *m, uint32_t decimation_factor, uint32_t delay);
/* symmetric real-signal transforms of the rows, mirror, to_complex: as the f32 set above */
int32_t bdsp_hip_mat_plain_sfft64(MatBuf64 *m);
int32_t bdsp_hip_mat_sfft64(MatBuf64 *m);
int32_t bdsp_hip_mat_windowed_sfft64(MatBuf64 *m, int32_t window);
int32_t bdsp_hip_mat_plain_sifft64(MatBuf64 *m);
int32_t bdsp_hip_mat_sifft64(MatBuf64 *m);
int32_t bdsp_hip_mat_windowed_sifft64(MatBuf64 *m, int32_t window);
int32_t bdsp_hip_mat_mirror64(MatBuf64 *m);
int32_t bdsp_hip_mat_to_complex64(MatBuf64 *m);
int32_t bdsp_hip_mat_convolve64(MatBuf64 *m, int32_t impulse_response, double rolloff, double ratio, size_t len); /* matrix/src/time_freq.rs:355-370 */
int32_t bdsp_hip_mat_convolve_ex64(MatBuf64 *m, int32_t impulse_response, double rolloff, double ratio, size_t len,
                                   int32_t path); /* path < 0: as bdsp_hip_mat_convolve; 0: the block convolution whatever the tap count (7 if 2L + 1 exceeds the row's points); else: the direct kernel.  For measuring the crossover. */
int32_t bdsp_hip_mat_convolve_real64(MatBuf64 *m, bdsp_real_fn64 impulse_response, const void *impulse_response_data,
                                     bool is_symmetric, double ratio, size_t len);                   /* :355-370 */
int32_t bdsp_hip_mat_convolve_complex64(MatBuf64 *m, bdsp_complex_fn64 impulse_response, const void *impulse_response_data,
                                        bool is_symmetric, double ratio, size_t len);                /* :372-387 */
int32_t bdsp_hip_mat_interpolate_lin64(MatBuf64 *m, double interpolation_factor, double delay);     /* :343-352 */
int32_t bdsp_hip_mat_interpolate_hermite64(MatBuf64 *m, double interpolation_factor, double delay); /* :333-342 */
/* math family, reverse, mixer, *_smaller and part operations of the rows: as the f32 set above */
int32_t bdsp_hip_mat_sqrt64(MatBuf64 *m);
int32_t bdsp_hip_mat_square64(MatBuf64 *m);
int32_t bdsp_hip_mat_ln64(MatBuf64 *m);
int32_t bdsp_hip_mat_exp64(MatBuf64 *m);
int32_t bdsp_hip_mat_sin64(MatBuf64 *m);
int32_t bdsp_hip_mat_cos64(MatBuf64 *m);
int32_t bdsp_hip_mat_tan64(MatBuf64 *m);
int32_t bdsp_hip_mat_asin64(MatBuf64 *m);
int32_t bdsp_hip_mat_acos64(MatBuf64 *m);
int32_t bdsp_hip_mat_atan64(MatBuf64 *m);
int32_t bdsp_hip_mat_sinh64(MatBuf64 *m);
int32_t bdsp_hip_mat_cosh64(MatBuf64 *m);
int32_t bdsp_hip_mat_tanh64(MatBuf64 *m);
int32_t bdsp_hip_mat_asinh64(MatBuf64 *m);
int32_t bdsp_hip_mat_acosh64(MatBuf64 *m);
int32_t bdsp_hip_mat_atanh64(MatBuf64 *m);
int32_t bdsp_hip_mat_abs64(MatBuf64 *m);
int32_t bdsp_hip_mat_ln_approx64(MatBuf64 *m);
int32_t bdsp_hip_mat_exp_approx64(MatBuf64 *m);
int32_t bdsp_hip_mat_sin_approx64(MatBuf64 *m);
int32_t bdsp_hip_mat_cos_approx64(MatBuf64 *m);
int32_t bdsp_hip_mat_root64(MatBuf64 *m, double value);
int32_t bdsp_hip_mat_powf64(MatBuf64 *m, double value);
int32_t bdsp_hip_mat_log64(MatBuf64 *m, double value);
int32_t bdsp_hip_mat_expf64(MatBuf64 *m, double value);
int32_t bdsp_hip_mat_log_approx64(MatBuf64 *m, double value);
int32_t bdsp_hip_mat_expf_approx64(MatBuf64 *m, double value);
int32_t bdsp_hip_mat_powf_approx64(MatBuf64 *m, double value);
int32_t bdsp_hip_mat_reverse64(MatBuf64 *m);
int32_t bdsp_hip_mat_multiply_complex_exponential64(MatBuf64 *m, double a, double b);
int32_t bdsp_hip_mat_add_smaller64(MatBuf64 *m, const MatBuf64 *other);
int32_t bdsp_hip_mat_sub_smaller64(MatBuf64 *m, const MatBuf64 *other);
int32_t bdsp_hip_mat_mul_smaller64(MatBuf64 *m, const MatBuf64 *other);
int32_t bdsp_hip_mat_div_smaller64(MatBuf64 *m, const MatBuf64 *other);
int32_t bdsp_hip_mat_add_smaller_vector64(MatBuf64 *m, const VecBuf64 *operand);
int32_t bdsp_hip_mat_sub_smaller_vector64(MatBuf64 *m, const VecBuf64 *operand);
int32_t bdsp_hip_mat_mul_smaller_vector64(MatBuf64 *m, const VecBuf64 *operand);
int32_t bdsp_hip_mat_div_smaller_vector64(MatBuf64 *m, const VecBuf64 *operand);
int32_t bdsp_hip_mat_get_real64(const MatBuf64 *m, MatBuf64 *destination);
int32_t bdsp_hip_mat_get_imag64(const MatBuf64 *m, MatBuf64 *destination);
int32_t bdsp_hip_mat_get_magnitude64(const MatBuf64 *m, MatBuf64 *destination);
int32_t bdsp_hip_mat_get_magnitude_squared64(const MatBuf64 *m, MatBuf64 *destination);
int32_t bdsp_hip_mat_get_phase64(const MatBuf64 *m, MatBuf64 *destination);
int32_t bdsp_hip_mat_get_real_imag64(const MatBuf64 *m, MatBuf64 *real, MatBuf64 *imag);
int32_t bdsp_hip_mat_get_mag_phase64(const MatBuf64 *m, MatBuf64 *mag, MatBuf64 *phase);
int32_t bdsp_hip_mat_set_real_imag64(MatBuf64 *m, const MatBuf64 *real, const MatBuf64 *imag);
int32_t bdsp_hip_mat_set_mag_phase64(MatBuf64 *m, const MatBuf64 *mag, const MatBuf64 *phase);
/* vector <-> matrix (matrix/src/to_from_mat_conversions.rs): see bdsp_hip_mat_from_frames32 */
int32_t bdsp_hip_mat_from_frames64(const VecBuf64 *vector, size_t frame_points, size_t hop, int32_t pad_tail, MatBuf64 **out);
int32_t bdsp_hip_mat_overlap_add64(const MatBuf64 *m, size_t hop, VecBuf64 **out);
int32_t bdsp_hip_mat_from_vectors64(const VecBuf64 *const *vectors, size_t count, MatBuf64 **out);
/* across the rows (data_reorganization.rs:477-555): see bdsp_hip_mat_transpose32 */
int32_t bdsp_hip_mat_transpose64(MatBuf64 *m);
int32_t bdsp_hip_mat_from_interleaved64(const VecBuf64 *vector, size_t channels, MatBuf64 **out);
int32_t bdsp_hip_mat_to_interleaved64(const MatBuf64 *m, VecBuf64 **out);
int32_t bdsp_hip_mat_zero_interleave64(MatBuf64 *m, int32_t factor);
/* chirp-z transform of a frequency band: see bdsp_hip_zoom_fft32 */
int32_t bdsp_hip_zoom_fft64(VecBuf64 *v, double start, double step, size_t bins);
int32_t bdsp_hip_mat_zoom_fft64(MatBuf64 *m, double start, double step, size_t bins);
int32_t bdsp_hip_mat_zoom_fft_starts64(MatBuf64 *m, const double *starts, size_t count, double step, size_t bins);
/* the product of two matrices: see bdsp_hip_mat_matmul32 */
int32_t bdsp_hip_mat_matmul64(const MatBuf64 *a, const MatBuf64 *b, int32_t b_conj_transposed, MatBuf64 **out);
/* Hermitian positive-definite systems: see bdsp_hip_mat_cholesky32 */
int32_t bdsp_hip_mat_cholesky64(const MatBuf64 *a, double loading, MatBuf64 **out);
int32_t bdsp_hip_mat_cholesky_solve64(const MatBuf64 *l, const MatBuf64 *b, int32_t part, MatBuf64 **out);
/* the eigendecomposition of a Hermitian matrix: see bdsp_hip_mat_eigh32 */
int32_t bdsp_hip_mat_eigh64(const MatBuf64 *a, MatBuf64 **w, MatBuf64 **v, int32_t *sweeps);
/* second-order-section filtering: see bdsp_hip_sosfilt32 */
int32_t bdsp_hip_sosfilt64(VecBuf64 *v, const double *sos, size_t sections, VecBuf64 *state /* may be NULL */);
int32_t bdsp_hip_mat_sosfilt64(MatBuf64 *m, const double *sos, size_t sections, MatBuf64 *state /* may be NULL */);
/* sliding order statistics: see bdsp_hip_rank_filter32 */
int32_t bdsp_hip_rank_filter64(VecBuf64 *v, size_t half, size_t rank, int64_t guard /* -1: none */, int32_t boundary);
int32_t bdsp_hip_mat_rank_filter64(MatBuf64 *m, size_t half, size_t rank, int64_t guard /* -1: none */, int32_t boundary);
/* detections as a compact list: see bdsp_hip_detect32 */
int32_t bdsp_hip_detect64(const VecBuf64 *v, int32_t kind, const void *threshold, size_t order, int32_t boundary,
                          size_t capacity, int64_t *counts /* 1 */, int64_t *index /* capacity */, double *value /* capacity */);
int32_t bdsp_hip_mat_detect64(const MatBuf64 *m, int32_t kind, const void *threshold, size_t order, int32_t boundary,
                              size_t capacity, int64_t *counts /* rows */, int64_t *index, double *value);
/* order statistics of every row: see bdsp_hip_sort32 */
int32_t bdsp_hip_sort64(VecBuf64 *v, int32_t descending);
int32_t bdsp_hip_mat_sort64(MatBuf64 *m, int32_t descending);
int32_t bdsp_hip_order_select64(const VecBuf64 *v, int32_t descending, size_t count, const uint64_t *ranks, int64_t *index, void *value);
int32_t bdsp_hip_mat_order_select64(const MatBuf64 *m, int32_t descending, size_t count, const uint64_t *ranks, int64_t *index, void *value);

/* ==========================================================================================
 * B3 -- kernels on caller-owned DEVICE memory.  `stream` is a hipStream_t passed as void*
 * (NULL = the library's own non-blocking stream; BDSP_HIP_STREAM_DEFAULT = HIP's null stream, the
 * stream a framework's "default stream" handle 0 stands for -- forward such a handle as
 * BDSP_HIP_STREAM_DEFAULT, never as 0).  Calls are asynchronous on that stream unless noted.
 * `elem` = 0 for f32, 1 for f64.  Scratch: ops that are not in place ping-pong between `data`
 * and `scratch` (same size); they return in *result_in_scratch whether the result ended in
 * `scratch` (1) or `data` (0), mirroring the reference's Buffer::trade (support_std.rs:78-82).
 * ======================================================================================== */

#define BDSP_HIP_STREAM_DEFAULT ((void *)1) /* HIP's null stream (same value as hipStreamLegacy) */

/* Unnormalised complex FFT of `batch` contiguous vectors of `points` complex each.
 * flags: BDSP_FFT_* bits. */
#define BDSP_FFT_INVERSE 1u      /* exp(+...) instead of exp(-...) */
#define BDSP_FFT_SHIFT_OUT 2u    /* fused fft_shift of the result (time_to_freq.rs:158-165) */
#define BDSP_FFT_SHIFT_IN 4u     /* fused ifft_shift of the input (freq_to_time.rs:160-168) */
#define BDSP_FFT_MAGNITUDE 8u    /* write |X| as `points` reals instead of complex (config C2) */
int bdsp_hip_dev_fft(int elem, void *data, void *scratch, size_t points, size_t batch,
                     unsigned flags, double in_scale, int window_id, double window_alpha,
                     int *result_in_scratch, void *stream);
/* Trips through device memory a power-of-two transform of `points` complex points makes (1: one workgroup-resident
 * kernel, 2 or 3: global Stockham passes) -- what bdsp_hip_dev_fft will launch for a PLAIN transform (no flags, scale or
 * window: f32 8192 points = 1, two passes once an option is fused); 0 for lengths that are not a power
 * of two (mixed-radix / chirp-z plans) or out of range.  The benchmark's per-pass figures read it from here. */
int bdsp_hip_fft_passes(int elem, size_t points);

/* Centred circular convolution (reference a9) of `batch` contiguous complex vectors of `points`
 * points with ONE shared filter of `taps` complex taps (device pointer), by fused overlap-save.
 * out must not alias in.  */
int bdsp_hip_dev_convolve(int elem, const void *in, void *out, size_t points, size_t batch,
                          const void *taps_dev, size_t taps, void *stream);

/* bdsp_hip_dev_convolve with the fused block kernel's dispatch-group shares given FOR THIS CALL: its persistent
 * workgroups are dispatched in groups (three for f32) and the groups dispatched first get a larger share of the blocks,
 * because the hardware issues the oldest wave first.  first_pct / second_pct = percent of the blocks for
 * the first / second group (defaults f32 43 / 37, f64 55 / -); (33, 33) = equal shares; (-1, -1) = the defaults, i.e.
 * bdsp_hip_dev_convolve.  The shares only move blocks between workgroups (bit-identical output); nothing outlives the
 * call and no other thread's launches see it -- the dispatch-order guard test times equal shares against the defaults
 * through this entry point.  BDSP_ERR_ARG_LENGTH for shares that leave the last group nothing to do. */
int bdsp_hip_dev_convolve_ex(int elem, const void *in, void *out, size_t points, size_t batch,
                             const void *taps_dev, size_t taps, int first_pct, int second_pct, void *stream);

/* The same convolution split in two, so a caller that reuses one filter (the batch driver, the
 * benchmark) builds its spectrum once: prepare writes bdsp_hip_conv_spectrum_points() complex
 * points (FFT of the zero-padded taps, pre-divided by the block length) to spectrum_dev;
 * convolve_prepared is the single fused overlap-save launch (taps <= 3073). */
size_t bdsp_hip_conv_spectrum_points(void);
int bdsp_hip_dev_conv_prepare(int elem, const void *taps_dev, size_t taps, void *spectrum_dev,
                              void *stream);
int bdsp_hip_dev_convolve_prepared(int elem, const void *in, void *out, size_t points, size_t batch,
                                   const void *spectrum_dev, size_t taps, void *stream);

/* Elementwise x[i] = x[i]*scale + offset is NOT offered (the reference never fuses them and a
 * fused multiply-add would round differently); separate entry points: */
int bdsp_hip_dev_real_scale(int elem, void *data, size_t len, double factor, void *stream);
int bdsp_hip_dev_real_offset(int elem, void *data, size_t len, int is_complex, double offset,
                             void *stream);

/* polyphase interpolatef (reference a13) on device memory; out holds
 * bdsp_hip_interpolatef_new_len(...) scalars. */
size_t bdsp_hip_interpolatef_new_len(int elem, size_t len, double factor);
int bdsp_hip_dev_interpolatef(int elem, const void *in, void *out, size_t len, int is_complex,
                              int function_id, double rolloff, double factor, double delay,
                              size_t conv_len, double delta, void *stream);

/* Blocks until everything queued on `stream` (NULL = library stream) has finished. */
int bdsp_hip_synchronize(void *stream);
/* Binds the calling thread's work to HIP device `ordinal` (one process per GPU: call once). */
int bdsp_hip_set_device(int ordinal);
/* Compute units of the bound device (256 on MI355X: 8 XCDs of 32); 0 without a device. */
int bdsp_hip_compute_units(void);

/* Timing hooks for bench.py: HIP events recorded on `stream`; elapsed milliseconds between
 * two recorded events.  (torch.cuda.Event only sees torch's current stream.) */
void *bdsp_hip_event_create(void);
int bdsp_hip_event_record(void *event, void *stream);
int bdsp_hip_event_elapsed_ms(void *start, void *stop, float *ms);
void bdsp_hip_event_destroy(void *event);

/* HIP graphs: capture a sequence of B2/B3 calls on one stream and replay it with a single launch
 * (small vectors are launch-bound).  Run the sequence once before capturing (tables, plans and workspace
 * are created on first use), replay on the capture stream, and keep host-facing calls (data32,
 * overwrite_data32, get_value32, B1 entry points, plain_sifft32) out of the captured region.
 * stream: hipStream_t as void*, NULL = the library's own stream (the one B2 handles use). */
int bdsp_hip_capture_begin(void *stream);
int bdsp_hip_capture_end(void *stream, void **graph_exec);
/* Drops an open capture without building a graph (a captured sequence that failed half way): the stream leaves capture
 * mode, pinned workspace and plans are released, the next capture_begin is accepted.  One capture at a time per
 * process, owned by the thread that opened it; other threads' calls neither disturb it nor are recorded by it. */
int bdsp_hip_capture_abort(void *stream);
/* The recovery route: drops the open capture from ANY thread.  For a process whose capturing thread exited or died
 * between capture_begin and capture_end -- bdsp_hip_capture_abort refuses other threads while the stream still records
 * (it accepts them once the stream no longer does), so without this every later capture_begin would be refused.  The
 * caller vouches that the owner is gone.  No-op (0) when no capture is open. */
int bdsp_hip_capture_reset(void *stream);
int bdsp_hip_graph_launch(void *graph_exec, void *stream);
void bdsp_hip_graph_destroy(void *graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_DSP_HIP_H */
