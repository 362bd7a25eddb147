// mat_sym.hip -- the symmetric real-signal transforms of a matrix (DspMat.plain_sfft / sfft / windowed_sfft,
// plain_sifft / sifft / windowed_sifft, mirror): the two index moves around the batched transforms.
//
// Replaces the row loop of the reference's matrix crate (matrix/src/time_freq.rs:83-107, 144-168 and 173-177 forward
// the traits to the rows one after the other); each row computes what time_to_freq.rs:188-298, freq_to_time.rs:180-248
// and freq.rs:52-83 compute.  One launch each, whatever the row count.
//
//   k_sy_crop_rows    out[r][j] = in[r][j], j < p, from rows of n = 2p - 1 bins: the non-redundant half of the full
//                     spectrum the batched real-input transform leaves (unmirror!)
//   k_sy_mirror_rows  everything op_sifft does before its transform: scale by 1/p and ifft_shift of the half spectrum
//                     (sifft / windowed_sifft), the "first bin must be real" test of every row (one flag word for the
//                     whole matrix), and the mirror to 2p - 1 bins.  With neither scale nor flag it is the public mirror.
//
// Both move one complex element per lane as one 8- or 16-byte packet (always aligned: a complex row starts at a
// multiple of the packet), walk the FLAT output index in a grid-stride loop -- so neither the row count nor where a row
// starts needs a special case -- and use 32-bit indices whenever the matrix allows (as reorg.hip).  The index maps are
// in mat_sym_core.h.
#include "bdsp_internal.h"
#include "mat_sym_core.h"

namespace bdsp {

static inline unsigned sy_grid(size_t n)
{
    size_t blocks = (n + 255) / 256;
    size_t cap = (size_t)num_cus() * 8;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks ? blocks : 1);
}

template <typename C, typename IDX>
__global__ __launch_bounds__(256) void k_sy_crop_rows(const C* __restrict__ in, C* __restrict__ out, IDX rows, IDX p)
{
    const IDX n = 2 * p - 1, total = rows * p;
    const IDX stride = (IDX)gridDim.x * blockDim.x;
    IDX o = (IDX)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    SyPos<IDX> at = sy_pos<IDX>(o, p);
    const SyPos<IDX> step = sy_stride<IDX>(stride, p);
    for (; o < total; o += stride) {
        out[o] = in[sy_crop_src<IDX>(at.row, at.col, n)];
        sy_advance<IDX>(&at, step, p);
    }
}

// h(j) = scale * in[r][(j + rot) mod p]; out[r][g] = g < p ? h(g) : conj(h(2p - 1 - g)).  The lane that writes g == 0
// tests h(0) against h(1) and raises *flag (flag may be null: no test).
template <typename C, typename IDX, bool SCALED>
__global__ __launch_bounds__(256) void k_sy_mirror_rows(const C* __restrict__ in, C* __restrict__ out, IDX rows, IDX p,
                                                         IDX rot, typename real_of<C>::type scale, unsigned* flag)
{
// the scale is ew_real_scale's: one multiply per component, each rounded on its own
#pragma clang fp contract(off)
    const IDX n = 2 * p - 1, total = rows * n;
    const IDX stride = (IDX)gridDim.x * blockDim.x;
    IDX o = (IDX)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    SyPos<IDX> at = sy_pos<IDX>(o, n);
    const SyPos<IDX> step = sy_stride<IDX>(stride, n);
    for (; o < total; o += stride) {
        const C* row = in + at.row * p;
        bool conj;
        C z = row[sy_mirror_bin<IDX>(at.col, p, rot, &conj)];
        if (SCALED) { z.x = z.x * scale; z.y = z.y * scale; }
        if (flag && at.col == 0) {
            double re1 = 0.0, im1 = 0.0;
            if (p > 1) {
                bool c1;
                C z1 = row[sy_mirror_bin<IDX>((IDX)1, p, rot, &c1)];
                if (SCALED) { z1.x = z1.x * scale; z1.y = z1.y * scale; }
                re1 = (double)z1.x;
                im1 = (double)z1.y;
            }
            if (sy_first_bin_fails((double)z.x, (double)z.y, re1, im1)) atomicOr(flag, 1u);
        }
        if (conj) z.y = -z.y;
        out[o] = z;
        sy_advance<IDX>(&at, step, n);
    }
}

// 32-bit indices while every flat index plus one grid stride stays below 2^32
static inline bool sy_fits_32(size_t span) { return span < (size_t(1) << 31); }

template <typename T>
int sy_crop_rows(const T* in, T* out, size_t rows, size_t p, hipStream_t s)
{
    if (rows == 0 || p == 0) return BDSP_OK;
    if (in == out) return BDSP_ERR_UNSUPPORTED;
    using C = cpx<T>;
    const C* i = reinterpret_cast<const C*>(in);
    C* o = reinterpret_cast<C*>(out);
    const size_t total = rows * p, span = rows * (2 * p - 1);
    if (sy_fits_32(span))
        hipLaunchKernelGGL((k_sy_crop_rows<C, unsigned>), dim3(sy_grid(total)), dim3(256), 0, s, i, o, (unsigned)rows, (unsigned)p);
    else
        hipLaunchKernelGGL((k_sy_crop_rows<C, size_t>), dim3(sy_grid(total)), dim3(256), 0, s, i, o, rows, p);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

template <typename T>
int sy_mirror_rows(const T* in, T* out, size_t rows, size_t p, size_t rot, bool scaled, T scale, unsigned* flag, hipStream_t s)
{
    if (rows == 0 || p == 0) return BDSP_OK;
    if (in == out || rot >= p) return BDSP_ERR_UNSUPPORTED;
    using C = cpx<T>;
    const C* i = reinterpret_cast<const C*>(in);
    C* o = reinterpret_cast<C*>(out);
    const size_t total = rows * (2 * p - 1);
    const dim3 grid(sy_grid(total)), block(256);
#define BDSP_SY(IDX, SC) hipLaunchKernelGGL((k_sy_mirror_rows<C, IDX, SC>), grid, block, 0, s, i, o, (IDX)rows, (IDX)p, (IDX)rot, scale, flag)
    if (sy_fits_32(total)) {
        if (scaled) BDSP_SY(unsigned, true);
        else BDSP_SY(unsigned, false);
    } else {
        if (scaled) BDSP_SY(size_t, true);
        else BDSP_SY(size_t, false);
    }
#undef BDSP_SY
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

#define BDSP_INST(T)                                                                               \
    template int sy_crop_rows<T>(const T*, T*, size_t, size_t, hipStream_t);                       \
    template int sy_mirror_rows<T>(const T*, T*, size_t, size_t, size_t, bool, T, unsigned*, hipStream_t);
BDSP_INST(float)
BDSP_INST(double)
#undef BDSP_INST

} // namespace bdsp
