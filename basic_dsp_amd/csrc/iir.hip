// iir.hip -- sosfilt: a cascade of second-order sections (direct form II transposed) along every row of a real or complex
// f32 / f64 matrix, in place (iir_core.h has the formulation, the LDS map, the scan tree and the per-lane arithmetic).
//
// One algorithm whatever the row count; the grid is rows x tiles of IIR_TILE points:
//   k_iir_tile   the tile goes coalesced into LDS and comes back so that every lane owns 16 consecutive points, which stay
//                in registers through all sections.  Per section: the chunk from a zero state (lane 0: from the tile's
//                incoming state), the tree over the 256 end states (six cross-lane steps inside a wave, the four wave
//                totals through LDS, one barrier), the chunk again from its true state.  The lane that owns the row's last
//                point stores the final state.
//   k_iir_carry  rows longer than a tile: s_(t+1) = M s_t + v_t along each row in double, one wave per row and channel.
// Rows of one tile: one launch.  Longer rows: k_iir_tile from zero states on every tile but the last, storing only the end
// states; k_iir_carry; k_iir_tile from the true states.  The launches are the only synchronisation between workgroups:
// no flag, no look-back.  Plain loads and stores only; every output is written by exactly one thread, once; the register
// arrays are indexed by unrolled loops alone, so there is no scratch.  tests/host_sim/sim_iir.cpp runs the functions of
// iir_core.h with threads as loops.
#include "bdsp_internal.h"
#include "iir_core.h"

namespace bdsp {

extern __shared__ __align__(16) unsigned char iir_smem[];

// blockIdx.x = row * grid_tiles + tile, grid_tiles = tiles (the whole row) or tiles - 1 (the zero-state pass).
// Incoming state of a tile: carry_in (doubles, iir_carry_index) if given, else state_in (T, iir_state_index) if given,
// else zero.  carry_out: every tile of the grid stores its end state there and no output.  state_out: the row's last
// tile stores the final state there.  state_in and state_out may be the same buffer: a row's state is read by lane 0
// before the section's barrier and written after it, by the same workgroup.
template <typename T, int C>
__global__ __launch_bounds__(IIR_THREADS) void k_iir_tile(T* data, size_t n, const IirSec<T>* __restrict__ tab, int S,
                                                           const T* state_in, const double* __restrict__ carry_in,
                                                           double* __restrict__ carry_out, T* state_out, unsigned tiles,
                                                           unsigned grid_tiles)
{
    constexpr int K = IIR_CHUNK * C; // scalars per lane
    T* lds = reinterpret_cast<T*>(iir_smem);
    const int tid = (int)threadIdx.x, lane = tid & (IIR_WAVE - 1), wave = tid / IIR_WAVE;
    const size_t row = blockIdx.x / grid_tiles, tile = blockIdx.x % grid_tiles;
    const int points = iir_tile_points(n, tile), scalars = points * C;
    T* at = data + (row * n + tile * (size_t)IIR_TILE) * (size_t)C;

    for (int k = 0; k < K; ++k) {
        const int g = k * IIR_THREADS + tid;
        lds[iir_lds_slot(g, C)] = g < scalars ? at[g] : (T)0;
    }
    __syncthreads();
    T x[K];
    const int mine = iir_lds_chunk(tid, C);
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = lds[mine + j];

    const bool owns_last = tid == iir_last_lane(points);
    // lanes past the row's end hold zeros that reach no stored value: they skip both runs and enter the tree with a zero
    // state (rows much shorter than a tile leave whole waves idle)
    const bool live = tid <= iir_last_lane(points);
    const int last_step = iir_last_count(points) - 1;
    const bool stores_state = owns_last && (carry_out || (state_out && tile + 1 == tiles));

    for (int sec = 0; sec < S; ++sec) {
        const IirSec<T> cf = tab[sec];
        T s0[C][2], v[C][2], ex[C][2];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            s0[c][0] = s0[c][1] = (T)0;
            if (tid == 0) {
                if (carry_in) {
                    s0[c][0] = (T)carry_in[iir_carry_index(row, tiles, tile, C, c, S, 2 * sec)];
                    s0[c][1] = (T)carry_in[iir_carry_index(row, tiles, tile, C, c, S, 2 * sec + 1)];
                } else if (state_in) {
                    s0[c][0] = state_in[iir_state_index(row, C, c, S, 2 * sec)];
                    s0[c][1] = state_in[iir_state_index(row, C, c, S, 2 * sec + 1)];
                }
            }
            T s1 = s0[c][0], s2 = s0[c][1];
            if (live) {
#pragma unroll
                for (int j = 0; j < IIR_CHUNK; ++j) (void)iir_step<T>(cf, x[j * C + c], &s1, &s2);
            }
            v[c][0] = s1;
            v[c][1] = s2;
        }
#pragma unroll
        for (int k = 0; k < IIR_IN_WAVE_STEPS; ++k) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const T f1 = __shfl_up(v[c][0], 1u << k), f2 = __shfl_up(v[c][1], 1u << k);
                iir_scan_step<T>(cf, k, lane, f1, f2, &v[c][0], &v[c][1]);
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            ex[c][0] = __shfl_up(v[c][0], 1u);
            ex[c][1] = __shfl_up(v[c][1], 1u);
            if (lane == IIR_WAVE - 1) {
                lds[iir_lds_total(sec, wave, C, c, 0)] = v[c][0];
                lds[iir_lds_total(sec, wave, C, c, 1)] = v[c][1];
            }
        }
        __syncthreads(); // (the next section writes the other slot: one barrier per section)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            T in1 = (T)0, in2 = (T)0, s1, s2, f1 = (T)0, f2 = (T)0;
            if (wave > 0) iir_wave_in<T>(cf, lds + iir_lds_total(sec, 0, C, c, 0), 2 * C, wave, &in1, &in2);
            iir_lane_in<T>(cf, wave, lane, ex[c][0], ex[c][1], in1, in2, s0[c][0], s0[c][1], &s1, &s2);
            if (live) {
#pragma unroll
                for (int j = 0; j < IIR_CHUNK; ++j) {
                    x[j * C + c] = iir_step<T>(cf, x[j * C + c], &s1, &s2);
                    if (j == last_step) { f1 = s1; f2 = s2; }
                }
            }
            if (stores_state) {
                if (carry_out) {
                    carry_out[iir_carry_index(row, tiles, tile, C, c, S, 2 * sec)] = (double)f1;
                    carry_out[iir_carry_index(row, tiles, tile, C, c, S, 2 * sec + 1)] = (double)f2;
                } else {
                    state_out[iir_state_index(row, C, c, S, 2 * sec)] = f1;
                    state_out[iir_state_index(row, C, c, S, 2 * sec + 1)] = f2;
                }
            }
        }
    }
    if (carry_out) return; // (uniform: the zero-state pass stores no output)
    // every lane overwrites the chunk that only it has read
#pragma unroll
    for (int j = 0; j < K; ++j) lds[mine + j] = x[j];
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const int g = k * IIR_THREADS + tid;
        if (g < scalars) at[g] = lds[iir_lds_slot(g, C)];
    }
}

// blockIdx.x = row * C + channel; lane i < 2S carries component i.  Slot t of the row's carry buffer holds v_t coming in
// (t < tiles - 1) and s_t, the state entering tile t, going out.
template <typename T>
__global__ __launch_bounds__(IIR_WAVE) void k_iir_carry(double* buf, const T* __restrict__ state_in, const double* __restrict__ m,
                                                         int S, int C, unsigned tiles)
{
    __shared__ double mt[4 * IIR_MAX_SECTIONS * IIR_MAX_SECTIONS];
    __shared__ double sl[2 * IIR_MAX_SECTIONS];
    const int i = (int)threadIdx.x, n2 = 2 * S, c = (int)(blockIdx.x % (unsigned)C);
    const size_t row = blockIdx.x / (unsigned)C;
    const bool on = i < n2;
    for (int e = i; e < n2 * n2; e += IIR_WAVE) mt[(e % n2) * n2 + e / n2] = m[e];
    double s = on && state_in ? (double)state_in[iir_state_index(row, C, c, S, i)] : 0.0;
    double* slot = buf + iir_carry_index(row, tiles, 0, C, c, S, on ? i : 0);
    const size_t pitch = (size_t)C * (size_t)n2;
    for (unsigned t0 = 0; t0 < tiles; t0 += IIR_CARRY_BATCH) {
        double vb[IIR_CARRY_BATCH];
#pragma unroll
        for (int u = 0; u < IIR_CARRY_BATCH; ++u) vb[u] = on && t0 + u + 1 < tiles ? slot[(size_t)(t0 + u) * pitch] : 0.0;
#pragma unroll
        for (int u = 0; u < IIR_CARRY_BATCH; ++u) {
            if (t0 + u >= tiles) break; // (uniform)
            if (on) { slot[(size_t)(t0 + u) * pitch] = s; sl[i] = s; }
            __syncthreads();
            const double next = on ? iir_carry_dot(mt, sl, n2, i, vb[u]) : 0.0;
            __syncthreads();
            s = next;
        }
    }
}

size_t iir_carry_doubles(size_t rows, size_t n, bool is_complex, size_t S)
{
    return iir_launches(n) < 3 ? 0 : rows * iir_tiles(n) * (is_complex ? 2 : 1) * 2 * S;
}

template <typename T, int C>
static int iir_run(T* data, size_t rows, size_t n, const IirSec<T>* tab, size_t S, T* state, const double* m, double* carry,
                   hipStream_t s)
{
    const size_t tiles = iir_tiles(n), lds = sizeof(T) * (size_t)iir_lds_scalars(C);
    if (rows > 0x7fffffffu / tiles) { set_last_error("sosfilt: rows x tiles above 2^31"); return BDSP_ERR_UNSUPPORTED; }
    auto kern = k_iir_tile<T, C>;
    if (iir_launches(n) == 1) {
        BDSP_TRY(kernel_lds(kern, lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(IIR_THREADS), lds, s, data, n, tab, (int)S, (const T*)state,
                           (const double*)nullptr, (double*)nullptr, state, 1u, 1u);
        BDSP_LAUNCH_CHECK();
        return BDSP_OK;
    }
    if (!carry || !m) return BDSP_ERR_UNSUPPORTED;
    BDSP_TRY(kernel_lds(kern, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(rows * (tiles - 1))), dim3(IIR_THREADS), lds, s, data, n, tab, (int)S, (const T*)nullptr,
                       (const double*)nullptr, carry, (T*)nullptr, (unsigned)tiles, (unsigned)(tiles - 1));
    BDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_iir_carry<T>), dim3((unsigned)(rows * C)), dim3(IIR_WAVE), 0, s, carry, (const T*)state, m, (int)S, C,
                       (unsigned)tiles);
    BDSP_LAUNCH_CHECK();
    BDSP_TRY(kernel_lds(kern, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(rows * tiles)), dim3(IIR_THREADS), lds, s, data, n, tab, (int)S, (const T*)nullptr,
                       (const double*)carry, (double*)nullptr, state, (unsigned)tiles, (unsigned)tiles);
    BDSP_LAUNCH_CHECK();
    return BDSP_OK;
}

// data: rows x n points in place; tab: S sections, m: the (2S)^2 transition and carry: iir_carry_doubles doubles, both
// only for rows longer than a tile; state (may be null): rows x 2S points, read and overwritten.  rows, n, S > 0
template <typename T>
int iir_sosfilt(T* data, size_t rows, size_t n, bool is_complex, const IirSec<T>* tab, size_t S, T* state, const double* m,
                double* carry, hipStream_t s)
{
    if (is_complex) return iir_run<T, 2>(data, rows, n, tab, S, state, m, carry, s);
    return iir_run<T, 1>(data, rows, n, tab, S, state, m, carry, s);
}

template int iir_sosfilt<float>(float*, size_t, size_t, bool, const IirSec<float>*, size_t, float*, const double*, double*, hipStream_t);
template int iir_sosfilt<double>(double*, size_t, size_t, bool, const IirSec<double>*, size_t, double*, const double*, double*, hipStream_t);

} // namespace bdsp
