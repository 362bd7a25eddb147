// sim_mat_mul.cpp -- the dispatch rule, index maps and lane arithmetic of basic_dsp_amd/csrc/mat_mul_core.h on the host,
// threads as loops.  usage: sim_mat_mul <tests/mat_mul_shapes.txt>
//
// For every line "path form M K N" of the shape file, in f32 and f64, real and complex:
//   * mm_dispatch returns the path the line names;
//   * the kernel of that path, written out here with the core header's maps (work item -> tile, staging slots, the
//     matrix instruction's operand and result lanes, the 4 x 4 blocks of the f64 kernel, the streaming kernel's LDS image
//     and column runs, the split chunks), writes every element of C -- of every partial, on the split path -- exactly
//     once, reads nothing outside a, b or the declared LDS planes, and the number of partials is mm_split_chunks;
//   * the result is bit-equal (==) to a plain triple loop: one chain over ascending k from +0 per element (fmaf / fma,
//     mm_cplx_step for complex), chunk sums added in ascending order -- with v_mfma_f32_32x32x2_f32 modelled as the
//     k-ordered fmaf chain it is documented to be, operands gathered and results scattered by the documented lane maps
//     (one instruction takes two k, so the triple loop of the complex f32 kernel takes the real sum's products in pairs
//     of k: mm_cplx_step); full tiles and edge tiles alike;
//   * and within (2 K + 4) eps sum |a| |b| of the product in long double (which would catch a sign both share).
// LDS: every staging write and every fragment read of the f32 kernel, and every staging write of the f64 kernel, is
// counted for bank conflicts from mm_lds_slot and the lane groups (32 lanes for 4-byte accesses, 16 for 8-byte writes):
// 0 is claimed and checked; a pitch of 64 instead of 65 is counted too, to show that the rule bites.
// Shapes above 2^22 multiply-adds are checked against the dispatch rule only (the GPU test runs them).
// Then the chunk arithmetic alone on a grid of (M, N, K) up to 2^24, where the chunks grow past the minimum.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <complex>
#include <string>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_mul_core.h"

using namespace bdsp;

static long g_fails = 0;
#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++g_fails < 20) { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                          \
    } while (0)

struct HostFma {
    float operator()(float a, float b, float c) const { return fmaf(a, b, c); }
    double operator()(double a, double b, double c) const { return fma(a, b, c); }
};

// one wave's operand register and accumulator registers, and the matrix instruction on them
struct WaveVec {
    float v[MM_LANES];
    WaveVec operator-() const { WaveVec r; for (int l = 0; l < MM_LANES; ++l) r.v[l] = -v[l]; return r; }
};
struct WaveAcc { float c[MM_LANES][16]; };
struct MfmaModel {
    WaveAcc operator()(const WaveVec& a, const WaveVec& b, WaveAcc c) const
    {
        float A[32][2], B[2][32];
        for (int l = 0; l < MM_LANES; ++l) {
            A[mm_mfma_ab_x(l)][mm_mfma_ab_k(l)] = a.v[l];
            B[mm_mfma_ab_k(l)][mm_mfma_ab_x(l)] = b.v[l];
        }
        for (int l = 0; l < MM_LANES; ++l)
            for (int g = 0; g < 16; ++g)
                for (int k = 0; k < 2; ++k) c.c[l][g] = fmaf(A[mm_mfma_c_row(l, g)][k], B[k][mm_mfma_c_col(l)], c.c[l][g]);
        return c;
    }
};

static long g_conflicts = 0, g_conflicts_pitch64 = 0, g_lds_accesses = 0;
// `slots` of the 256 threads of one instruction, elements of `dwords` dwords, lane groups of `group`
static void count_conflicts(const int* slots, int dwords, int group)
{
    for (int g0 = 0; g0 < MM_THREADS; g0 += group) {
        unsigned banks = 0, banks64 = 0;
        for (int l = g0; l < g0 + group; ++l)
            for (int d = 0; d < dwords; ++d) {
                banks |= 1u << ((slots[l] * dwords + d) % 32);
                const int k = slots[l] / MM_PITCH, x = slots[l] % MM_PITCH;
                banks64 |= 1u << (((k * 64 + x) * dwords + d) % 32);
            }
        g_conflicts += group * dwords - __builtin_popcount(banks);
        g_conflicts_pitch64 += group * dwords - __builtin_popcount(banks64);
        ++g_lds_accesses;
    }
}

template <typename T>
static T rd(const std::vector<T>& v, size_t i, const char* what)
{
    CHECK(i < v.size(), "%s read at %zu of %zu", what, i, v.size());
    return i < v.size() ? v[i] : (T)0;
}

// the tiled kernel (one chunk) and the split kernel: part[chunk][M][N][E], cnt = writes per scalar
template <typename T, bool CPLX>
static void sim_tiled(const std::vector<T>& a, const std::vector<T>& b, size_t M, size_t N, size_t K, bool trans,
                      size_t chunk_len, size_t nchunks, std::vector<T>& part, std::vector<int>& cnt)
{
    constexpr bool DBL = sizeof(T) == 8;
    constexpr int TK = mm_tk(DBL), E = CPLX ? 2 : 1, PL = mm_plane_elems(TK), DW = DBL ? 2 : 1;
    const size_t tiles_n = mm_tiles_along(N, MM_TN), ntiles = mm_tiles(M, N), nwork = ntiles * nchunks;
    std::vector<T> sA(E * PL), sB(E * PL);
    int slots[MM_THREADS];
    auto put = [&](std::vector<T>& plane, int k, int x, T re, T im, int tid) {
        const int s = mm_lds_slot(k, x);
        CHECK(k >= 0 && k < TK && x >= 0 && x < MM_TM && s < PL, "LDS slot k %d x %d", k, x);
        plane[s] = re;
        if (CPLX) plane[PL + s] = im;
        slots[tid] = s;
    };
    auto stage_rows = [&](const std::vector<T>& src, std::vector<T>& plane, size_t X, size_t x0, size_t k0, size_t kend, bool neg) {
        for (int r = 0; r < mm_stage_steps(TK); ++r) {
            for (int tid = 0; tid < MM_THREADS; ++tid) {
                int x, k;
                mm_stage_kc(tid, r, TK, &x, &k);
                const size_t gx = x0 + x, gk = k0 + k;
                T re = 0, im = 0;
                if (gx < X && gk < kend) {
                    re = rd(src, (gx * K + gk) * E, "rows");
                    if (CPLX) im = rd(src, (gx * K + gk) * E + 1, "rows");
                    if (neg) im = -im;
                }
                put(plane, k, x, re, im, tid);
            }
            count_conflicts(slots, DW, DBL ? 16 : 32);
        }
    };
    auto stage_cols = [&](const std::vector<T>& src, std::vector<T>& plane, size_t j0, size_t k0, size_t kend) {
        for (int r = 0; r < mm_stage_steps(TK); ++r) {
            for (int tid = 0; tid < MM_THREADS; ++tid) {
                int x, k;
                mm_stage_xc(tid, r, &x, &k);
                const size_t gx = j0 + x, gk = k0 + k;
                T re = 0, im = 0;
                if (gx < N && gk < kend) {
                    re = rd(src, (gk * N + gx) * E, "cols");
                    if (CPLX) im = rd(src, (gk * N + gx) * E + 1, "cols");
                }
                put(plane, k, x, re, im, tid);
            }
            count_conflicts(slots, DW, DBL ? 16 : 32);
        }
    };
    auto store = [&](size_t chunk, size_t row, size_t col, T re, T im) {
        if (row >= M || col >= N) return;
        const size_t at = chunk * (M * N * E) + (row * N + col) * E;
        CHECK(at + E <= part.size(), "store at %zu of %zu", at, part.size());
        part[at] = re;
        ++cnt[at];
        if (CPLX) { part[at + 1] = im; ++cnt[at + 1]; }
    };
    for (size_t w = 0; w < nwork; ++w) {
        size_t chunk, i0, j0;
        mm_work_item(w, ntiles, tiles_n, &chunk, &i0, &j0);
        const size_t kbeg = chunk * chunk_len, kend = K - kbeg < chunk_len ? K : kbeg + chunk_len;
        CHECK(chunk < nchunks && kbeg < K, "chunk %zu of %zu", chunk, nchunks);
        static WaveAcc re[4], ia[4], ib[4];                     // f32: per wave
        static T vre[MM_THREADS][4][4], via[MM_THREADS][4][4], vib[MM_THREADS][4][4]; // f64: per thread
        memset(re, 0, sizeof(re)); memset(ia, 0, sizeof(ia)); memset(ib, 0, sizeof(ib));
        memset(vre, 0, sizeof(vre)); memset(via, 0, sizeof(via)); memset(vib, 0, sizeof(vib));
        for (size_t k0 = kbeg; k0 < kend; k0 += TK) {
            stage_rows(a, sA, M, i0, k0, kend, false);
            if (trans) stage_rows(b, sB, N, j0, k0, kend, true);
            else stage_cols(b, sB, j0, k0, kend);
            if (!DBL) {
                for (int kk = 0; kk < TK; kk += 2) {
                    int sa[MM_THREADS], sb[MM_THREADS];
                    for (int wave = 0; wave < 4; ++wave) {
                        WaveVec ar, ai, br, bi;
                        for (int lane = 0; lane < MM_LANES; ++lane) {
                            const int pa = mm_lds_slot(kk + mm_mfma_ab_k(lane), mm_wave_row0(wave) + mm_mfma_ab_x(lane));
                            const int pb = mm_lds_slot(kk + mm_mfma_ab_k(lane), mm_wave_col0(wave) + mm_mfma_ab_x(lane));
                            CHECK(pa < PL && pb < PL, "fragment slot");
                            sa[wave * MM_LANES + lane] = pa;
                            sb[wave * MM_LANES + lane] = pb;
                            ar.v[lane] = (float)sA[pa]; br.v[lane] = (float)sB[pb];
                            ai.v[lane] = CPLX ? (float)sA[PL + pa] : 0.f; bi.v[lane] = CPLX ? (float)sB[PL + pb] : 0.f;
                        }
                        if (CPLX) mm_cplx_step(ar, ai, br, bi, &re[wave], &ia[wave], &ib[wave], MfmaModel());
                        else re[wave] = MfmaModel()(ar, br, re[wave]);
                    }
                    count_conflicts(sa, 1, 32);
                    count_conflicts(sb, 1, 32);
                }
            } else {
                for (int tid = 0; tid < MM_THREADS; ++tid)
                    for (int kk = 0; kk < TK; ++kk)
                        for (int r = 0; r < 4; ++r)
                            for (int c = 0; c < 4; ++c) {
                                const int pa = mm_lds_slot(kk, mm_valu_row(tid, r)), pb = mm_lds_slot(kk, mm_valu_col(tid, c));
                                CHECK(pa < PL && pb < PL, "block slot");
                                if (CPLX) mm_cplx_step(sA[pa], sA[PL + pa], sB[pb], sB[PL + pb], &vre[tid][r][c], &via[tid][r][c], &vib[tid][r][c], HostFma());
                                else vre[tid][r][c] = HostFma()(sA[pa], sB[pb], vre[tid][r][c]);
                            }
            }
        }
        if (!DBL) {
            for (int wave = 0; wave < 4; ++wave)
                for (int lane = 0; lane < MM_LANES; ++lane)
                    for (int g = 0; g < 16; ++g)
                        store(chunk, i0 + mm_wave_row0(wave) + mm_mfma_c_row(lane, g), j0 + mm_wave_col0(wave) + mm_mfma_c_col(lane),
                              (T)re[wave].c[lane][g], (T)(ia[wave].c[lane][g] + ib[wave].c[lane][g]));
        } else {
            for (int tid = 0; tid < MM_THREADS; ++tid)
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c)
                        store(chunk, i0 + mm_valu_row(tid, r), j0 + mm_valu_col(tid, c), vre[tid][r][c], via[tid][r][c] + vib[tid][r][c]);
        }
    }
}

template <typename T, bool CPLX>
static void sim_stream(const std::vector<T>& a, const std::vector<T>& b, size_t M, size_t N, size_t K, std::vector<T>& out,
                       std::vector<int>& cnt)
{
    constexpr int E = CPLX ? 2 : 1;
    const int MB = mm_stream_mb(M), kn = (int)K, mn = (int)M;
    CHECK((size_t)MB >= M && M <= MM_STREAM_MAX_M && K <= MM_STREAM_MAX_K, "stream limits");
    std::vector<T> sa(MM_STREAM_MAX_K * MB * E, (T)NAN);
    for (int idx = 0; idx < kn * MB * E; ++idx) {
        const int c = idx % E, m = (idx / E) % MB, k = idx / (E * MB);
        CHECK(idx == mm_stream_slot(m, k, c, MB, E), "stream slot");
        sa[idx] = m < mn ? rd(a, ((size_t)m * K + k) * E + c, "a") : (T)0;
    }
    const size_t nruns = (N + MM_STREAM_COLS - 1) / MM_STREAM_COLS;
    for (size_t run = 0; run < nruns; ++run)
        for (int tid = 0; tid < MM_THREADS; ++tid) {
            const size_t n = run * MM_STREAM_COLS + tid;
            if (n >= N) continue;
            T re[16] = {}, ia[16] = {}, ib[16] = {};
            for (int k = 0; k < kn; ++k) {
                const T br = rd(b, ((size_t)k * N + n) * E, "b"), bi = CPLX ? rd(b, ((size_t)k * N + n) * E + 1, "b") : (T)0;
                for (int m = 0; m < MB; ++m) {
                    if (CPLX)
                        mm_cplx_step(rd(sa, mm_stream_slot(m, k, 0, MB, E), "sa"), rd(sa, mm_stream_slot(m, k, E - 1, MB, E), "sa"), br,
                                     bi, &re[m], &ia[m], &ib[m], HostFma());
                    else re[m] = HostFma()(rd(sa, mm_stream_slot(m, k, 0, MB, E), "sa"), br, re[m]);
                }
            }
            for (int m = 0; m < MB; ++m)
                if (m < mn) {
                    const size_t at = ((size_t)m * N + n) * E;
                    CHECK(at + E <= out.size(), "stream store");
                    out[at] = re[m]; ++cnt[at];
                    if (CPLX) { out[at + 1] = ia[m] + ib[m]; ++cnt[at + 1]; }
                }
        }
}

static unsigned long long g_seed = 88172645463325252ull;
static double rnd()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (double)(g_seed >> 11) / 9007199254740992.0;
}
template <typename T>
static std::vector<T> fill(size_t n)
{
    std::vector<T> v(n);
    for (auto& x : v) {
        const double mag = pow(10.0, 4.0 * rnd() - 2.0), u = 2.0 * rnd() - 1.0;
        x = rnd() < 0.02 ? (T)0 : (T)(u * mag);
    }
    return v;
}

template <typename T, bool CPLX>
static double run_shape(MmPath path, bool trans, size_t M, size_t K, size_t N)
{
    constexpr int E = CPLX ? 2 : 1;
    const std::vector<T> a = fill<T>(M * K * E), b = fill<T>(K * N * E);
    const size_t total = M * N * E;
    const size_t chunk_len = path == MM_PATH_SPLIT ? mm_split_chunk(M, N, K) : K;
    const size_t nchunks = path == MM_PATH_SPLIT ? mm_split_chunks(M, N, K) : 1;
    std::vector<T> part(total * nchunks, (T)NAN), out(total);
    std::vector<int> cnt(total * nchunks, 0);
    if (path == MM_PATH_STREAM) sim_stream<T, CPLX>(a, b, M, N, K, part, cnt);
    else sim_tiled<T, CPLX>(a, b, M, N, K, trans, chunk_len, nchunks, part, cnt);
    for (size_t i = 0; i < cnt.size(); ++i) CHECK(cnt[i] == 1, "element %zu of %zu written %d times", i, cnt.size(), cnt[i]);
    for (size_t i = 0; i < total; ++i) { // k_mm_split_sum
        T s = part[i];
        for (size_t c = 1; c < nchunks; ++c) s += part[c * total + i];
        out[i] = s;
    }
    // the plain triple loop, and the product in long double
    const T eps = std::numeric_limits<T>::epsilon();
    const bool pairs = sizeof(T) == 4 && path != MM_PATH_STREAM;
    double worst = 0;
    auto A = [&](size_t i, size_t k, int c) { return a[(i * K + k) * E + c]; };
    auto B = [&](size_t k, size_t j, int c) { // b' = B or conj(B)^T
        if (!trans) return b[(k * N + j) * E + c];
        const T v = b[(j * K + k) * E + c];
        return c ? -v : v;
    };
    for (size_t i = 0; i < M; ++i)
        for (size_t j = 0; j < N; ++j) {
            T sum_re = 0, sum_im = 0;
            std::complex<long double> exact = 0;
            long double mod = 0;
            for (size_t c = 0; c < nchunks; ++c) {
                T re = 0, ia = 0, ib = 0;
                const size_t kend = K < (c + 1) * chunk_len ? K : (c + 1) * chunk_len;
                for (size_t k = c * chunk_len; k < kend; ++k) {
                    if (CPLX && pairs) { // one matrix instruction takes two k: see mm_cplx_step
                        if ((k - c * chunk_len) % 2) continue;
                        const bool two = k + 1 < kend;
                        re = fmaf(A(i, k, 0), B(k, j, 0), re);
                        if (two) re = fmaf(A(i, k + 1, 0), B(k + 1, j, 0), re);
                        re = fmaf(-A(i, k, 1), B(k, j, 1), re);
                        if (two) re = fmaf(-A(i, k + 1, 1), B(k + 1, j, 1), re);
                        for (size_t q = k; q < k + 1 + two; ++q) {
                            ia = fmaf(A(i, q, 0), B(q, j, 1), ia);
                            ib = fmaf(A(i, q, 1), B(q, j, 0), ib);
                        }
                    } else if (CPLX) mm_cplx_step(A(i, k, 0), A(i, k, E - 1), B(k, j, 0), B(k, j, E - 1), &re, &ia, &ib, HostFma());
                    else re = HostFma()(A(i, k, 0), B(k, j, 0), re);
                }
                sum_re = c ? sum_re + re : re;
                sum_im = c ? sum_im + (ia + ib) : ia + ib;
            }
            for (size_t k = 0; k < K; ++k) {
                const std::complex<long double> x(A(i, k, 0), CPLX ? A(i, k, E - 1) : 0), y(B(k, j, 0), CPLX ? B(k, j, E - 1) : 0);
                exact += x * y;
                mod += std::abs(x) * std::abs(y);
            }
            const T ore = out[(i * N + j) * E], oim = CPLX ? out[(i * N + j) * E + 1] : (T)0;
            CHECK(ore == sum_re && oim == sum_im, "(%zu, %zu): %g %g, triple loop %g %g", i, j, (double)ore, (double)oim, (double)sum_re, (double)sum_im);
            const long double err = std::abs(std::complex<long double>(ore, oim) - exact), bound = (2 * K + 4) * (long double)eps * mod;
            CHECK(err <= bound, "(%zu, %zu): error %Lg above the bound %Lg", i, j, err, bound);
            if (bound > 0 && (double)(err / bound) > worst) worst = (double)(err / bound);
        }
    return worst;
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: %s <shape file>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("FAIL cannot open %s\n", argv[1]); return 2; }
    static const char* names[] = {"stream", "tiled", "split"};
    char line[256];
    int shapes = 0, large = 0, per_path[3] = {0, 0, 0};
    double worst[3][2] = {{0, 0}, {0, 0}, {0, 0}};
    while (fgets(line, sizeof(line), f)) {
        char p[32], form[32];
        size_t M, K, N;
        if (line[0] == '#' || sscanf(line, "%31s %31s %zu %zu %zu", p, form, &M, &K, &N) != 5) continue;
        const bool trans = !strcmp(form, "trans");
        CHECK(trans || !strcmp(form, "plain"), "form %s", form);
        const MmPath path = mm_dispatch(M, N, K, trans);
        CHECK(!strcmp(names[path], p), "%s %s %zu %zu %zu: dispatch says %s", p, form, M, K, N, names[path]);
        ++shapes;
        ++per_path[path];
        if (M * K * N > ((size_t)1 << 22)) { ++large; continue; } // the dispatch rule only: the GPU test runs these
        auto up = [&](int prec, double r) { if (r > worst[path][prec]) worst[path][prec] = r; };
        up(0, run_shape<float, false>(path, trans, M, K, N));
        up(0, run_shape<float, true>(path, trans, M, K, N));
        up(1, run_shape<double, false>(path, trans, M, K, N));
        up(1, run_shape<double, true>(path, trans, M, K, N));
    }
    fclose(f);
    for (int p = 0; p < 3; ++p)
        printf("%-6s %3d shapes, worst error / bound: f32 %.3f  f64 %.3f\n", names[p], per_path[p], worst[p][0], worst[p][1]);
    CHECK(per_path[0] >= 20 && per_path[1] >= 20 && per_path[2] >= 20, "shapes per path");
    printf("LDS: %ld wave accesses counted, %ld bank conflicts at pitch %d (%ld at pitch 64)\n", g_lds_accesses, g_conflicts, MM_PITCH,
           g_conflicts_pitch64);
    CHECK(g_conflicts == 0, "bank conflicts");
    CHECK(g_conflicts_pitch64 > 0, "the conflict count does not bite");
    CHECK(2 * mm_plane_elems(mm_tk(false)) * 2 * sizeof(float) <= 65536 && 2 * mm_plane_elems(mm_tk(true)) * 2 * sizeof(double) <= 65536,
          "LDS planes above 64 KB");
    // the chunk arithmetic on its own: the chunks cover K exactly once, are multiples of both tile depths, never more
    // work items than the target (or one chunk per tile), and grow past the minimum for long K
    long combos = 0, grown = 0;
    const size_t dims[] = {1, 63, 64, 65, 129, 448, 449, 512}, ks[] = {256, 511, 512, 513, 1025, 8192, 8193, 8200, 65536, 1000003, (size_t)1 << 24};
    for (size_t M : dims)
        for (size_t N : dims)
            for (size_t K : ks) {
                if (mm_dispatch(M, N, K, true) != MM_PATH_SPLIT) continue;
                const size_t c = mm_split_chunk(M, N, K), n = mm_split_chunks(M, N, K);
                CHECK(c % 32 == 0 && c >= MM_SPLIT_MIN_CHUNK, "chunk %zu", c);
                CHECK(n >= 1 && (n - 1) * c < K && n * c >= K, "%zu chunks of %zu for K %zu", n, c, K);
                CHECK(c == MM_SPLIT_MIN_CHUNK || n * mm_tiles(M, N) <= MM_SPLIT_TARGET_BLOCKS, "%zu chunks x %zu tiles", n, mm_tiles(M, N));
                ++combos;
                grown += c > MM_SPLIT_MIN_CHUNK;
            }
    printf("chunks: %ld shapes, %ld with chunks above %zu; 512 x 8200 x 512 -> %zu chunks of %zu\n", combos, grown, MM_SPLIT_MIN_CHUNK,
           mm_split_chunks(512, 512, 8200), mm_split_chunk(512, 512, 8200));
    CHECK(grown > 0 && mm_split_chunk(512, 512, 8200) == 544, "chunk growth");
    printf("%d shapes (%d of them checked against the dispatch rule only), %ld failures\n%s\n", shapes, large, g_fails, g_fails ? "FAILED" : "ok");
    return g_fails ? 1 : 0;
}
