// sim_iir.cpp -- host simulation of iir.hip: the functions of iir_core.h driven with threads as loops, phase by phase as
// the kernels run them (a cross-lane move is a read of the previous phase's array).  Stand-alone: g++ -O2 -std=c++17
// -ffp-contract=off sim_iir.cpp, plainly or with -fsanitize=address,undefined; run with tests/iir_shapes.txt.  It checks
//   * the plan: launches, grids and tile sizes of the one-tile and the three-launch form;
//   * every output scalar and every state scalar is written exactly once, nothing past a row's end;
//   * the LDS map: inside the allocation, a bijection, and the bank cycles iir_core.h claims;
//   * the scan tree: every step joins adjacent runs of chunks with the table whose power is the run's length, and the
//     tables are the powers of A they are named after;
//   * accuracy: e_dev / max(e_ser, eps max|truth|) per row against the serial recurrence in long double, e_ser the error of
//     the serial recurrence in T with separately rounded operations -- the worst ratio is printed.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../basic_dsp_amd/csrc/iir_core.h"

using namespace bdsp;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        if (!(cond)) { ++g_fail; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// the families of tests/iir_shapes.txt: pole pairs r e^(+-i theta), a1 = -2 r cos theta, a2 = r^2, zeros at -1, unit gain
// at DC; section 0 of `resonator` has r = 0.9995, of `integrator` is [1 0 0 1 -1 0]; `fir` has a1 = a2 = 0
static std::vector<double> make_sos(const std::string& family, int S)
{
    const double pi = 3.14159265358979323846;
    std::vector<double> sos((size_t)6 * S);
    for (int k = 0; k < S; ++k) {
        double* c = &sos[6 * k];
        if (family == "fir") { c[0] = 0.25; c[1] = 0.5; c[2] = 0.25; c[3] = 1; c[4] = 0; c[5] = 0; continue; }
        if (family == "integrator" && k == 0) { c[0] = 1; c[1] = 0; c[2] = 0; c[3] = 1; c[4] = -1; c[5] = 0; continue; }
        double r = 0.70 + 0.25 * (k + 1) / (S + 1), th = pi * (0.10 + 0.15 * k / S);
        if (family == "resonator" && k == 0) { r = 0.9995; th = 0.05 * pi; }
        const double a1 = -2 * r * cos(th), a2 = r * r, g = (1 + a1 + a2) / 4;
        c[0] = g; c[1] = 2 * g; c[2] = g; c[3] = 1; c[4] = a1; c[5] = a2;
    }
    return sos;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double uniform()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_rng >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

struct Counts {
    std::vector<int> data, state;
};

// one workgroup of k_iir_tile
template <typename T, int C>
static void sim_tile(std::vector<T>& data, Counts& cnt, size_t n, const IirSec<T>* tab, int S, const std::vector<T>* state_in,
                     const std::vector<double>* carry_in, std::vector<double>* carry_out, std::vector<T>* state_out, unsigned tiles,
                     unsigned grid_tiles, unsigned block)
{
    constexpr int K = IIR_CHUNK * C;
    std::vector<T> lds((size_t)iir_lds_scalars(C), (T)0);
    const size_t row = block / grid_tiles, tile = block % grid_tiles;
    const int points = iir_tile_points(n, tile), scalars = points * C;
    const size_t at = (row * n + tile * (size_t)IIR_TILE) * (size_t)C;
    for (int tid = 0; tid < IIR_THREADS; ++tid)
        for (int k = 0; k < K; ++k) {
            const int g = k * IIR_THREADS + tid;
            lds.at((size_t)iir_lds_slot(g, C)) = g < scalars ? data.at(at + g) : (T)0;
        }
    std::vector<T> x((size_t)IIR_THREADS * K);
    for (int tid = 0; tid < IIR_THREADS; ++tid)
        for (int j = 0; j < K; ++j) x[(size_t)tid * K + j] = lds.at((size_t)iir_lds_chunk(tid, C) + j);
    const int last_lane = iir_last_lane(points), last_step = iir_last_count(points) - 1;
    std::vector<T> v((size_t)IIR_THREADS * C * 2), prev, s0((size_t)C * 2), ex((size_t)IIR_THREADS * C * 2);
    for (int sec = 0; sec < S; ++sec) {
        const IirSec<T> cf = tab[sec];
        for (int c = 0; c < C; ++c)
            for (int i = 0; i < 2; ++i) {
                T s = (T)0;
                if (carry_in) s = (T)carry_in->at(iir_carry_index(row, tiles, tile, C, c, S, 2 * sec + i));
                else if (state_in) s = state_in->at(iir_state_index(row, C, c, S, 2 * sec + i));
                s0[c * 2 + i] = s;
            }
        for (int tid = 0; tid < IIR_THREADS; ++tid)
            for (int c = 0; c < C; ++c) {
                T s1 = tid == 0 ? s0[c * 2] : (T)0, s2 = tid == 0 ? s0[c * 2 + 1] : (T)0;
                for (int j = 0; j < IIR_CHUNK && tid <= last_lane; ++j) (void)iir_step<T>(cf, x[(size_t)tid * K + j * C + c], &s1, &s2);
                v[((size_t)tid * C + c) * 2] = s1;
                v[((size_t)tid * C + c) * 2 + 1] = s2;
            }
        for (int k = 0; k < IIR_IN_WAVE_STEPS; ++k) {
            prev = v;
            for (int tid = 0; tid < IIR_THREADS; ++tid) {
                const int lane = tid % IIR_WAVE, from = lane >= (1 << k) ? tid - (1 << k) : tid; // __shfl_up
                for (int c = 0; c < C; ++c)
                    iir_scan_step<T>(cf, k, lane, prev[((size_t)from * C + c) * 2], prev[((size_t)from * C + c) * 2 + 1],
                                     &v[((size_t)tid * C + c) * 2], &v[((size_t)tid * C + c) * 2 + 1]);
            }
        }
        for (int tid = 0; tid < IIR_THREADS; ++tid) {
            const int lane = tid % IIR_WAVE, wave = tid / IIR_WAVE, from = lane >= 1 ? tid - 1 : tid;
            for (int c = 0; c < C; ++c)
                for (int i = 0; i < 2; ++i) {
                    ex[((size_t)tid * C + c) * 2 + i] = v[((size_t)from * C + c) * 2 + i];
                    if (lane == IIR_WAVE - 1) lds.at((size_t)iir_lds_total(sec, wave, C, c, i)) = v[((size_t)tid * C + c) * 2 + i];
                }
        }
        for (int tid = 0; tid < IIR_THREADS; ++tid) {
            const int lane = tid % IIR_WAVE, wave = tid / IIR_WAVE;
            for (int c = 0; c < C; ++c) {
                T in1 = (T)0, in2 = (T)0, s1, s2, f1 = (T)0, f2 = (T)0;
                if (wave > 0) iir_wave_in<T>(cf, &lds.at((size_t)iir_lds_total(sec, 0, C, c, 0)), 2 * C, wave, &in1, &in2);
                iir_lane_in<T>(cf, wave, lane, ex[((size_t)tid * C + c) * 2], ex[((size_t)tid * C + c) * 2 + 1], in1, in2, s0[c * 2],
                               s0[c * 2 + 1], &s1, &s2);
                for (int j = 0; j < IIR_CHUNK && tid <= last_lane; ++j) { // (lanes past the row's end skip both runs)
                    T& xx = x[(size_t)tid * K + j * C + c];
                    xx = iir_step<T>(cf, xx, &s1, &s2);
                    if (j == last_step) { f1 = s1; f2 = s2; }
                }
                if (tid != last_lane) continue;
                if (carry_out) {
                    carry_out->at(iir_carry_index(row, tiles, tile, C, c, S, 2 * sec)) = (double)f1;
                    carry_out->at(iir_carry_index(row, tiles, tile, C, c, S, 2 * sec + 1)) = (double)f2;
                } else if (state_out && tile + 1 == tiles) {
                    for (int i = 0; i < 2; ++i) {
                        const size_t at_s = iir_state_index(row, C, c, S, 2 * sec + i);
                        state_out->at(at_s) = i ? f2 : f1;
                        ++cnt.state.at(at_s);
                    }
                }
            }
        }
    }
    if (carry_out) return;
    for (int tid = 0; tid < IIR_THREADS; ++tid)
        for (int j = 0; j < K; ++j) lds.at((size_t)iir_lds_chunk(tid, C) + j) = x[(size_t)tid * K + j];
    for (int tid = 0; tid < IIR_THREADS; ++tid)
        for (int k = 0; k < K; ++k) {
            const int g = k * IIR_THREADS + tid;
            if (g < scalars) { data.at(at + g) = lds.at((size_t)iir_lds_slot(g, C)); ++cnt.data.at(at + g); }
        }
}

// one workgroup of k_iir_carry
template <typename T>
static void sim_carry(std::vector<double>& buf, const std::vector<T>* state_in, const std::vector<double>& m, int S, int C, unsigned tiles,
                      unsigned block)
{
    const int n2 = 2 * S, c = (int)(block % (unsigned)C);
    const size_t row = block / (unsigned)C;
    std::vector<double> mt((size_t)n2 * n2), s(n2), sl(n2), next(n2);
    for (int e = 0; e < n2 * n2; ++e) mt[(size_t)(e % n2) * n2 + e / n2] = m[e];
    for (int i = 0; i < n2; ++i) s[i] = state_in ? (double)state_in->at(iir_state_index(row, C, c, S, i)) : 0.0;
    for (unsigned t = 0; t < tiles; ++t) {
        for (int i = 0; i < n2; ++i) {
            const size_t at = iir_carry_index(row, tiles, t, C, c, S, i);
            const double v = t + 1 < tiles ? buf.at(at) : 0.0;
            buf.at(at) = s[i];
            sl[i] = s[i];
            next[i] = v;
        }
        for (int i = 0; i < n2; ++i) next[i] = iir_carry_dot(mt.data(), sl.data(), n2, i, next[i]);
        s = next;
    }
}

// iir_run: the launches in order; returns their number
template <typename T, int C>
static int sim_run(std::vector<T>& data, Counts& cnt, size_t rows, size_t n, const std::vector<IirSec<T>>& tab, const std::vector<double>& m,
                   std::vector<T>* state)
{
    const int S = (int)tab.size();
    const unsigned tiles = (unsigned)iir_tiles(n);
    if (iir_launches(n) == 1) {
        for (unsigned b = 0; b < rows; ++b) sim_tile<T, C>(data, cnt, n, tab.data(), S, state, nullptr, nullptr, state, 1u, 1u, b);
        return 1;
    }
    std::vector<double> carry(rows * tiles * C * 2 * S, NAN);
    for (unsigned b = 0; b < rows * (tiles - 1); ++b) sim_tile<T, C>(data, cnt, n, tab.data(), S, nullptr, nullptr, &carry, nullptr, tiles, tiles - 1, b);
    for (unsigned b = 0; b < rows * C; ++b) sim_carry<T>(carry, state, m, S, C, tiles, b);
    for (unsigned b = 0; b < rows * tiles; ++b) sim_tile<T, C>(data, cnt, n, tab.data(), S, nullptr, &carry, nullptr, state, tiles, tiles, b);
    return 3;
}

// the serial recurrence on one real signal in precision R, every operation rounded on its own
template <typename R, typename T>
static void serial(const std::vector<IirSec<T>>& tab, const T* x, size_t n, size_t stride, std::vector<R>& y, std::vector<R>& st)
{
    y.resize(n);
    for (size_t i = 0; i < n; ++i) y[i] = (R)x[i * stride];
    for (size_t k = 0; k < tab.size(); ++k) {
        const R b0 = (R)tab[k].b0, b1 = (R)tab[k].b1, b2 = (R)tab[k].b2, a1 = -(R)tab[k].na1, a2 = -(R)tab[k].na2;
        volatile R s1 = st[2 * k], s2 = st[2 * k + 1], t, u;
        for (size_t i = 0; i < n; ++i) {
            const R xi = y[i];
            t = b0 * xi;
            const R yi = t + s1;
            t = b1 * xi; u = a1 * yi; t = t - u; s1 = t + s2;
            t = b2 * xi; u = a2 * yi; s2 = t - u;
            y[i] = yi;
        }
        st[2 * k] = s1;
        st[2 * k + 1] = s2;
    }
}

static double g_worst[2] = {0, 0}, g_worst_state[2] = {0, 0};

template <typename T, int C>
static void run_line(size_t rows, size_t n, int S, const std::string& family, bool with_state)
{
    const std::vector<double> sos = make_sos(family, S);
    CHECK(iir_sos_valid(sos.data(), S), "sos");
    std::vector<IirSec<T>> tab(S);
    std::vector<double> m((size_t)4 * S * S);
    iir_make_tables<T>(sos.data(), S, tab.data(), m.data());
    std::vector<T> data(rows * n * C), x0, state, state0;
    for (auto& d : data) d = (T)uniform();
    x0 = data;
    if (with_state) {
        state.resize(rows * 2 * S * C);
        for (auto& d : state) d = (T)(0.5 * uniform());
        state0 = state;
    }
    Counts cnt;
    cnt.data.assign(data.size(), 0);
    cnt.state.assign(state.size(), 0);
    const int launches = n && S ? sim_run<T, C>(data, cnt, rows, n, tab, m, with_state ? &state : nullptr) : 0;
    CHECK(launches == (S ? iir_launches(n) : 0), "launches %d", launches);
    if (!n || !S) return;
    for (int w : cnt.data) CHECK(w == 1, "an output written %d times", w);
    for (int w : cnt.state) CHECK(w == 1, "a state scalar written %d times", w);
    const double eps = sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16; // 2^-23 / 2^-52, as numpy.finfo
    for (size_t r = 0; r < rows; ++r)
        for (int c = 0; c < C; ++c) {
            std::vector<long double> truth, tst(2 * S, 0.0L);
            std::vector<T> ser, sst(2 * S, (T)0);
            for (int i = 0; i < 2 * S && with_state; ++i) {
                sst[i] = state0[iir_state_index(r, C, c, S, i)];
                tst[i] = (long double)sst[i];
            }
            serial<long double, T>(tab, &x0[r * n * C + c], n, C, truth, tst);
            serial<T, T>(tab, &x0[r * n * C + c], n, C, ser, sst);
            long double e_ser = 0, e_dev = 0, mag = 0, s_ser = 0, s_dev = 0, s_mag = 0;
            for (size_t i = 0; i < n; ++i) {
                e_ser = std::max(e_ser, fabsl((long double)ser[i] - truth[i]));
                e_dev = std::max(e_dev, fabsl((long double)data[(r * n + i) * C + c] - truth[i]));
                mag = std::max(mag, fabsl(truth[i]));
            }
            const double ratio = (double)(e_dev / std::max(e_ser, (long double)eps * mag + 1e-300L));
            g_worst[sizeof(T) == 8] = std::max(g_worst[sizeof(T) == 8], ratio);
            CHECK(ratio <= 16.0, "%s n %zu S %d: e_dev / yardstick %.3f", family.c_str(), n, S, ratio);
            if (!with_state) continue;
            for (int i = 0; i < 2 * S; ++i) {
                s_ser = std::max(s_ser, fabsl((long double)sst[i] - tst[i]));
                s_dev = std::max(s_dev, fabsl((long double)state[iir_state_index(r, C, c, S, i)] - tst[i]));
                s_mag = std::max(s_mag, fabsl(tst[i]));
            }
            const double sr = (double)(s_dev / std::max(s_ser, (long double)eps * s_mag + 1e-300L));
            g_worst_state[sizeof(T) == 8] = std::max(g_worst_state[sizeof(T) == 8], sr);
            CHECK(sr <= 16.0, "%s n %zu S %d: state error / yardstick %.3f", family.c_str(), n, S, sr);
        }
    // the integrator alone on ones counts 1, 2, 3, ... exactly
    if (family == "integrator" && S == 1 && !with_state) {
        std::vector<T> ones(n * C, (T)1);
        Counts c2;
        c2.data.assign(ones.size(), 0);
        sim_run<T, C>(ones, c2, 1, n, tab, m, nullptr);
        for (size_t i = 0; i < n * C; ++i) CHECK(ones[i] == (T)(i / C + 1), "integrator at %zu", i);
    }
}

// extra cycles of one access of `lanes` lanes at element addresses addr[], `dwords` per element, `banks` banks, groups of
// `group` contiguous lanes
static int extra_cycles(const std::vector<int>& addr, int dwords, int banks, int group)
{
    int extra = 0;
    for (size_t g0 = 0; g0 < addr.size(); g0 += group) {
        std::vector<int> use(banks, 0);
        int worst = 1;
        for (int l = 0; l < group; ++l)
            for (int d = 0; d < dwords; ++d) worst = std::max(worst, ++use[(addr[g0 + l] * dwords + d) % banks]);
        extra += worst - 1;
    }
    return extra;
}

static void check_lds()
{
    for (int C = 1; C <= 2; ++C) {
        const int K = IIR_CHUNK * C;
        std::vector<int> seen((size_t)iir_lds_map_scalars(C), 0);
        for (int g = 0; g < IIR_TILE * C; ++g) {
            const int a = iir_lds_slot(g, C);
            CHECK(a >= 0 && a < iir_lds_map_scalars(C), "slot out of the map");
            if (a >= 0 && a < iir_lds_map_scalars(C)) ++seen[a];
            CHECK(a == iir_lds_chunk(g / K, C) + g % K, "the two sides of the map disagree");
        }
        for (int s : seen) CHECK(s <= 1, "two scalars on one slot");
        CHECK(iir_lds_total(1, IIR_WAVES - 1, C, C - 1, 1) == iir_lds_scalars(C) - 1 && iir_lds_total(0, 0, C, 0, 0) == iir_lds_map_scalars(C),
              "the wave totals");
        int chunk32 = 0, chunk64r = 0, chunk64w = 0, row32 = 0, row64r = 0, row64w = 0, accesses = 0;
        for (int w = 0; w < IIR_WAVES; ++w) {
            for (int j = 0; j < K; ++j) { // chunk side: one wave, scalar j of every lane's chunk
                std::vector<int> addr;
                for (int l = 0; l < IIR_WAVE; ++l) addr.push_back(iir_lds_chunk(w * IIR_WAVE + l, C) + j);
                chunk32 += extra_cycles(addr, 1, 32, 32);
                chunk64r += extra_cycles(addr, 2, 64, 32);
                chunk64w += extra_cycles(addr, 2, 32, 16);
            }
            for (int k = 0; k < K; ++k) { // row side
                std::vector<int> addr;
                for (int l = 0; l < IIR_WAVE; ++l) addr.push_back(iir_lds_slot(k * IIR_THREADS + w * IIR_WAVE + l, C));
                row32 += extra_cycles(addr, 1, 32, 32);
                row64r += extra_cycles(addr, 2, 64, 32);
                row64w += extra_cycles(addr, 2, 32, 16);
                accesses += 1;
            }
        }
        printf("LDS %s: chunk side f32 %d, f64 read %d, f64 write %d extra bank cycles; row side (%d accesses) f32 %d, f64 read %d, f64 write %d\n",
               C == 1 ? "real" : "complex", chunk32, chunk64r, chunk64w, accesses, row32, row64r, row64w);
        CHECK(chunk32 == 0 && chunk64r == 0 && chunk64w == 0, "the chunk side is not conflict-free");
        const int per_group = C == 1 ? 2 * accesses : 0; // one extra cycle per 32-lane group of a real tile
        CHECK(row32 == per_group && row64r == per_group && row64w == 0, "the row side's cycles are not the claimed ones");
    }
}

// runs of chunks [lo, hi]: a step may only join adjacent runs, with the table whose power is the later run's length
struct Run { int lo, hi; };
static void check_tree()
{
    std::vector<Run> v(IIR_THREADS), prev;
    for (int t = 0; t < IIR_THREADS; ++t) v[t] = {t, t};
    for (int k = 0; k < IIR_IN_WAVE_STEPS; ++k) {
        prev = v;
        for (int t = 0; t < IIR_THREADS; ++t) {
            const int lane = t % IIR_WAVE;
            if (!iir_scan_takes(lane, k)) continue;
            const Run f = prev[t - (1 << k)];
            CHECK(f.hi + 1 == v[t].lo && v[t].hi - v[t].lo + 1 == (1 << k), "step %d lane %d joins the wrong runs", k, t);
            v[t].lo = f.lo;
        }
    }
    for (int t = 0; t < IIR_THREADS; ++t) CHECK(v[t].lo == t / IIR_WAVE * IIR_WAVE && v[t].hi == t, "lane %d after the tree", t);
    for (int q = 1; q < IIR_WAVES; ++q) { // the Horner chain: P_6 advances by one wave
        Run a = v[IIR_WAVE - 1];
        for (int p = 1; p < q; ++p) { CHECK(a.hi + 1 == v[p * IIR_WAVE + IIR_WAVE - 1].lo, "wave chain"); a.hi = v[p * IIR_WAVE + IIR_WAVE - 1].hi; }
        CHECK(a.lo == 0 && a.hi == q * IIR_WAVE - 1 && (1 << (IIR_POWERS - 1)) == IIR_WAVE, "wave %d's incoming state", q);
        for (int j = 0; j < IIR_WAVE; ++j) { // iir_advance: the set bits of j sum to the chunks before lane j in its wave
            int adv = 0;
            for (int k = 0; k < IIR_IN_WAVE_STEPS; ++k) if ((j >> k) & 1) adv += 1 << k;
            CHECK(adv == j, "advance");
        }
    }
    // the tables are the powers they are named after: P_k against 16 * 2^k homogeneous steps in long double
    const std::vector<double> sos = make_sos("resonator", 2);
    std::vector<IirSec<double>> tab(2);
    iir_make_tables<double>(sos.data(), 2, tab.data(), nullptr);
    for (int sec = 0; sec < 2; ++sec)
        for (int k = 0; k < IIR_POWERS; ++k)
            for (int col = 0; col < 2; ++col) {
                long double s1 = col == 0, s2 = col == 1;
                for (int i = 0; i < IIR_CHUNK << k; ++i) {
                    const long double y = s1;
                    s1 = (long double)tab[sec].na1 * y + s2;
                    s2 = (long double)tab[sec].na2 * y;
                }
                CHECK(fabsl(s1 - tab[sec].p[k][col]) < 1e-12 && fabsl(s2 - tab[sec].p[k][2 + col]) < 1e-12, "P_%d of section %d", k, sec);
            }
    // M against IIR_TILE steps of the cascade from a unit state, through the serial model
    std::vector<double> m(16);
    iir_make_tables<double>(sos.data(), 2, tab.data(), m.data());
    for (int col = 0; col < 4; ++col) {
        std::vector<long double> st(4, 0.0L), y;
        st[col] = 1.0L;
        std::vector<double> zero(IIR_TILE, 0.0);
        serial<long double, double>(tab, zero.data(), IIR_TILE, 1, y, st);
        for (int i = 0; i < 4; ++i) CHECK(fabsl(st[i] - m[i * 4 + col]) < 1e-12, "M[%d][%d]", i, col);
    }
}

static void check_plan()
{
    CHECK(iir_launches(0) == 0 && iir_launches(1) == 1 && iir_launches(IIR_TILE) == 1 && iir_launches(IIR_TILE + 1) == 3, "launches");
    CHECK(iir_tiles(IIR_TILE) == 1 && iir_tiles(IIR_TILE + 1) == 2 && iir_tiles(2 * IIR_TILE + 17) == 3, "tiles");
    CHECK(iir_tile_points(2 * IIR_TILE + 17, 2) == 17 && iir_tile_points(2 * IIR_TILE + 17, 1) == IIR_TILE, "tile points");
    CHECK(iir_last_lane(17) == 1 && iir_last_count(17) == 1 && iir_last_lane(16) == 0 && iir_last_count(16) == 16, "last lane");
    CHECK(iir_last_lane(IIR_TILE) == IIR_THREADS - 1 && iir_last_count(IIR_TILE) == IIR_CHUNK && iir_last_lane(1) == 0 && iir_last_count(1) == 1, "last lane");
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: sim_iir tests/iir_shapes.txt\n"); return 2; }
    check_plan();
    check_lds();
    check_tree();
    std::ifstream f(argv[1]);
    std::string line;
    int lines = 0;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line);
        std::string kind, prec, family;
        size_t rows, n;
        int S;
        if (!(is >> kind >> prec >> rows >> n >> S >> family)) { CHECK(false, "bad line: %s", line.c_str()); continue; }
        CHECK(S >= 1 && S <= IIR_MAX_SECTIONS, "sections");
        ++lines;
        for (int with_state = 0; with_state < 2; ++with_state) {
            if (kind == "real" && prec == "f32") run_line<float, 1>(rows, n, S, family, with_state);
            else if (kind == "complex" && prec == "f32") run_line<float, 2>(rows, n, S, family, with_state);
            else if (kind == "real" && prec == "f64") run_line<double, 1>(rows, n, S, family, with_state);
            else if (kind == "complex" && prec == "f64") run_line<double, 2>(rows, n, S, family, with_state);
            else CHECK(false, "bad line: %s", line.c_str());
        }
    }
    printf("worst e_dev / max(e_ser, eps max|truth|): f32 %.3f, f64 %.3f\n", g_worst[0], g_worst[1]);
    printf("worst final-state ratio: f32 %.3f, f64 %.3f\n", g_worst_state[0], g_worst_state[1]);
    printf("%d shape lines (each with and without an incoming state), %d failures\n", lines, g_fail);
    printf(g_fail ? "FAILED\n" : "ok\n");
    return g_fail ? 1 : 0;
}
