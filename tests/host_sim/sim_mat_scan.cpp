// Host simulation of k_ms_unwrap (basic_dsp_amd/csrc/mat_scan.hip): the kernel's passes with threads as loops, on the
// index functions of mat_scan_core.h.  Checks, for f32 and f64, every tile shape and every tail:
//   * every element of the matrix goes to exactly one LDS slot of its tile and comes back to its own address, once;
//   * no two lanes of a lane group hit the same LDS bank on distinct addresses, in the walk and in the load / store
//     passes (bank rule per instruction, see lds_conflicts);
//   * the walker over the simulated tiles reproduces the plain recurrence with the library fmod (orc_unwrap of the
//     oracle) bit for bit.
// g++ -O2 -std=c++17 -ffp-contract=off; prints OK.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_scan_core.h"

using namespace bdsp;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                                  \
    do {                                                                                                  \
        if (!(cond)) { if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++g_fail; } \
    } while (0)

// One wave-instruction: byte address per lane (-1 = lane masked off), `bytes` 4 or 8.  Lane groups and bank moduli:
// ds_read_b32 / ds_write_b32: two 32-lane halves, (a / 4) % 32; ds_read_b64: two 32-lane halves, (a / 4) % 64;
// ds_write_b64: four groups of 16 contiguous lanes, (a / 4) % 32.  Identical addresses broadcast.
static int lds_conflicts(const long* addr, int bytes, bool write)
{
    const int group = (bytes == 8 && write) ? 16 : 32;
    const int banks = (bytes == 8 && !write) ? 64 : 32;
    int conflicts = 0;
    for (int g0 = 0; g0 < MS_LANES; g0 += group) {
        long owner[64];
        for (int b = 0; b < 64; ++b) owner[b] = -1;
        for (int l = g0; l < g0 + group; ++l) {
            if (addr[l] < 0) continue;
            for (int d = 0; d < bytes / 4; ++d) {
                const long dw = addr[l] / 4 + d;
                const int b = (int)(dw % banks);
                if (owner[b] >= 0 && owner[b] != dw) ++conflicts;
                owner[b] = dw;
            }
        }
    }
    return conflicts;
}

template <typename T>
static void reference_unwrap(T* x, size_t len, T divisor) // orc_unwrap, real_ops.rs:262-284
{
    const T half = divisor / 2;
    for (size_t i = 0, j = 1; j < len; ++i, ++j) {
        T diff = x[j] - x[i];
        if (diff > half) { diff = std::fmod(diff, divisor); diff = diff - divisor; x[j] = x[i] + diff; }
        else if (diff < -half) { diff = std::fmod(diff, divisor); diff = diff + divisor; x[j] = x[i] + diff; }
    }
}

// the kernel, one workgroup after the other; `walk` false: the tiles pass through untouched (traffic check)
template <typename T>
static void sim_kernel(std::vector<T>& x, size_t rows, size_t row_len, T divisor, int R, bool walk, std::vector<int>* loads,
                       std::vector<int>* stores)
{
    const int W = ms_tile_width(sizeof(T), R), PER = ms_tile_elems(sizeof(T)) / MS_LANES;
    std::vector<T> tile(ms_lds_elems(R, W));
    std::vector<T> pre((size_t)PER * MS_LANES);
    const T half = divisor / T(2), inv = T(1) / std::fabs(divisor);
    const size_t groups = (rows + R - 1) / R;
    for (size_t g = 0; g < groups; ++g) {
        const size_t row0 = g * R;
        if (row0 >= rows || row_len == 0) continue;
        const int rv = rows - row0 < (size_t)R ? (int)(rows - row0) : R;
        const size_t ntiles = (row_len + W - 1) / W;
        std::vector<T> prev(MS_LANES, T(0));
        auto fetch = [&](size_t t) {
            const int m = ms_tile_cols(row_len, t, W);
            for (int k = 0; k < PER; ++k)
                for (int lane = 0; lane < MS_LANES; ++lane) {
                    int r, c;
                    ms_tile_rc(k, lane, W, &r, &c);
                    const bool own = r < rv && c < m;
                    r = r < rv ? r : rv - 1;
                    c = c < m ? c : m - 1;
                    const size_t a = (row0 + r) * row_len + t * W + c;
                    CHECK(a < x.size(), "load out of bounds %zu", a);
                    pre[(size_t)k * MS_LANES + lane] = x[a];
                    if (own && loads) ++(*loads)[a];
                }
        };
        auto to_lds = [&]() {
            std::set<int> slots;
            for (int k = 0; k < PER; ++k) {
                long addr[MS_LANES];
                for (int lane = 0; lane < MS_LANES; ++lane) {
                    int r, c;
                    ms_tile_rc(k, lane, W, &r, &c);
                    CHECK(r >= 0 && r < R && c >= 0 && c < W, "tile position (%d, %d)", r, c);
                    const int slot = ms_lds_slot(r, c, W);
                    CHECK(slot >= 0 && slot < (int)tile.size(), "slot %d", slot);
                    if (!walk) CHECK(slots.insert(slot).second, "slot %d written twice", slot);
                    tile[slot] = pre[(size_t)k * MS_LANES + lane];
                    addr[lane] = (long)slot * (long)sizeof(T);
                }
                if (!walk) CHECK(lds_conflicts(addr, sizeof(T), true) == 0, "bank conflict in the LDS fill, R %d k %d", R, k);
            }
            if (!walk) CHECK((int)slots.size() == R * W, "fill covers %zu of %d slots", slots.size(), R * W);
        };
        fetch(0);
        to_lds();
        for (size_t t = 0; t < ntiles; ++t) {
            const bool more = t + 1 < ntiles;
            if (more) fetch(t + 1);
            const int m = ms_tile_cols(row_len, t, W);
            // lock-step walk: all walking lanes are at the same column
            for (int j = 0; j < m; ++j) {
                if (!walk) { // (the bank checks ride on the traffic pass: they do not depend on the data)
                    long addr[MS_LANES];
                    for (int lane = 0; lane < MS_LANES; ++lane) addr[lane] = lane < rv ? (long)ms_lds_slot(lane, j, W) * (long)sizeof(T) : -1;
                    CHECK(lds_conflicts(addr, sizeof(T), false) == 0, "bank conflict in the walk (read), R %d W %d col %d", R, W, j);
                    CHECK(lds_conflicts(addr, sizeof(T), true) == 0, "bank conflict in the walk (write), R %d W %d col %d", R, W, j);
                    continue;
                }
                for (int lane = 0; lane < rv; ++lane) {
                    T* row = tile.data() + ms_lds_slot(lane, 0, W);
                    if (t == 0 && j == 0) { prev[lane] = row[0]; continue; }
                    prev[lane] = ms_unwrap_step(row[j], prev[lane], half, divisor, inv);
                    row[j] = prev[lane];
                }
            }
            for (int k = 0; k < PER; ++k) {
                long addr[MS_LANES];
                for (int lane = 0; lane < MS_LANES; ++lane) {
                    int r, c;
                    ms_tile_rc(k, lane, W, &r, &c);
                    addr[lane] = (long)ms_lds_slot(r, c, W) * (long)sizeof(T);
                    if (r < rv && c < m) {
                        const size_t a = (row0 + r) * row_len + t * W + c;
                        CHECK(a < x.size(), "store out of bounds %zu", a);
                        x[a] = tile[ms_lds_slot(r, c, W)];
                        if (stores) ++(*stores)[a];
                    }
                }
                if (!walk) CHECK(lds_conflicts(addr, sizeof(T), false) == 0, "bank conflict in the LDS drain, R %d k %d", R, k);
            }
            if (more) to_lds();
        }
    }
}

template <typename T>
static void run_type(const char* name)
{
    std::mt19937_64 rng(12345);
    const size_t row_counts[] = {1, 63, 64, 65, 257};
    const int shapes[] = {64, 16, 4, 1};
    for (int R : shapes) {
        const int W = ms_tile_width(sizeof(T), R);
        CHECK(R * W * (int)sizeof(T) == MS_TILE_BYTES, "tile bytes");
        CHECK(R < 64 || W * sizeof(T) >= 256, "runs shorter than 256 bytes");
        CHECK(ms_lds_stride(W) % 2 == 1, "LDS stride must be odd");
        const size_t lens[] = {0, 1, (size_t)W - 1, (size_t)W, (size_t)W + 1, 3 * (size_t)W + 5};
        for (size_t rows : row_counts)
            for (size_t len : lens) {
                if (R < 64 && rows * len > 600000) continue; // wide tiles: the long rows with few row counts only
                const size_t n = rows * len;
                // traffic: every element read once, written once, to its own address
                std::vector<T> x(n), y;
                for (size_t i = 0; i < n; ++i) x[i] = (T)(i % 16777216);
                y = x;
                std::vector<int> loads(n, 0), stores(n, 0);
                sim_kernel<T>(y, rows, len, T(7), R, false, &loads, &stores);
                bool once = true;
                for (size_t i = 0; i < n; ++i) once = once && loads[i] == 1 && stores[i] == 1;
                CHECK(once, "%s R %d %zu x %zu: an element not moved exactly once", name, R, rows, len);
                CHECK(n == 0 || std::memcmp(x.data(), y.data(), n * sizeof(T)) == 0, "%s R %d %zu x %zu: element came back elsewhere", name, R, rows, len);
                // the walk against the plain recurrence
                struct Case { double lo, hi, div; } cases[] = {{-30, 30, 7}, {-3.14159, 3.14159, 6.283185307179586}, {-1e6, 1e6, 1e-3},
                                                               {-1e6, 1e6, 3}, {-30, 30, -7}, {-100, 100, 0.1}};
                for (const Case& cs : cases) {
                    std::uniform_real_distribution<double> u(cs.lo, cs.hi);
                    for (size_t i = 0; i < n; ++i) x[i] = (T)u(rng);
                    if (cs.div == 3)
                        for (size_t i = 0; i < n; i += 7) x[i] = (T)(std::round((double)x[i] / 3) * 3); // quotients at integers
                    y = x;
                    sim_kernel<T>(y, rows, len, (T)cs.div, R, true, nullptr, nullptr);
                    for (size_t r = 0; r < rows; ++r) reference_unwrap<T>(x.data() + r * len, len, (T)cs.div);
                    CHECK(n == 0 || std::memcmp(x.data(), y.data(), n * sizeof(T)) == 0, "%s R %d %zu x %zu divisor %g: walk differs from the recurrence", name, R,
                          rows, len, cs.div);
                }
            }
    }
    // the tile shape follows the row count: few rows -> few rows per workgroup, never more than 4 workgroups per CU
    // while the matrix has at most 64 rows per CU x 4
    CHECK(ms_rows_per_group(1, 256) == 1 && ms_rows_per_group(1024, 256) == 1 && ms_rows_per_group(1025, 256) == 4, "shape choice");
    CHECK(ms_rows_per_group(16384, 256) == 16 && ms_rows_per_group(16385, 256) == 64 && ms_rows_per_group(1u << 20, 256) == 64, "shape choice");
}

int main()
{
    run_type<float>("f32");
    run_type<double>("f64");
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK\n");
    return 0;
}
