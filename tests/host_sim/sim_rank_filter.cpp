// Host simulation of rank_filter.hip: the functions of basic_dsp_amd/csrc/rank_filter_core.h with threads as loops, on
// every line of tests/rank_filter_shapes.txt (rows n half rank guard boundary) and both key widths.  A stand-alone
// program: g++ -O2 -std=c++17 [-fsanitize=address,undefined] sim_rank_filter.cpp && ./a.out tests/rank_filter_shapes.txt
//
// Per line and key width it checks
//   - every output index of every row is written exactly once;
//   - every LDS slot that is written or read lies inside the allocation of rank_lds_keys(half) keys, and every slot that
//     is read was written before the barrier;
//   - the boundary index function agrees with a brute-force definition (walking position by position from the row);
//   - BOTH selectors equal std::sort on the keys of every window of the line, the window gathered from the row by the
//     definition (guard < |d| <= half), on data with many ties and edge patterns;
//   - for the lines where the kernel takes the count selector: all lanes of a wave make the same number of LDS reads, and
//     at every step the 32-lane halves read consecutive slots with no extra bank cycle (ds_read_b32: bank (a / 4) % 32,
//     ds_read_b64: bank (a / 4) % 64).
// Once: the key map is a strictly monotone bijection on the edge patterns (+-0, +-denormals, +-inf, +-NaN with payloads)
// and agrees with < on random finite values.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../basic_dsp_amd/csrc/rank_filter_core.h"

using namespace bdsp;

static int g_failures = 0;
#define CHECK(cond, ...)                                                                                                \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            if (g_failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++g_failures;                                                                                               \
        }                                                                                                               \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}

template <typename K> struct Fmt;
template <> struct Fmt<uint32_t> { using F = float; static constexpr int E = 8, M = 23; static const char* name() { return "f32"; } };
template <> struct Fmt<uint64_t> { using F = double; static constexpr int E = 11, M = 52; static const char* name() { return "f64"; } };

template <typename K> K pattern(int sign, uint64_t exp, uint64_t mant)
{
    return (K)(((K)sign << (Fmt<K>::E + Fmt<K>::M)) | ((K)exp << Fmt<K>::M) | (K)mant);
}

// the edge patterns in ascending totalOrder
template <typename K> std::vector<K> edge_patterns()
{
    const uint64_t emax = (1ull << Fmt<K>::E) - 1, mmax = (1ull << Fmt<K>::M) - 1, quiet = 1ull << (Fmt<K>::M - 1), bias = emax >> 1;
    std::vector<K> up = {pattern<K>(0, 0, 0), pattern<K>(0, 0, 1), pattern<K>(0, 0, mmax), pattern<K>(0, 1, 0), pattern<K>(0, bias, 0),
                         pattern<K>(0, emax - 1, mmax), pattern<K>(0, emax, 0), pattern<K>(0, emax, 1), pattern<K>(0, emax, quiet),
                         pattern<K>(0, emax, quiet + 5), pattern<K>(0, emax, mmax)};
    std::vector<K> all;
    for (size_t i = up.size(); i-- > 0;) all.push_back(up[i] | pattern<K>(1, 0, 0)); // the negatives, from -NaN up to -0
    all.insert(all.end(), up.begin(), up.end());
    return all;
}

template <typename K> void check_key_map()
{
    using F = typename Fmt<K>::F;
    const std::vector<K> e = edge_patterns<K>();
    for (size_t i = 0; i < e.size(); ++i) {
        CHECK(rank_bits<K>(rank_key<K>(e[i])) == e[i], "%s key map is no bijection at edge %zu", Fmt<K>::name(), i);
        if (i) CHECK(rank_key<K>(e[i - 1]) < rank_key<K>(e[i]), "%s key map not strictly monotone at edge %zu", Fmt<K>::name(), i);
    }
    CHECK(rank_key<K>(0) == (K)1 << (8 * sizeof(K) - 1), "key of +0.0");
    for (int t = 0; t < 200000; ++t) {
        const K a = (K)rnd(), b = (K)rnd();
        CHECK(rank_bits<K>(rank_key<K>(a)) == a && rank_key<K>(rank_bits<K>(a)) == a, "%s key map is no bijection", Fmt<K>::name());
        F fa, fb;
        std::memcpy(&fa, &a, sizeof(K));
        std::memcpy(&fb, &b, sizeof(K));
        if (std::isfinite(fa) && std::isfinite(fb) && fa != fb)
            CHECK((fa < fb) == (rank_key<K>(a) < rank_key<K>(b)), "%s key order disagrees with < on finite values", Fmt<K>::name());
    }
}

// position q of a row by the definition, walking one position at a time: the row index, or -1 for +0.0
static int64_t brute_index(int64_t q, int64_t n, int boundary)
{
    if (boundary == RANK_ZERO) return q >= 0 && q < n ? q : -1;
    if (boundary == RANK_NEAREST) { while (q < 0) ++q; while (q >= n) --q; return q; }
    while (q < 0) q += n;
    while (q >= n) q -= n;
    return q;
}

struct Shape {
    size_t rows, n;
    int half, rank, guard, boundary;
    std::string text;
};

// the kernel's LDS through a view that checks every access
template <typename K> struct CheckedLds {
    const std::vector<K>* keys;
    const std::vector<unsigned char>* written;
    std::vector<int>* trace; // may be null
    mutable long reads = 0;
    mutable bool bad = false;
    K operator[](int slot) const
    {
        ++reads;
        if (slot < 0 || (size_t)slot >= keys->size() || !(*written)[(size_t)slot]) { bad = true; return 0; }
        if (trace) trace->push_back(slot);
        return (*keys)[(size_t)slot];
    }
};

// extra LDS cycles of one 32-lane group reading the given slots of key_bytes each
static int extra_cycles(const std::vector<int>& slots, int key_bytes)
{
    const int banks = key_bytes == 4 ? 32 : 64, dwords = key_bytes / 4;
    std::vector<std::vector<int>> at((size_t)banks);
    for (int s : slots)
        for (int d = 0; d < dwords; ++d) {
            std::vector<int>& v = at[(size_t)((s * dwords + d) % banks)];
            if (std::find(v.begin(), v.end(), s * dwords + d) == v.end()) v.push_back(s * dwords + d); // identical addresses broadcast
        }
    int worst = 1;
    for (const auto& v : at) worst = std::max(worst, (int)v.size());
    return worst - 1;
}

static long g_bank_steps[2] = {0, 0}, g_bank_extra[2] = {0, 0};

template <typename K> void run_shape(const Shape& sh, int width_index)
{
    const int64_t n = (int64_t)sh.n;
    const size_t W = rank_window_size((size_t)sh.half, sh.guard);
    CHECK(rank_args_valid((size_t)sh.half, (size_t)sh.rank, sh.guard, sh.boundary) && sh.half <= RANK_MAX_HALF, "%s: invalid line", sh.text.c_str());
    const RankWindow w = rank_window(sh.half, sh.guard);
    CHECK((size_t)(w.len_a + w.len_b) == W, "%s: the segments hold %d keys, W = %zu", sh.text.c_str(), w.len_a + w.len_b, W);
    const bool takes_count = rank_uses_count(W, (int)sizeof(K));

    // 16 levels and a sprinkle of edge patterns: many ties
    const std::vector<K> edges = edge_patterns<K>();
    std::vector<K> levels;
    for (int l = 0; l < 16; ++l) {
        typename Fmt<K>::F f = (typename Fmt<K>::F)(0.5 * (l - 8));
        K b;
        std::memcpy(&b, &f, sizeof(K));
        levels.push_back(b);
    }
    std::vector<K> data(sh.rows * sh.n), out(sh.rows * sh.n, 0);
    for (K& v : data) v = rnd() % 8 == 0 ? edges[rnd() % edges.size()] : levels[rnd() % 16];
    std::vector<int> count(sh.rows * sh.n, 0);

    const size_t tiles = rank_tiles(sh.n);
    const size_t alloc = (size_t)rank_lds_keys(sh.half);
    for (size_t block = 0; block < sh.rows * tiles; ++block) {
        const size_t row = block / tiles, tile = block % tiles;
        const int points = rank_tile_points(sh.n, tile), loaded = rank_loaded(points, sh.half);
        CHECK(points > 0 && points <= RANK_TILE && (size_t)loaded <= alloc, "%s: tile %zu has %d points, loads %d of %zu", sh.text.c_str(), tile, points, loaded, alloc);
        const K* src = data.data() + row * sh.n;
        const int64_t first = rank_first_position(tile, sh.half);
        std::vector<K> lds(alloc, 0);
        std::vector<unsigned char> written(alloc, 0);
        for (int tid = 0; tid < RANK_THREADS; ++tid)
            for (int p = tid; p < loaded; p += RANK_THREADS) {
                const int64_t g = rank_src_index(first + p, n, sh.boundary);
                CHECK(g == brute_index(first + p, n, sh.boundary), "%s: position %lld reads %lld", sh.text.c_str(), (long long)(first + p), (long long)g);
                CHECK(g >= -1 && g < n, "%s: source index %lld outside the row", sh.text.c_str(), (long long)g);
                if ((size_t)p >= alloc) { CHECK(false, "%s: LDS slot %d outside the allocation", sh.text.c_str(), p); continue; }
                CHECK(!written[(size_t)p], "%s: LDS slot %d written twice", sh.text.c_str(), p);
                written[(size_t)p] = 1;
                lds[(size_t)p] = rank_key<K>(g < 0 || g >= n ? (K)0 : src[g]);
            }
        // ---- barrier ----
        const bool trace_this = takes_count && block == 0;
        std::vector<std::vector<int>> traces(trace_this ? (size_t)RANK_TILE : 0);
        std::vector<K> win;
        for (int tid = 0; tid < RANK_THREADS; ++tid)
            for (int k = 0; k < RANK_PER_LANE; ++k) {
                const int o = rank_out_index(tid, k);
                if (o >= points) continue;
                CheckedLds<K> view{&lds, &written, trace_this ? &traces[(size_t)o] : nullptr};
                const K by_count = rank_select_count<K>(view, o, w, sh.rank);
                CHECK(view.reads == (long)(W + W * W), "%s: the count selector made %ld reads, W = %zu", sh.text.c_str(), view.reads, W);
                view.trace = nullptr;
                view.reads = 0;
                const K by_bisect = rank_select_bisect<K>(view, o, w, sh.rank);
                CHECK(view.reads == (long)(8 * sizeof(K) * W), "%s: the bisect selector made %ld reads", sh.text.c_str(), view.reads);
                CHECK(!view.bad, "%s: output %d of tile %zu reads an LDS slot outside the allocation or never written", sh.text.c_str(), o, tile);
                // the window by the definition, from the row
                const int64_t i = (int64_t)(tile * RANK_TILE) + o;
                win.clear();
                for (int64_t d = -sh.half; d <= sh.half; ++d) {
                    if (sh.guard >= 0 && std::llabs(d) <= sh.guard) continue;
                    const int64_t g = brute_index(i + d, n, sh.boundary);
                    win.push_back(rank_key<K>(g < 0 ? (K)0 : src[g]));
                }
                std::sort(win.begin(), win.end());
                CHECK(win.size() == W, "%s: window of %zu keys, W = %zu", sh.text.c_str(), win.size(), W);
                const K want = win[(size_t)sh.rank];
                CHECK(by_count == want, "%s %s: count selector wrong at row %zu point %lld", sh.text.c_str(), Fmt<K>::name(), row, (long long)i);
                CHECK(by_bisect == want, "%s %s: bisect selector wrong at row %zu point %lld", sh.text.c_str(), Fmt<K>::name(), row, (long long)i);
                const size_t at = row * sh.n + (size_t)i;
                CHECK(at < out.size(), "%s: output index %zu outside the matrix", sh.text.c_str(), at);
                if (at < out.size()) { out[at] = rank_bits<K>(takes_count ? by_count : by_bisect); ++count[at]; }
            }
        if (trace_this) {
            // a wave = 64 consecutive tid with the same k; its 32-lane halves step through the selector together
            for (int k = 0; k < RANK_PER_LANE; ++k)
                for (int half_wave = 0; half_wave < RANK_THREADS / 32; ++half_wave) {
                    std::vector<int> lanes;
                    for (int l = 0; l < 32; ++l)
                        if (rank_out_index(half_wave * 32 + l, k) < points) lanes.push_back(rank_out_index(half_wave * 32 + l, k));
                    if (lanes.empty()) continue;
                    const size_t steps = traces[(size_t)lanes[0]].size();
                    for (int o : lanes) CHECK(traces[(size_t)o].size() == steps, "%s: lanes of one wave differ in their read counts", sh.text.c_str());
                    std::vector<int> slots(lanes.size());
                    for (size_t s = 0; s < steps; ++s) {
                        for (size_t l = 0; l < lanes.size(); ++l) slots[l] = traces[(size_t)lanes[l]][s];
                        for (size_t l = 1; l < lanes.size(); ++l)
                            CHECK(slots[l] == slots[l - 1] + 1, "%s: consecutive lanes do not read consecutive slots", sh.text.c_str());
                        g_bank_extra[width_index] += extra_cycles(slots, (int)sizeof(K));
                        ++g_bank_steps[width_index];
                    }
                }
        }
    }
    for (size_t at = 0; at < count.size(); ++at) CHECK(count[at] == 1, "%s: output %zu written %d times", sh.text.c_str(), at, count[at]);
    // the stored bits are bits of the row's own values or +0.0
    for (size_t row = 0; row < sh.rows; ++row)
        for (size_t i = 0; i < sh.n; ++i) {
            const K v = out[row * sh.n + i];
            bool found = v == 0 && sh.boundary == RANK_ZERO;
            for (size_t j = 0; j < sh.n && !found; ++j) found = data[row * sh.n + j] == v;
            CHECK(found, "%s: output %zu of row %zu is no input value", sh.text.c_str(), i, row);
        }
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: %s tests/rank_filter_shapes.txt\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
    check_key_map<uint32_t>();
    check_key_map<uint64_t>();
    std::printf("key map: strictly monotone bijection on %zu edge patterns per width\n", edge_patterns<uint32_t>().size());
    // the argument rule
    CHECK(!rank_args_valid(1, 3, -1, RANK_ZERO) && rank_args_valid(1, 2, -1, RANK_ZERO), "rank >= W");
    CHECK(!rank_args_valid(4, 0, 4, RANK_WRAP) && rank_args_valid(4, 1, 3, RANK_WRAP) && !rank_args_valid(4, 2, 3, RANK_WRAP), "guard >= half");
    CHECK(!rank_args_valid(1, 0, -1, 3) && !rank_args_valid(1, 0, -1, -1) && !rank_args_valid(1, 0, -2, 0), "unknown boundary / guard");
    CHECK(!rank_args_valid(0, 0, 0, 0) && rank_args_valid(0, 0, -1, 0) && rank_args_valid(SIZE_MAX, SIZE_MAX - 1, -1, 0), "extremes");
    CHECK(rank_uses_count((size_t)RANK_CROSS_F32, 4) && !rank_uses_count((size_t)RANK_CROSS_F32 + 1, 4), "f32 crossover");
    CHECK(rank_uses_count((size_t)RANK_CROSS_F64, 8) && !rank_uses_count((size_t)RANK_CROSS_F64 + 1, 8), "f64 crossover");
    std::string line;
    int lines = 0;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line);
        Shape sh;
        std::string guard, boundary;
        is >> sh.rows >> sh.n >> sh.half >> sh.rank >> guard >> boundary;
        if (!is) { std::printf("FAIL: cannot parse '%s'\n", line.c_str()); ++g_failures; continue; }
        sh.guard = guard == "none" ? -1 : std::stoi(guard);
        sh.boundary = boundary == "zero" ? RANK_ZERO : boundary == "wrap" ? RANK_WRAP : boundary == "nearest" ? RANK_NEAREST : -1;
        sh.text = line;
        const int before = g_failures;
        run_shape<uint32_t>(sh, 0);
        run_shape<uint64_t>(sh, 1);
        if (g_failures != before) std::printf("FAIL line: %s\n", line.c_str());
        ++lines;
    }
    std::printf("count selector LDS reads: f32 %ld group steps, %ld extra bank cycles; f64 %ld group steps, %ld extra bank cycles\n",
                g_bank_steps[0], g_bank_extra[0], g_bank_steps[1], g_bank_extra[1]);
    std::printf("%d shape lines (both key widths, both selectors), %d failures\n", lines, g_failures);
    if (g_failures || g_bank_extra[0] || g_bank_extra[1] || !g_bank_steps[0] || !g_bank_steps[1]) { std::printf("FAILED\n"); return 1; }
    std::printf("ok\n");
    return 0;
}
