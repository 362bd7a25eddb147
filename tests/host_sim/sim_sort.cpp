// sim_sort.cpp -- the launches of sort.hip on the host, with threads as loops: the same functions of sort_core.h, on checking
// views of LDS and of the buffers.  For every line `rows n` of the shapes file, both key widths, both directions, with and
// without index:
//   every output slot of every launch is written exactly once, nothing else is written;
//   every LDS word is inside the allocation and written before it is read;
//   each merge-path split is unique (the two workgroups that compute a diagonal agree), monotone over the workgroups of a
//   pair, and the pieces sum to the outputs produced;
//   the final keys and indices equal std::stable_sort; pads never reach an output;
//   the LDS bank cycles of every store and load of every change of layout, by the rules of the instructions that move 4- and
//   8-byte words, and the extra cycles among them.
// usage: sim_sort <shapes file>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../basic_dsp_amd/csrc/sort_core.h"

using namespace bdsp;

static long g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_fail < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } \
            ++g_fail;                                      \
        }                                                  \
    } while (0)

template <typename V>
struct LdsView {
    std::vector<V>* mem;
    std::vector<char>* written;
    V get(int i) const
    {
        CHECK(i >= 0 && i < (int)mem->size(), "LDS read outside the allocation: %d", i);
        if (i < 0 || i >= (int)mem->size()) return V();
        CHECK((*written)[i], "LDS word %d read before it was written", i);
        return (*mem)[i];
    }
    void put(int i, V v) const
    {
        CHECK(i >= 0 && i < (int)mem->size(), "LDS write outside the allocation: %d", i);
        if (i < 0 || i >= (int)mem->size()) return;
        (*mem)[i] = v;
        (*written)[i] = 1;
    }
};

template <typename K>
struct RunView { // a run in global memory
    const K* p;
    uint32_t len;
    K operator[](uint32_t i) const
    {
        CHECK(i < len, "split reads element %u of a run of %u", i, len);
        return i < len ? p[i] : K();
    }
};

// ---------------------------------------------------------------- bank cycles
struct Banks {
    long group_steps = 0, extra = 0;
};
static Banks g_banks[2]; // by key width

// one instruction of a wave: words[lane]; lanes per group, banks, bytes tell the rule
static void count_instruction(const int* words, int group_lanes, int banks, Banks* out)
{
    for (int g0 = 0; g0 < 64; g0 += group_lanes) {
        int worst = 1;
        for (int bank = 0; bank < banks; ++bank) {
            std::vector<int> seen;
            for (int l = g0; l < g0 + group_lanes; ++l)
                if (words[l] % banks == bank && std::find(seen.begin(), seen.end(), words[l]) == seen.end()) seen.push_back(words[l]);
            worst = std::max(worst, (int)seen.size());
        }
        out->group_steps += 1;
        out->extra += worst - 1;
    }
}
// the 16 stores or loads of a workgroup in layout B: 4-byte words move as ds_read_b32 / ds_write_b32 (two groups of 32 lanes,
// bank = word % 32); 8-byte words as ds_read_b64 (two groups of 32, bank pair = word % 32) and ds_write_b64 (four groups of 16,
// bank pair = word % 16)
template <int B>
static void count_layout(bool store, int key_bytes, bool index, Banks* total)
{
    static Banks memo[2][2][2]; // (the map does not depend on the data: counted once per rule, added at every use)
    static bool known[2][2][2];
    Banks* out = &memo[store][key_bytes == 8][index];
    if (known[store][key_bytes == 8][index]) {
        total->group_steps += out->group_steps;
        total->extra += out->extra;
        return;
    }
    known[store][key_bytes == 8][index] = true;
    for (int wave = 0; wave < SORT_THREADS / 64; ++wave)
        for (int r = 0; r < SORT_PER_LANE; ++r) {
            int words[64];
            for (int l = 0; l < 64; ++l) words[l] = sort_phys(sort_slot<B>(wave * 64 + l, r));
            if (key_bytes == 4) count_instruction(words, 32, 32, out);
            else if (store) count_instruction(words, 16, 16, out);
            else count_instruction(words, 32, 32, out);
            if (index) count_instruction(words, 32, 32, out);
        }
    total->group_steps += out->group_steps;
    total->extra += out->extra;
}

// ---------------------------------------------------------------- a workgroup
template <typename K, bool INDEX>
struct Group {
    std::vector<K> lk_mem = std::vector<K>(SORT_TILE);
    std::vector<uint32_t> li_mem = std::vector<uint32_t>(INDEX ? SORT_TILE : 0);
    std::vector<char> lk_w = std::vector<char>(SORT_TILE, 0), li_w = std::vector<char>(INDEX ? SORT_TILE : 0, 0);
    LdsView<K> lk{&lk_mem, &lk_w};
    LdsView<uint32_t> li{&li_mem, &li_w};
    std::vector<SortRegs<K, INDEX>> g = std::vector<SortRegs<K, INDEX>>(SORT_THREADS);

    template <int FROM, int TO>
    void relayout()
    {
        for (int t = 0; t < SORT_THREADS; ++t) sort_lds_store<FROM, K, INDEX>(lk, li, t, g[t]);
        for (int t = 0; t < SORT_THREADS; ++t) sort_lds_load<TO, K, INDEX>(lk, li, t, g[t]);
        count_layout<FROM>(true, (int)sizeof(K), INDEX, &g_banks[sizeof(K) == 8]);
        count_layout<TO>(false, (int)sizeof(K), INDEX, &g_banks[sizeof(K) == 8]);
    }
    template <int B>
    void steps(int stage, int hi, int lo)
    {
        for (int t = 0; t < SORT_THREADS; ++t) sort_steps<B, K, INDEX>(g[t], t, stage, hi, lo);
    }
};

template <typename K>
struct Buffer { // rows x n keys and indices with a write count per element
    std::vector<K> k;
    std::vector<uint32_t> i;
    std::vector<int> writes;
    explicit Buffer(size_t total) : k(total), i(total), writes(total, 0) {}
};

// k_sort_tile
template <typename K, bool INDEX>
static void launch_tile(const std::vector<K>& in, Buffer<K>& out, size_t rows, size_t n, const SortPlan& plan, bool descending)
{
    std::fill(out.writes.begin(), out.writes.end(), 0);
    for (size_t group = 0; group < plan.groups; ++group) {
        Group<K, INDEX> w;
        const int sp = plan.seg_log2;
        for (int t = 0; t < SORT_THREADS; ++t)
            for (int r = 0; r < SORT_PER_LANE; ++r) {
                const SortCell c = sort_tile_cell(plan, rows, n, group, sort_slot<8>(t, r));
                CHECK(!c.valid || c.row * n + c.col < in.size(), "tile load outside the data");
                w.g[t].k[r] = c.valid ? sort_to_key<K>(in[c.row * n + c.col], descending) : (K)~(K)0;
                if (INDEX) w.g[t].i[INDEX ? r : 0] = c.valid ? (uint32_t)c.col : SORT_PAD_INDEX;
            }
        w.template relayout<8, 0>();
        for (int t = 0; t < SORT_THREADS; ++t) sort_first_stages<K, INDEX>(w.g[t], t, sp);
        for (int s = SORT_LANE_LOG2 + 1; s <= sp; ++s) {
            const int stage = s == sp ? SORT_ASCENDING : s;
            if (s > 8) {
                w.template relayout<0, 8>();
                w.template steps<8>(stage, s - 1, 8);
                w.template relayout<8, 4>();
            } else {
                w.template relayout<0, 4>();
            }
            w.template steps<4>(stage, s - 1 < 7 ? s - 1 : 7, 4);
            w.template relayout<4, 0>();
            w.template steps<0>(stage, 3, 0);
        }
        w.template relayout<0, 8>();
        for (int t = 0; t < SORT_THREADS; ++t)
            for (int r = 0; r < SORT_PER_LANE; ++r) {
                const SortCell c = sort_tile_cell(plan, rows, n, group, sort_slot<8>(t, r));
                if (c.valid) {
                    const size_t at = c.row * n + c.col;
                    out.k[at] = w.g[t].k[r];
                    if (INDEX) {
                        out.i[at] = w.g[t].i[INDEX ? r : 0];
                        CHECK(out.i[at] != SORT_PAD_INDEX, "a pad reached output %zu of the tile launch", at);
                    }
                    ++out.writes[at];
                }
            }
    }
    for (size_t e = 0; e < out.writes.size(); ++e) CHECK(out.writes[e] == 1, "tile launch wrote element %zu %d times", e, out.writes[e]);
}

// k_sort_merge
template <typename K, bool INDEX>
static void launch_merge(const Buffer<K>& src, Buffer<K>& dst, size_t rows, size_t n, const SortPlan& plan, size_t run)
{
    std::fill(dst.writes.begin(), dst.writes.end(), 0);
    for (size_t row = 0; row < rows; ++row) {
        size_t prev_start = (size_t)-1;
        uint32_t prev_a1 = 0, prev_d1 = 0, taken = 0;
        for (size_t tile = 0; tile < plan.tiles; ++tile) {
            const SortMerge m = sort_merge_geom(n, run, tile);
            const size_t base = row * n + m.start;
            CHECK(m.start + m.la + m.lb <= n && m.d0 < m.d1 && m.d1 <= m.la + m.lb, "merge geometry of tile %zu", tile);
            const RunView<K> a{src.k.data() + base, m.la}, b{src.k.data() + base + m.la, m.lb};
            uint32_t lo0, hi0, lo1, hi1;
            sort_split_range(m.d0, m.la, m.lb, &lo0, &hi0);
            sort_split_range(m.d1, m.la, m.lb, &lo1, &hi1);
            for (int step = sort_split_steps(m.la, m.lb); step > 0; --step) {
                sort_split_step(a, b, m.d0, &lo0, &hi0);
                sort_split_step(a, b, m.d1, &lo1, &hi1);
            }
            CHECK(lo0 == hi0 && lo1 == hi1, "the bisection has not ended: [%u, %u] [%u, %u]", lo0, hi0, lo1, hi1);
            const uint32_t a0 = lo0, a1 = lo1, na = a1 - a0, b0 = m.d0 - a0, nb = (m.d1 - m.d0) - na;
            CHECK(a0 <= a1 && a1 <= m.la && m.d0 - a0 <= m.d1 - a1 && m.d1 - a1 <= m.lb, "split not monotone at tile %zu", tile);
            if (m.start == prev_start) {
                CHECK(m.d0 == prev_d1 && a0 == prev_a1, "split not unique at tile %zu: %u against %u", tile, a0, prev_a1);
            } else {
                CHECK(m.d0 == 0 && a0 == 0, "a pair does not start at its first output");
                taken = 0;
            }
            taken += na + nb;
            if (m.d1 == m.la + m.lb) CHECK(taken == m.la + m.lb && a1 == m.la, "the pieces of a pair sum to %u of %u", taken, m.la + m.lb);
            prev_start = m.start; prev_a1 = a1; prev_d1 = m.d1;

            Group<K, INDEX> w;
            for (int t = 0; t < SORT_THREADS; ++t)
                for (int r = 0; r < SORT_PER_LANE; ++r) {
                    const int64_t s = sort_merge_source(sort_slot<8>(t, r), a0, na, b0, nb, m.la);
                    CHECK(s < (int64_t)(m.la + m.lb), "merge load outside the pair");
                    w.g[t].k[r] = s >= 0 ? src.k[base + (size_t)s] : (K)~(K)0;
                    if (INDEX) w.g[t].i[INDEX ? r : 0] = s >= 0 ? src.i[base + (size_t)s] : SORT_PAD_INDEX;
                }
            w.template steps<8>(SORT_ASCENDING, 11, 8);
            w.template relayout<8, 4>();
            w.template steps<4>(SORT_ASCENDING, 7, 4);
            w.template relayout<4, 0>();
            w.template steps<0>(SORT_ASCENDING, 3, 0);
            w.template relayout<0, 8>();
            const uint32_t produced = m.d1 - m.d0;
            for (int t = 0; t < SORT_THREADS; ++t)
                for (int r = 0; r < SORT_PER_LANE; ++r) {
                    const uint32_t e = (uint32_t)sort_slot<8>(t, r);
                    if (e < produced) {
                        const size_t at = base + m.d0 + e;
                        dst.k[at] = w.g[t].k[r];
                        if (INDEX) {
                            dst.i[at] = w.g[t].i[INDEX ? r : 0];
                            CHECK(dst.i[at] != SORT_PAD_INDEX, "a pad reached output %zu of a merge pass", at);
                        }
                        ++dst.writes[at];
                    }
                }
        }
    }
    for (size_t e = 0; e < dst.writes.size(); ++e) CHECK(dst.writes[e] == 1, "merge pass wrote element %zu %d times", e, dst.writes[e]);
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t next_random()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return g_seed;
}

template <typename K, bool INDEX>
static void run_case(size_t rows, size_t n, bool descending)
{
    const size_t total = rows * n;
    std::vector<K> x(total);
    // a third random bits, the rest from 16 patterns (ties), with the extremes of the key range among them
    const K few[16] = {(K)0, (K)~(K)0, (K)1 << (8 * sizeof(K) - 1), (K)(~(K)0 >> 1), (K)1, (K)2, (K)3, (K)0x7f800000u,
                       (K)0xff800000u, (K)0x3f800000u, (K)0xbf800000u, (K)5, (K)6, (K)7, (K)8, (K)9};
    for (size_t e = 0; e < total; ++e) x[e] = next_random() % 3 == 0 ? (K)next_random() : few[next_random() % 16];
    const SortPlan plan = sort_plan(rows, n);
    CHECK(sort_supported(rows, n) && plan.groups > 0 && plan.passes == sort_ceil_log2((n + SORT_TILE - 1) / SORT_TILE), "plan");
    Buffer<K> one(total), two(total);
    Buffer<K>*cur = &one, *other = &two;
    launch_tile<K, INDEX>(x, *cur, rows, n, plan, descending);
    size_t run = SORT_TILE;
    for (int pass = 0; pass < plan.passes; ++pass, run *= 2) {
        launch_merge<K, INDEX>(*cur, *other, rows, n, plan, run);
        std::swap(cur, other);
    }
    CHECK(plan.passes == 0 || run >= n, "the last run does not cover the row");
    for (size_t row = 0; row < rows; ++row) {
        std::vector<uint32_t> order(n);
        for (size_t j = 0; j < n; ++j) order[j] = (uint32_t)j;
        const K* src = x.data() + row * n;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) { return sort_to_key<K>(src[p], descending) < sort_to_key<K>(src[q], descending); });
        for (size_t j = 0; j < n; ++j) {
            const size_t at = row * n + j;
            CHECK(sort_to_bits<K>(cur->k[at], descending) == src[order[j]], "row %zu rank %zu: wrong value", row, j);
            if (INDEX) CHECK(cur->i[at] == order[j], "row %zu rank %zu: index %u, stable_sort %u", row, j, cur->i[at], order[j]);
        }
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: sim_sort <shapes file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    // the swizzle is a bijection of the allocation
    std::vector<char> hit(SORT_TILE, 0);
    for (int s = 0; s < SORT_TILE; ++s) {
        const int w = sort_phys(s);
        CHECK(w >= 0 && w < SORT_TILE && !hit[w], "sort_phys is not a bijection at slot %d", s);
        if (w >= 0 && w < SORT_TILE) hit[w] = 1;
    }
    char line[256];
    int lines = 0;
    while (fgets(line, sizeof line, f)) {
        size_t rows, n;
        if (line[0] == '#' || sscanf(line, "%zu %zu", &rows, &n) != 2) continue;
        ++lines;
        for (int descending = 0; descending < 2; ++descending) {
            run_case<uint32_t, false>(rows, n, descending != 0);
            run_case<uint32_t, true>(rows, n, descending != 0);
            run_case<uint64_t, false>(rows, n, descending != 0);
            run_case<uint64_t, true>(rows, n, descending != 0);
        }
    }
    fclose(f);
    printf("LDS bank cycles of the layout changes: f32 %ld group steps, %ld extra bank cycles; f64 %ld group steps, %ld extra bank cycles\n",
           g_banks[0].group_steps, g_banks[0].extra, g_banks[1].group_steps, g_banks[1].extra);
    printf("%d shape lines (both key widths, both directions, with and without index), %ld failures\n", lines, g_fail);
    if (g_fail) return 1;
    printf("ok\n");
    return 0;
}
