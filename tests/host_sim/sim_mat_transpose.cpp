// sim_mat_transpose.cpp -- the tile geometry, lane maps and lane loops of mat_transpose.hip (basic_dsp_amd/csrc/
// mat_transpose_core.h) on the host, threads as loops.  The kernels hand their pointers to tp_lane_load / tp_lane_store /
// tp_lane_flat; here the same functions get arrays that count every write and refuse every access out of bounds, in
// global memory and in LDS (an LDS read of a slot no thread wrote counts as well).
//
//   tiled and flat   every R x C with R, C in 1..70, and {127, 128, 129, 1023, 1024, 1025} x {1, 2, 3} both ways round:
//                    every destination element written exactly once with dst[c][r] = src[r][c], tiles of 64 and of 32,
//                    one tile per block and a grid of 3 blocks that loops; the flat map both ways round over several
//                    grids.  Both paths run on every shape, whichever the launcher would pick.
//   index widths     everything once with 32-bit and once with 64-bit indices
//   maps only        70000 x 70002 > 2^32 elements with 64-bit indices: the first tiles, the tiles around flat index
//                    2^32 and the last ones, and lanes of the flat map there, against the index arithmetic
//   LDS banks        the conflicts of the row-wise writes and the column-wise reads of a tile from tp_lds_slot and the
//                    lane groups of the instructions: bank (a / 4) % 32 for every write and for 4-byte reads, (a / 4) % 64
//                    for 8- and 16-byte reads; extra cycles = (most distinct dword addresses on one bank) - 1 per group.
//                    0 at the pitch of S + 1 for 4, 8 and 16 bytes; the same count at a pitch of S for comparison.
//
// g++ -O2 -std=c++17 (optionally -fsanitize=address,undefined) sim_mat_transpose.cpp && ./a.out
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_transpose_core.h"

using namespace bdsp;

static int failures = 0;
#define EXPECT(cond, ...)                                                                          \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                          \
    } while (0)

typedef unsigned long long P; // the element: its value is its source index + 1

static unsigned long long reads_oob = 0, writes_oob = 0, lds_oob = 0, lds_unwritten = 0;

struct InArr {
    const std::vector<P>* v;
    P operator[](size_t i) const
    {
        if (i >= v->size()) { ++reads_oob; return ~P(0); }
        return (*v)[i];
    }
};

struct OutArr {
    std::vector<P>* v;
    std::vector<int>* writes;
    struct Ref {
        OutArr* a;
        size_t i;
        void operator=(P x)
        {
            if (i >= a->v->size()) { ++writes_oob; return; }
            (*a->v)[i] = x;
            ++(*a->writes)[i];
        }
    };
    Ref operator[](size_t i) { return Ref{this, i}; }
};

// an LDS tile: bounds-checked both ways, and a read must find a slot written since the last clear()
struct LdsArr {
    std::vector<P>* v;
    std::vector<char>* written;
    struct Ref {
        LdsArr* a;
        long i;
        void operator=(P x)
        {
            if (i < 0 || (size_t)i >= a->v->size()) { ++lds_oob; return; }
            (*a->v)[i] = x;
            (*a->written)[i] = 1;
        }
        operator P() const
        {
            if (i < 0 || (size_t)i >= a->v->size()) { ++lds_oob; return ~P(0); }
            if (!(*a->written)[i]) ++lds_unwritten;
            return (*a->v)[i];
        }
    };
    Ref operator[](long i) { return Ref{this, i}; }
};

static std::vector<P> source(size_t n)
{
    std::vector<P> x(n);
    for (size_t i = 0; i < n; ++i) x[i] = i + 1;
    return x;
}

static void check_result(const std::vector<P>& dst, const std::vector<int>& writes, size_t R, size_t C, const char* what)
{
    for (size_t c = 0; c < C; ++c)
        for (size_t r = 0; r < R; ++r) {
            const size_t d = c * R + r;
            EXPECT(writes[d] == 1, "%s %zu x %zu: dst[%zu][%zu] written %d times", what, R, C, c, r, writes[d]);
            EXPECT(dst[d] == r * C + c + 1, "%s %zu x %zu: dst[%zu][%zu] holds source %llu", what, R, C, c, r, dst[d] - 1);
        }
}

// the tiled kernel: `blocks` workgroups of 256 threads, each looping over its tiles as k_tp_tiled does
template <typename IDX, int S>
static void tiled_case(size_t R, size_t C, size_t blocks)
{
    const std::vector<P> src = source(R * C);
    std::vector<P> dst(R * C, 0), lds(tp_lds_elems(S));
    std::vector<int> writes(R * C, 0);
    std::vector<char> written(lds.size());
    const size_t tiles_c = tp_tiles_along(C, S), ntiles = tp_tiles_along(R, S) * tiles_c;
    if (blocks == 0 || blocks > ntiles) blocks = ntiles;
    for (size_t b = 0; b < blocks; ++b)
        for (IDX t = (IDX)b; t < (IDX)ntiles; t += (IDX)blocks) {
            IDX r0, c0;
            tp_tile_origin<IDX>(t, (IDX)tiles_c, S, &r0, &c0);
            EXPECT((size_t)r0 < R && (size_t)c0 < C && r0 % S == 0 && c0 % S == 0, "tile %zu of %zu x %zu", (size_t)t, R, C);
            written.assign(written.size(), 0);
            for (int tid = 0; tid < TP_THREADS; ++tid)
                tp_lane_load<P, IDX, S>(InArr{&src}, LdsArr{&lds, &written}, (IDX)R, (IDX)C, r0, c0, tid);
            // __syncthreads()
            for (int tid = 0; tid < TP_THREADS; ++tid)
                tp_lane_store<P, IDX, S>(LdsArr{&lds, &written}, OutArr{&dst, &writes}, (IDX)R, (IDX)C, r0, c0, tid);
        }
    check_result(dst, writes, R, C, S == 64 ? "tiled 64" : "tiled 32");
}

static const unsigned GRIDS[][2] = {{1, 1}, {1, 3}, {2, 4}, {1, 64}, {3, 7}, {5, 256}}; // {blocks, threads per block}

template <typename IDX>
static void flat_case(size_t R, size_t C, const unsigned* g)
{
    const std::vector<P> src = source(R * C);
    for (int near_is_src = 0; near_is_src < 2; ++near_is_src) {
        // near_is_src: the source is the flat [N][K] side, K = C; else the destination is, K = R
        const size_t N = near_is_src ? R : C, K = near_is_src ? C : R, stride = (size_t)g[0] * g[1];
        std::vector<P> dst(R * C, 0);
        std::vector<int> writes(R * C, 0);
        for (size_t first = 0; first < stride; ++first)
            tp_lane_flat<P, IDX>(InArr{&src}, OutArr{&dst, &writes}, (IDX)(R * C), (IDX)N, (IDX)K, near_is_src != 0, (IDX)first,
                                 (IDX)stride);
        check_result(dst, writes, R, C, near_is_src ? "flat, source near" : "flat, destination near");
    }
}

template <typename IDX>
static void shape(size_t R, size_t C, bool all_grids)
{
    tiled_case<IDX, 64>(R, C, 0);
    tiled_case<IDX, 32>(R, C, 0);
    tiled_case<IDX, 64>(R, C, 3);
    tiled_case<IDX, 32>(R, C, 3);
    if (all_grids) { for (const auto& g : GRIDS) flat_case<IDX>(R, C, g); }
    else { flat_case<IDX>(R, C, GRIDS[4]); flat_case<IDX>(R, C, GRIDS[5]); }
}

template <typename IDX>
static void check_all()
{
    for (size_t R = 1; R <= 70; ++R)
        for (size_t C = 1; C <= 70; ++C) shape<IDX>(R, C, R <= 9 && C <= 9);
    for (size_t n : {127, 128, 129, 1023, 1024, 1025})
        for (size_t k = 1; k <= 3; ++k) { shape<IDX>(n, k, false); shape<IDX>(k, n, false); }
    // the launcher's choice
    EXPECT(tp_is_thin(70000, 3) && tp_is_thin(3, 70000) && tp_is_thin(1, 1) && tp_is_thin(15, 15) && !tp_is_thin(16, 16) &&
           !tp_is_thin(70000, 16), "thin-path rule");
}

// maps only: an extent above 2^32 with 64-bit indices.  The source "array" answers its index, the destination checks
// that the value it is handed is the source index its own index stands for; nothing is stored.
static const size_t BIG_R = 70000, BIG_C = 70002;
static unsigned long long big_checked = 0;
struct BigIn {
    P operator[](size_t i) const
    {
        if (i >= BIG_R * BIG_C) { ++reads_oob; return ~P(0); }
        return i + 1;
    }
};
struct BigOut {
    struct Ref {
        size_t d;
        void operator=(P x)
        {
            if (d >= BIG_R * BIG_C) { ++writes_oob; return; }
            const size_t c = d / BIG_R, r = d % BIG_R;
            EXPECT(x == r * BIG_C + c + 1, "70000 x 70002: dst index %zu got source %llu", d, x - 1);
            ++big_checked;
        }
    };
    Ref operator[](size_t d) { return Ref{d}; }
};

static void check_large()
{
    const size_t total = BIG_R * BIG_C;
    EXPECT(total > (size_t(1) << 32) && !tp_fits_32(total) && tp_fits_32((size_t(1) << 31) - 1) && !tp_fits_32(size_t(1) << 31),
           "index width");
    constexpr int S = 64;
    const size_t tiles_c = tp_tiles_along(BIG_C, S), tiles_r = tp_tiles_along(BIG_R, S), ntiles = tiles_r * tiles_c;
    EXPECT(tiles_c == 1094 && tiles_r == 1094, "tile counts");
    std::vector<P> lds(tp_lds_elems(S));
    std::vector<char> written(lds.size());
    // the tile that holds source index 2^32, its neighbours, the first and the last tiles (partial in both directions)
    const size_t at = ((size_t(1) << 32) / BIG_C / S) * tiles_c + ((size_t(1) << 32) % BIG_C) / S;
    const size_t tiles[] = {0, 1, tiles_c - 1, tiles_c, at - 1, at, at + 1, ntiles - tiles_c, ntiles - 2, ntiles - 1};
    for (size_t t : tiles) {
        size_t r0, c0;
        tp_tile_origin<size_t>(t, tiles_c, S, &r0, &c0);
        EXPECT(r0 == t / tiles_c * S && c0 == t % tiles_c * S, "origin of tile %zu", t);
        written.assign(written.size(), 0);
        for (int tid = 0; tid < TP_THREADS; ++tid)
            tp_lane_load<P, size_t, S>(BigIn{}, LdsArr{&lds, &written}, BIG_R, BIG_C, r0, c0, tid);
        const unsigned long long before = big_checked;
        for (int tid = 0; tid < TP_THREADS; ++tid)
            tp_lane_store<P, size_t, S>(LdsArr{&lds, &written}, BigOut{}, BIG_R, BIG_C, r0, c0, tid);
        const size_t h = BIG_R - r0 < (size_t)S ? BIG_R - r0 : S, w = BIG_C - c0 < (size_t)S ? BIG_C - c0 : S;
        EXPECT(big_checked - before == h * w, "tile %zu stored %llu of %zu elements", t, big_checked - before, h * w);
    }
    // the flat map: lanes whose first trips lie at the start, around 2^32 and at the end, three trips each (N = BIG_C
    // long, K = BIG_R short would not be thin -- the map does not care)
    const size_t stride = (size_t)2048 * 256;
    const size_t firsts[] = {0, 1, stride - 1};
    for (size_t first : firsts) {
        const unsigned long long before = big_checked;
        tp_lane_flat<P, size_t>(BigIn{}, BigOut{}, (size_t)3 * stride, BIG_R, BIG_C, true, first, stride);
        EXPECT(big_checked - before == 3, "flat lane %zu", first);
    }
    {   // trips that cross 2^32: a lane with a stride that reaches it in its third trip
        const size_t big_stride = (size_t(1) << 31) + 12345;
        const unsigned long long before = big_checked;
        tp_lane_flat<P, size_t>(BigIn{}, BigOut{}, total, BIG_R, BIG_C, true, 77, big_stride);
        EXPECT(big_checked - before == (total - 77 + big_stride - 1) / big_stride, "flat lane across 2^32");
    }
    std::printf("maps only: %zu x %zu > 2^32\n", BIG_R, BIG_C);
}

// ---------------------------------------------------------------------------------------------
// LDS bank conflicts of one tile pass, from the slot map and the lane groups of the instruction
// ---------------------------------------------------------------------------------------------
typedef std::vector<std::vector<int>> Groups;

static Groups contiguous(int size)
{
    Groups g;
    for (int l = 0; l < TP_LANES; l += size) {
        g.emplace_back();
        for (int i = 0; i < size; ++i) g.back().push_back(l + i);
    }
    return g;
}

static Groups read_b128_groups()
{
    const int a[16] = {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27};
    const int b[16] = {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31};
    Groups g(4);
    for (int i = 0; i < 16; ++i) { g[0].push_back(a[i]); g[1].push_back(b[i]); g[2].push_back(a[i] + 32); g[3].push_back(b[i] + 32); }
    return g;
}

// extra LDS cycles of every wave instruction of one pass over a tile of elements of E bytes with `pitch` elements per row
static long conflicts(int E, int pitch, bool column_reads)
{
    const int S = tp_tile_side((size_t)E), dwords = E / 4;
    const Groups groups = column_reads ? (E == 16 ? read_b128_groups() : contiguous(32))
                                       : contiguous(E == 4 ? 32 : (E == 8 ? 16 : 8));
    const int banks = column_reads && E >= 8 ? 64 : 32;
    long extra = 0;
    for (int k = 0; k < tp_steps(S); ++k)
        for (int wave = 0; wave < TP_THREADS / TP_LANES; ++wave)
            for (const auto& group : groups) {
                std::map<int, std::set<long>> on_bank; // bank -> the distinct dword addresses on it
                for (int lane : group) {
                    int r, c;
                    if (column_reads) tp_store_rc(k, wave * TP_LANES + lane, S, &r, &c);
                    else tp_load_rc(k, wave * TP_LANES + lane, S, &r, &c);
                    EXPECT(r >= 0 && r < S && c >= 0 && c < S, "lane map out of the tile");
                    if (pitch == tp_pitch(S)) EXPECT(tp_lds_slot(r, c, S) == r * pitch + c, "slot map");
                    const long a = (long)(r * pitch + c) * E; // byte address
                    for (int d = 0; d < dwords; ++d) on_bank[(int)((a / 4 + d) % banks)].insert(a / 4 + d);
                }
                size_t worst = 1;
                for (const auto& b : on_bank) worst = b.second.size() > worst ? b.second.size() : worst;
                extra += (long)worst - 1;
            }
    return extra;
}

static void check_banks()
{
    long padded[3][2], plain[3][2];
    const int sizes[3] = {4, 8, 16};
    for (int i = 0; i < 3; ++i) {
        const int S = tp_tile_side((size_t)sizes[i]);
        for (int side = 0; side < 2; ++side) {
            padded[i][side] = conflicts(sizes[i], tp_pitch(S), side != 0);
            plain[i][side] = conflicts(sizes[i], S, side != 0);
            EXPECT(padded[i][side] == 0, "%d-byte elements: %ld extra cycles on the %s side", sizes[i], padded[i][side], side ? "read" : "write");
        }
        EXPECT(plain[i][0] == 0 && plain[i][1] > 0, "%d-byte elements at a pitch of S", sizes[i]);
    }
    EXPECT(tp_tile_side(4) == 64 && tp_tile_side(8) == 64 && tp_tile_side(16) == 32 && tp_pitch(64) == 65 && tp_pitch(32) == 33,
           "tile geometry");
    std::printf("LDS bank conflicts at pitch S + 1: 4 B write %ld read %ld, 8 B write %ld read %ld, 16 B write %ld read %ld\n",
                padded[0][0], padded[0][1], padded[1][0], padded[1][1], padded[2][0], padded[2][1]);
    std::printf("LDS bank conflicts at pitch S (for comparison): 4 B write %ld read %ld, 8 B write %ld read %ld, 16 B write %ld read %ld\n",
                plain[0][0], plain[0][1], plain[1][0], plain[1][1], plain[2][0], plain[2][1]);
}

int main()
{
    check_all<unsigned>();
    check_all<size_t>();
    std::printf("tiled (64, 32) and flat: R x C 1..70 x 1..70, 127 128 129 1023 1024 1025 x 1 2 3 both ways round\n");
    std::printf("32- and 64-bit indices\n");
    check_large();
    check_banks();
    EXPECT(reads_oob == 0, "%llu global reads out of bounds", reads_oob);
    EXPECT(writes_oob == 0, "%llu global writes out of bounds", writes_oob);
    EXPECT(lds_oob == 0, "%llu LDS accesses out of bounds", lds_oob);
    EXPECT(lds_unwritten == 0, "%llu LDS reads of a slot nobody wrote", lds_unwritten);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
