// Host simulation of detect.hip: the functions of basic_dsp_amd/csrc/detect_core.h with threads as loops, on every line of
// tests/detect_shapes.txt (rows n order boundary kind) and both precisions.  A stand-alone program:
// g++ -O2 -std=c++17 [-fsanitize=address,undefined] sim_detect.cpp && ./a.out tests/detect_shapes.txt
//
// Per line and precision it runs the four launches (count, scan tiles, scan rows, write) as the kernels do and checks
//   - every detection of the serial model (the definition, position by position) is written exactly once, at the slot a
//     serial row-major scan gives, with its index and the bits of its value, and nothing is written at or beyond the
//     capacity (capacities: beyond the total, the total, one less, and a cut inside a wave);
//   - every LDS slot that is written or read lies inside the allocation, and every slot that is read was written before;
//   - the boundary index function agrees with a brute-force walk from the row;
//   - the count of every (step, wave) segment, the segment bases and the lane ranks agree with a serial count, across the
//     wave and step seams;
//   - the prefix launches give the serial 64-bit sums.
// Once: the prefix arithmetic over several chunks with counts whose sum passes 2^32.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "../../basic_dsp_amd/csrc/detect_core.h"

using namespace bdsp;

static long g_failures = 0;
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

static long g_lds_accesses = 0, g_boundary_checks = 0, g_segments = 0, g_lane_ranks = 0, g_written = 0, g_scan_entries = 0, g_cases = 0;

// LDS through a view that checks every access: inside the allocation, written before it is read
template <typename V> struct CheckedLds {
    std::vector<V>* cells;
    std::vector<unsigned char>* written;
    bool* bad;
    struct Ref {
        const CheckedLds* l;
        int slot;
        bool inside() const { return slot >= 0 && (size_t)slot < l->cells->size(); }
        operator V() const
        {
            ++g_lds_accesses;
            if (!inside() || !(*l->written)[(size_t)slot]) { *l->bad = true; return V(); }
            return (*l->cells)[(size_t)slot];
        }
        Ref& operator=(V v)
        {
            ++g_lds_accesses;
            if (!inside()) { *l->bad = true; return *this; }
            (*l->cells)[(size_t)slot] = v;
            (*l->written)[(size_t)slot] = 1;
            return *this;
        }
    };
    Ref operator[](int slot) const { return Ref{this, slot}; }
};

template <typename V> struct Lds {
    std::vector<V> cells;
    std::vector<unsigned char> written;
    bool bad = false;
    explicit Lds(size_t n) : cells(n), written(n, 0) {}
    CheckedLds<V> view() { return CheckedLds<V>{&cells, &written, &bad}; }
    void clear() { std::fill(written.begin(), written.end(), 0); }
};

template <typename T> struct Fmt;
template <> struct Fmt<float> { using U = uint32_t; static const char* name() { return "f32"; } };
template <> struct Fmt<double> { using U = uint64_t; static const char* name() { return "f64"; } };

template <typename T> typename Fmt<T>::U bits_of(T v)
{
    typename Fmt<T>::U u;
    std::memcpy(&u, &v, sizeof(T));
    return u;
}

// 16 levels of both signs with +-0, and now and then +-inf, +-NaN or a denormal
template <typename T> T sample(bool special)
{
    const uint64_t r = rnd();
    if (special && r % 10 < 2) {
        switch ((r >> 8) % 7) {
        case 0: return std::numeric_limits<T>::quiet_NaN();
        case 1: return -std::numeric_limits<T>::quiet_NaN();
        case 2: return std::numeric_limits<T>::infinity();
        case 3: return -std::numeric_limits<T>::infinity();
        case 4: return std::numeric_limits<T>::denorm_min();
        case 5: return (T)-0.0;
        default: return (T)0.0;
        }
    }
    const int level = (int)((r >> 16) % 16) - 8;
    return level == 0 && ((r >> 32) & 1) ? (T)-0.0 : (T)level * (T)0.25;
}

// position q of a row by the definition, walking one position at a time: the row index, or -1 where nothing is read
static int64_t brute_index(int64_t q, int64_t n, int boundary)
{
    if (boundary == DETECT_OPEN) return q >= 0 && q < n ? q : -1;
    if (boundary == DETECT_NEAREST) { while (q < 0) ++q; while (q >= n) --q; return q; }
    while (q < 0) q += n;
    while (q >= n) q -= n;
    return q;
}

struct Shape {
    size_t rows, n;
    int order, boundary, kind;
    bool neg_inf;
    std::string text;
};

template <typename T> struct Problem {
    Shape sh;
    std::vector<T> x;          // rows x n
    double t = 0.0;            // scalar
    std::vector<double> t_rows;
    std::vector<T> t_cells;    // n or rows x n
    size_t t_stride = 0;
};

// the definition
template <typename T> bool model_detects(const Problem<T>& p, size_t row, size_t j)
{
    const Shape& s = p.sh;
    const T v = p.x[row * s.n + j];
    const double t_row = s.kind == DETECT_PER_ROW ? p.t_rows[row] : p.t;
    if (s.kind == DETECT_SCALAR || s.kind == DETECT_PER_ROW) { if (!((double)v > t_row)) return false; }
    if (s.kind == DETECT_PROFILE) { if (!(v > p.t_cells[j])) return false; }
    if (s.kind == DETECT_PER_CELL) { if (!(v > p.t_cells[row * s.n + j])) return false; }
    for (int d = -s.order; d <= s.order; ++d) {
        if (d == 0) continue;
        const int64_t g = brute_index((int64_t)j + d, (int64_t)s.n, s.boundary);
        if (g < 0) continue;
        if (!(v > p.x[row * s.n + (size_t)g])) return false;
    }
    return true;
}

// the chunk loop of k_detect_scan_tiles / k_detect_scan_rows over `entries`: exclusive prefix in place, the total returned
static int64_t sim_scan(std::vector<int64_t>& entries)
{
    Lds<int64_t> b0(DETECT_THREADS), b1(DETECT_THREADS);
    const size_t count = entries.size();
    int64_t carry = 0;
    for (size_t c0 = 0; c0 < count; c0 += DETECT_SCAN_CHUNK) {
        b0.clear();
        b1.clear();
        std::vector<int64_t> own(DETECT_THREADS, 0);
        CheckedLds<int64_t> src = b0.view(), dst = b1.view();
        for (int tid = 0; tid < DETECT_THREADS; ++tid) {
            own[(size_t)tid] = detect_scan_own(entries, detect_scan_first(c0, tid), count);
            src[tid] = own[(size_t)tid];
        }
        for (int step = 0; step < DETECT_SCAN_STEPS; ++step) {
            for (int tid = 0; tid < DETECT_THREADS; ++tid) detect_scan_step(src, dst, tid, step);
            CheckedLds<int64_t> t = src; src = dst; dst = t;
        }
        CHECK(src.cells == (detect_scan_result_buffer() ? &b1.cells : &b0.cells), "the scan result's buffer");
        const int64_t total = src[DETECT_THREADS - 1];
        for (int tid = 0; tid < DETECT_THREADS; ++tid) {
            const int64_t inclusive = src[tid];
            detect_scan_write(entries, detect_scan_first(c0, tid), count, carry + inclusive - own[(size_t)tid]);
        }
        carry += total;
        g_scan_entries += (long)(count - c0 < (size_t)DETECT_SCAN_CHUNK ? count - c0 : (size_t)DETECT_SCAN_CHUNK);
    }
    CHECK(!b0.bad && !b1.bad, "a scan buffer slot outside the allocation or read before it was written");
    return carry;
}

// the tile phase of k_detect_count / k_detect_write: fills lds, returns the flags of every (tid, k) and the segment counts
template <typename T>
void sim_tile(const Problem<T>& p, size_t row, size_t tile, Lds<T>& lds, Lds<unsigned>& seg, std::vector<unsigned>& mine)
{
    const Shape& s = p.sh;
    lds.clear();
    seg.clear();
    CheckedLds<T> l = lds.view();
    CheckedLds<unsigned> sg = seg.view();
    const int points = detect_tile_points(s.n, tile), loaded = detect_loaded(points, s.order);
    const T* src = p.x.data() + row * s.n;
    const int64_t first = detect_first_position(tile, s.order);
    for (int tid = 0; tid < DETECT_THREADS; ++tid)
        for (int q = tid; q < loaded; q += DETECT_THREADS) {
            const int64_t g = rank_src_index(first + q, (int64_t)s.n, s.boundary);
            CHECK(g < (int64_t)s.n, "source index beyond the row");
            l[q] = g < 0 ? (T)0 : src[g];
        }
    const double t_row = s.kind == DETECT_PER_ROW ? p.t_rows[row] : p.t;
    mine.assign(DETECT_THREADS, 0u);
    for (int tid = 0; tid < DETECT_THREADS; ++tid)
        for (int k = 0; k < DETECT_PER_LANE; ++k) {
            const int o = detect_cell(tid, k);
            if (o >= points) continue;
            const size_t j = tile * (size_t)DETECT_TILE + (size_t)o;
            const int slot = detect_slot(o, s.order);
            const T t_cell = s.kind >= DETECT_PROFILE ? p.t_cells[row * p.t_stride + j] : (T)0;
            if (detect_above<T>(l[slot], s.kind, t_row, t_cell) &&
                detect_is_peak<T>(l, slot, detect_reach(j, s.n, s.order, s.boundary, 0), detect_reach(j, s.n, s.order, s.boundary, 1)))
                mine[(size_t)tid] |= 1u << k;
            CHECK(((mine[(size_t)tid] >> k) & 1u) == (model_detects(p, row, j) ? 1u : 0u), "%s %s: the predicate of row %zu cell %zu", s.text.c_str(),
                  Fmt<T>::name(), row, j);
        }
    // the ballots: one per (step, wave); lane 0 stores the count
    for (int k = 0; k < DETECT_PER_LANE; ++k)
        for (int wave = 0; wave < DETECT_THREADS / DETECT_WAVE; ++wave) {
            uint64_t ballot = 0;
            for (int lane = 0; lane < DETECT_WAVE; ++lane) ballot |= (uint64_t)((mine[(size_t)(wave * DETECT_WAVE + lane)] >> k) & 1u) << lane;
            const int sidx = detect_segment(wave * DETECT_WAVE, k);
            sg[sidx] = (unsigned)detect_popcount(ballot);
            // a segment is 64 consecutive cells in index order
            CHECK(sidx == detect_cell(wave * DETECT_WAVE, k) / DETECT_WAVE && detect_cell(wave * DETECT_WAVE + 63, k) == sidx * DETECT_WAVE + 63, "segment map");
            unsigned serial = 0;
            for (int c = sidx * DETECT_WAVE; c < (sidx + 1) * DETECT_WAVE && c < points; ++c)
                serial += model_detects(p, row, tile * (size_t)DETECT_TILE + (size_t)c) ? 1u : 0u;
            CHECK(serial == (unsigned)detect_popcount(ballot), "%s: the count of segment %d", s.text.c_str(), sidx);
            ++g_segments;
        }
}

template <typename T> void run_line(const Shape& s)
{
    using U = typename Fmt<T>::U;
    Problem<T> p;
    p.sh = s;
    const bool ramp = s.order > 64;
    p.x.resize(s.rows * s.n);
    for (size_t r = 0; r < s.rows; ++r)
        for (size_t j = 0; j < s.n; ++j) p.x[r * s.n + j] = ramp ? (T)((double)j - (double)s.n / 2 + (j % 413 == 7 ? 5000.0 + (double)(j + r) : 0.0)) : sample<T>(true);
    p.t = s.neg_inf ? -std::numeric_limits<double>::infinity() : 0.0;
    if (s.kind == DETECT_PER_ROW) for (size_t r = 0; r < s.rows; ++r) p.t_rows.push_back((double)sample<T>(r % 3 == 2));
    if (s.kind == DETECT_PROFILE) for (size_t j = 0; j < s.n; ++j) p.t_cells.push_back(sample<T>(true));
    if (s.kind == DETECT_PER_CELL) { for (size_t i = 0; i < s.rows * s.n; ++i) p.t_cells.push_back(sample<T>(true)); p.t_stride = s.n; }

    // the boundary index against a brute-force walk
    for (int64_t q = -(int64_t)(2 * s.order + 5); q < (int64_t)s.n + 2 * s.order + 5; ++q) {
        const int64_t g = rank_src_index(q, (int64_t)s.n, s.boundary);
        CHECK(g == brute_index(q, (int64_t)s.n, s.boundary), "%s: boundary index of %lld", s.text.c_str(), (long long)q);
        ++g_boundary_checks;
    }
    // the serial list
    std::vector<int64_t> want_index, want_count(s.rows, 0);
    std::vector<U> want_bits;
    for (size_t r = 0; r < s.rows; ++r)
        for (size_t j = 0; j < s.n; ++j)
            if (model_detects(p, r, j)) { want_index.push_back((int64_t)j); want_bits.push_back(bits_of(p.x[r * s.n + j])); ++want_count[r]; }
    const uint64_t total = want_index.size();

    const size_t tiles = detect_tiles(s.n);
    CHECK(detect_lds_bytes(s.order, sizeof(T)) == detect_data_offset() + sizeof(T) * (size_t)(DETECT_TILE + 2 * s.order) && detect_data_offset() % 16 == 0, "LDS bytes");
    Lds<T> lds((size_t)detect_lds_values(s.order));
    Lds<unsigned> seg(DETECT_SEGMENTS);
    std::vector<unsigned> mine;
    // launch 1: count
    std::vector<int64_t> tile_ws(s.rows * tiles, -1);
    for (size_t b = 0; b < s.rows * tiles; ++b) {
        sim_tile(p, b / tiles, b % tiles, lds, seg, mine);
        tile_ws[b] = (int64_t)detect_tile_total(seg.view());
    }
    // launch 2: scan tiles; workgroup b takes the rows b, b + blocks, ...
    std::vector<int64_t> row_count(s.rows, -1), row_off;
    const unsigned blocks = detect_scan_blocks(s.rows);
    CHECK(blocks >= 1 && blocks <= (unsigned)DETECT_SCAN_CHUNK, "scan blocks");
    for (unsigned b = 0; b < blocks; ++b)
        for (size_t row = b; row < s.rows; row += blocks) {
            std::vector<int64_t> t(tile_ws.begin() + (long)(row * tiles), tile_ws.begin() + (long)((row + 1) * tiles));
            CHECK(row_count[row] == -1, "a row scanned twice");
            row_count[row] = sim_scan(t);
            std::copy(t.begin(), t.end(), tile_ws.begin() + (long)(row * tiles));
        }
    for (size_t r = 0; r < s.rows; ++r) CHECK(row_count[r] == want_count[r], "%s %s: count of row %zu: %lld, serial %lld", s.text.c_str(), Fmt<T>::name(), r,
                                             (long long)row_count[r], (long long)want_count[r]);
    // launch 3: scan rows
    row_off = row_count;
    const int64_t grand = sim_scan(row_off);
    CHECK((uint64_t)grand == total, "%s: total %lld, serial %llu", s.text.c_str(), (long long)grand, (unsigned long long)total);
    // launch 4: write, for several capacities
    const uint64_t caps[] = {total + 5, total, total ? total - 1 : 0, total / 2 + (total > 70 ? 37 : 0)};
    for (uint64_t capacity : caps) {
        if (capacity == 0) continue; // the launch is skipped
        std::vector<int64_t> index(capacity, -1);
        std::vector<U> value(capacity, 0);
        std::vector<int> writes(capacity, 0);
        for (size_t b = 0; b < s.rows * tiles; ++b) {
            const size_t row = b / tiles, tile = b % tiles;
            const uint64_t base = (uint64_t)(row_off[row] + tile_ws[b]);
            if (base >= capacity) continue;
            sim_tile(p, row, tile, lds, seg, mine);
            CheckedLds<T> l = lds.view();
            CheckedLds<unsigned> sg = seg.view();
            for (int k = 0; k < DETECT_PER_LANE; ++k)
                for (int wave = 0; wave < DETECT_THREADS / DETECT_WAVE; ++wave) {
                    uint64_t ballot = 0;
                    for (int lane = 0; lane < DETECT_WAVE; ++lane) ballot |= (uint64_t)((mine[(size_t)(wave * DETECT_WAVE + lane)] >> k) & 1u) << lane;
                    for (int lane = 0; lane < DETECT_WAVE; ++lane) {
                        const int tid = wave * DETECT_WAVE + lane;
                        const bool hit = (mine[(size_t)tid] >> k) & 1u;
                        const int below = detect_lane_rank(ballot, lane);
                        int serial = 0;
                        for (int i = 0; i < lane; ++i) serial += (int)((ballot >> i) & 1u);
                        CHECK(below == serial, "lane rank");
                        ++g_lane_ranks;
                        const uint64_t pos = base + detect_segment_base(sg, detect_segment(tid, k)) + (uint64_t)below;
                        if (hit && pos < capacity) {
                            const int o = detect_cell(tid, k);
                            index[pos] = (int64_t)(tile * (size_t)DETECT_TILE + (size_t)o);
                            value[pos] = bits_of((T)l[detect_slot(o, s.order)]);
                            ++writes[pos];
                            ++g_written;
                        } else if (hit) {
                            CHECK(pos >= capacity, "a detection dropped below the capacity");
                        }
                    }
                }
        }
        const uint64_t listed = total < capacity ? total : capacity;
        for (uint64_t i = 0; i < capacity; ++i) {
            if (i < listed) {
                CHECK(writes[i] == 1, "%s %s capacity %llu: slot %llu written %d times", s.text.c_str(), Fmt<T>::name(), (unsigned long long)capacity,
                      (unsigned long long)i, writes[i]);
                CHECK(index[i] == want_index[i] && value[i] == want_bits[i], "%s %s capacity %llu: slot %llu holds index %lld, serial %lld", s.text.c_str(),
                      Fmt<T>::name(), (unsigned long long)capacity, (unsigned long long)i, (long long)index[i], (long long)want_index[i]);
            } else {
                CHECK(writes[i] == 0, "%s: slot %llu beyond the list written", s.text.c_str(), (unsigned long long)i);
            }
        }
    }
    CHECK(!lds.bad, "%s %s: a value slot outside the allocation or read before it was written", s.text.c_str(), Fmt<T>::name());
    CHECK(!seg.bad, "%s %s: a segment slot outside the allocation or read before it was written", s.text.c_str(), Fmt<T>::name());
    ++g_cases;
}

// several chunks, counts whose sum passes 2^32
static void check_long_prefix()
{
    for (size_t entries : {(size_t)DETECT_SCAN_CHUNK + 3, (size_t)3 * DETECT_SCAN_CHUNK + 7, (size_t)2 * DETECT_SCAN_CHUNK}) {
        std::vector<int64_t> v(entries), want(entries);
        int64_t sum = 0;
        for (size_t i = 0; i < entries; ++i) {
            v[i] = (int64_t)(rnd() % 0x7fffffffull);
            want[i] = sum;
            sum += v[i];
        }
        const int64_t total = sim_scan(v);
        CHECK(sum > (int64_t)1 << 32, "the sum passes 2^32");
        CHECK(total == sum, "long prefix total");
        for (size_t i = 0; i < entries; ++i) CHECK(v[i] == want[i], "long prefix entry %zu", i);
        CHECK(detect_scan_chunks(entries) > 1, "more than one chunk");
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: %s tests/detect_shapes.txt\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<Shape> shapes;
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line);
        Shape s;
        std::string boundary, kind;
        if (!(is >> s.rows >> s.n >> s.order >> boundary >> kind)) { std::printf("FAIL bad line: %s\n", line.c_str()); return 1; }
        s.boundary = boundary == "open" ? DETECT_OPEN : boundary == "wrap" ? DETECT_WRAP : boundary == "nearest" ? DETECT_NEAREST : -1;
        s.neg_inf = kind == "scalar-inf";
        s.kind = kind == "none" ? DETECT_NONE : (kind == "scalar" || s.neg_inf) ? DETECT_SCALAR : kind == "row" ? DETECT_PER_ROW
                 : kind == "profile" ? DETECT_PROFILE : kind == "cell" ? DETECT_PER_CELL : -1;
        if (!detect_args_valid(s.kind, s.boundary) || s.order < 0 || s.order > DETECT_MAX_ORDER || s.rows == 0 || s.n == 0) {
            std::printf("FAIL bad line: %s\n", line.c_str());
            return 1;
        }
        s.text = line;
        shapes.push_back(s);
    }
    for (const Shape& s : shapes) {
        run_line<float>(s);
        run_line<double>(s);
    }
    check_long_prefix();
    std::printf("%zu shape lines (both precisions), %ld cases\n", shapes.size(), g_cases);
    std::printf("detections: %ld writes, each slot below min(total, capacity) exactly once at its serial place, none at or beyond the capacity\n", g_written);
    std::printf("LDS: %ld accesses, all inside the allocation and written before read\n", g_lds_accesses);
    std::printf("boundary index: %ld positions agree with the brute-force walk\n", g_boundary_checks);
    std::printf("ballot and prefix arithmetic: %ld segments, %ld lane ranks agree with the serial count\n", g_segments, g_lane_ranks);
    std::printf("64-bit prefixes: %ld entries scanned, sums past 2^32 over more than one chunk\n", g_scan_entries);
    std::printf("%ld failures\n", g_failures);
    if (g_failures) return 1;
    std::printf("ok\n");
    return 0;
}
