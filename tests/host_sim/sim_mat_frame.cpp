// sim_mat_frame.cpp -- the lane loops and index maps of mat_frame.hip (basic_dsp_amd/csrc/mat_frame_core.h) on the
// host, threads as loops.  The kernels hand their pointers to mf_lane_*; here the same functions get arrays that count
// every write and refuse every read or write out of bounds.
//
//   from_frames   every (P, F, H, pad_tail) with P 0..20, F and H 1..6, plus (1025, 256, 128), (1000, 127, 1),
//                 (70002, 3, 1): both row counts against a brute-force count, every output written exactly once, every
//                 read in bounds or replaced by zero, against x[r * H + j]
//   overlap_add   rows 0..20 (here 1..20: no rows, no launch), F and H 1..6, plus (257, 100, 25), (2, 4097, 4096),
//                 (70000, 3, 1): the first and the last contributing row of every output exact, the sum in ascending
//                 row order against the row loop y[r * H .. r * H + F) += m[r], bit for bit
//   from_vectors  rows 1..5 x points 1..9
//   zero_pad, rotate   row points 1..70, 127..129, 1023..1025, rows 1, 2, 3; End / Surround / Center to one point more,
//                 to 2n and to 2n + 3; rotations by ceil(n / 2) and floor(n / 2): equal to the per-row maps, restated
//                 here on their own (two copied segments over zeros; out[i] = in[(i + shift) mod n])
//   maps only     one extent pair above 2^32: positions, advance and sources with 64-bit indices
//
// Grids are chosen so that lanes run zero, one and several trips and the stride is smaller than, equal to and larger
// than a row.  g++ -O2 -std=c++17 (optionally -fsanitize=address,undefined) sim_mat_frame.cpp && ./a.out
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_frame_core.h"

using namespace bdsp;

static int failures = 0;
#define EXPECT(cond, ...)                                                                          \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                          \
    } while (0)

static const unsigned GRIDS[][2] = {{1, 1}, {1, 3}, {2, 4}, {1, 64}, {3, 7}, {5, 256}}; // {blocks, threads per block}
static const unsigned BIG_GRID[2] = {16, 256};

static unsigned long long reads_out_of_bounds = 0, writes_out_of_bounds = 0;

// an input: reads are checked (an out-of-bounds read is counted and answers a value no test expects)
template <typename P>
struct InArr {
    const std::vector<P>* v;
    P operator[](size_t i) const
    {
        if (i >= v->size()) { ++reads_out_of_bounds; return (P)-12345; }
        return (*v)[i];
    }
};

// an output: writes are checked and counted per element
template <typename P>
struct OutArr {
    std::vector<P>* v;
    std::vector<int>* writes;
    struct Ref {
        OutArr* a;
        size_t i;
        void operator=(P x)
        {
            if (i >= a->v->size()) { ++writes_out_of_bounds; return; }
            (*a->v)[i] = x;
            ++(*a->writes)[i];
        }
    };
    Ref operator[](size_t i) { return Ref{this, i}; }
};

template <typename P>
struct Tab {
    const std::vector<std::vector<P>>* rows;
    InArr<P> operator[](size_t r) const
    {
        if (r >= rows->size()) { ++reads_out_of_bounds; return InArr<P>{&(*rows)[0]}; }
        return InArr<P>{&(*rows)[r]};
    }
};

template <class F>
static void for_each_lane(const unsigned* grid, F f)
{
    const size_t stride = (size_t)grid[0] * grid[1];
    for (unsigned b = 0; b < grid[0]; ++b)
        for (unsigned t = 0; t < grid[1]; ++t) f((size_t)b * grid[1] + t, stride);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void check_written_once(const std::vector<int>& writes, const char* what, size_t a, size_t b, size_t c)
{
    for (size_t i = 0; i < writes.size(); ++i)
        EXPECT(writes[i] == 1, "%s (%zu, %zu, %zu): element %zu written %d times", what, a, b, c, i, writes[i]);
}

// ---------------------------------------------------------------------------------------------
// from_frames
// ---------------------------------------------------------------------------------------------
static size_t brute_rows(size_t P, size_t F, size_t H, bool pad_tail)
{
    size_t rows = 0;
    if (!pad_tail) {
        while (rows * H + F <= P) ++rows; // whole frames
        return rows;
    }
    while (rows == 0 ? P > 0 : (rows - 1) * H + F < P) ++rows; // frames until the last point is covered
    return rows;
}

template <typename IDX>
static void frames_case(size_t P, size_t F, size_t H, bool pad_tail, bool all_grids)
{
    const size_t rows = mf_frame_rows(P, F, H, pad_tail);
    EXPECT(rows == brute_rows(P, F, H, pad_tail), "rows of (%zu, %zu, %zu, %d): %zu", P, F, H, (int)pad_tail, rows);
    if (pad_tail && rows) EXPECT((rows - 1) * H + F >= P && (rows == 1 || (rows - 2) * H + F < P), "tail of (%zu, %zu, %zu)", P, F, H);
    if (rows == 0) return;
    std::vector<double> x(P);
    for (size_t i = 0; i < P; ++i) x[i] = (double)i + 0.25;
    const size_t total = rows * F, h = H < P ? H : P; // as the launcher
    for (const auto& gr : GRIDS) {
        const unsigned* g = all_grids ? gr : BIG_GRID;
        std::vector<double> out(total, -1.0);
        std::vector<int> writes(total, 0);
        for_each_lane(g, [&](size_t first, size_t stride) {
            mf_lane_from_frames<double, IDX>(InArr<double>{&x}, OutArr<double>{&out, &writes}, (IDX)total, (IDX)P, (IDX)F, (IDX)h,
                                             (IDX)first, (IDX)stride);
        });
        check_written_once(writes, "from_frames", P, F, H);
        for (size_t r = 0; r < rows; ++r)
            for (size_t j = 0; j < F; ++j) {
                const size_t src = r * H + j;
                EXPECT(out[r * F + j] == (src < P ? x[src] : 0.0), "from_frames (%zu, %zu, %zu) row %zu point %zu", P, F, H, r, j);
            }
        if (!all_grids) break;
    }
}

// ---------------------------------------------------------------------------------------------
// overlap_add
// ---------------------------------------------------------------------------------------------
template <typename IDX>
static void ola_case(size_t rows, size_t F, size_t H, bool all_grids)
{
    const size_t h = rows == 1 ? F : H, total = mf_ola_points(rows, F, h);
    EXPECT(total == (rows - 1) * h + F, "overlap_add length");
    std::vector<double> m(rows * F);
    // values whose sum depends on the order: 1e16-sized terms next to small ones
    for (size_t i = 0; i < m.size(); ++i) m[i] = (i % 5 == 0 ? 1.0e16 : 1.0) * ((i % 3) ? 1.0 : -1.0) + (double)(i % 7) * 0.37;
    std::vector<double> ref(total, 0.0);
    for (size_t r = 0; r < rows; ++r)
        for (size_t j = 0; j < F; ++j) ref[r * h + j] += m[r * F + j];
    // the first and the last contributing row of every output
    for (size_t i = 0; i < total; ++i) {
        size_t lo = rows, hi = 0;
        // every row; for the 70000-row case the rows around i / h (a row further away starts past i or ends before it)
        const size_t span = F / h + 2, from = rows > 300 && i / h > span ? i / h - span : 0;
        const size_t to = rows > 300 && i / h + 2 < rows ? i / h + 2 : rows;
        for (size_t r = from; r < to; ++r)
            if (i >= r * h && i - r * h < F) { if (lo == rows) lo = r; hi = r; }
        IDX r0, r1;
        mf_ola_rows<IDX>((IDX)(i / h), (IDX)(i % h), (IDX)rows, (IDX)F, (IDX)h, &r0, &r1);
        if (lo == rows) EXPECT(r0 > r1, "overlap_add (%zu, %zu, %zu): output %zu lies in a gap", rows, F, H, i);
        else EXPECT((size_t)r0 == lo && (size_t)r1 == hi, "overlap_add (%zu, %zu, %zu): rows of output %zu: %zu..%zu, expected %zu..%zu",
                    rows, F, H, i, (size_t)r0, (size_t)r1, lo, hi);
    }
    for (const auto& gr : GRIDS) {
        const unsigned* g = all_grids ? gr : BIG_GRID;
        std::vector<double> y(total, -1.0);
        std::vector<int> writes(total, 0);
        for_each_lane(g, [&](size_t first, size_t stride) {
            mf_lane_overlap_add<double, IDX>(InArr<double>{&m}, OutArr<double>{&y, &writes}, (IDX)total, (IDX)rows, (IDX)F, (IDX)h,
                                             (IDX)first, (IDX)stride);
        });
        check_written_once(writes, "overlap_add", rows, F, H);
        for (size_t i = 0; i < total; ++i) EXPECT(same_bits(y[i], ref[i]), "overlap_add (%zu, %zu, %zu): output %zu", rows, F, H, i);
        if (!all_grids) break;
    }
}

// ---------------------------------------------------------------------------------------------
// from_vectors
// ---------------------------------------------------------------------------------------------
template <typename IDX>
static void vectors_case(size_t rows, size_t points)
{
    std::vector<std::vector<double>> vs(rows, std::vector<double>(points));
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < points; ++c) vs[r][c] = (double)(r * 1000 + c);
    const size_t total = rows * points;
    for (const auto& gr : GRIDS) {
        std::vector<double> out(total, -1.0);
        std::vector<int> writes(total, 0);
        for_each_lane(gr, [&](size_t first, size_t stride) {
            mf_lane_from_vectors<double, IDX>(Tab<double>{&vs}, OutArr<double>{&out, &writes}, (IDX)total, (IDX)points, (IDX)first,
                                              (IDX)stride);
        });
        check_written_once(writes, "from_vectors", rows, points, 0);
        for (size_t i = 0; i < total; ++i) EXPECT(out[i] == vs[i / points][i % points], "from_vectors %zu x %zu: element %zu", rows, points, i);
    }
}

// ---------------------------------------------------------------------------------------------
// zero_pad and rotate against the per-row maps, restated without the core header
// ---------------------------------------------------------------------------------------------
// zero_pad's two segments (End, Surround: right = diff / 2, Center) and the copy rule, restated
static void ref_zero_pad_row(const double* in, double* out, size_t pb, size_t points, int option)
{
    size_t d0 = 0, s0 = 0, n0 = pb, d1 = 0, s1 = 0, n1 = 0;
    if (option == 1) {
        size_t diff = points - pb, right = diff / 2;
        d0 = diff - right;
    } else if (option != 0) {
        size_t right = pb / 2, left = pb - pb / 2;
        n0 = left;
        d1 = points - right; s1 = pb - right; n1 = right;
    }
    for (size_t g = 0; g < points; ++g) {
        double v = 0.0;
        if (g >= d0 && g - d0 < n0) v = in[s0 + (g - d0)];
        else if (g >= d1 && g - d1 < n1) v = in[s1 + (g - d1)];
        out[g] = v;
    }
}

template <typename IDX>
static void moves_case(size_t rows, size_t n, const unsigned* g)
{
    std::vector<double> in(rows * n);
    for (size_t i = 0; i < in.size(); ++i) in[i] = (double)i + 1.0;
    const size_t targets[3] = {n + 1, 2 * n, 2 * n + 3};
    for (size_t points : targets)
        for (int option = 0; option < 3; ++option) {
            const size_t total = rows * points;
            std::vector<double> ref(total), out(total, -1.0);
            std::vector<int> writes(total, 0);
            for (size_t r = 0; r < rows; ++r) ref_zero_pad_row(&in[r * n], &ref[r * points], n, points, option);
            size_t d0, n0, d1, s1, n1;
            mf_pad_geom(n, points, option, &d0, &n0, &d1, &s1, &n1);
            const MfPad<IDX> pad{(IDX)d0, (IDX)n0, (IDX)d1, (IDX)s1, (IDX)n1};
            for_each_lane(g, [&](size_t first, size_t stride) {
                mf_lane_zero_pad<double, IDX>(InArr<double>{&in}, OutArr<double>{&out, &writes}, (IDX)total, (IDX)n, (IDX)points, pad,
                                              (IDX)first, (IDX)stride);
            });
            check_written_once(writes, "zero_pad", rows, n, points);
            for (size_t i = 0; i < total; ++i) EXPECT(out[i] == ref[i], "zero_pad %zu x %zu -> %zu option %d: element %zu", rows, n, points, option, i);
        }
    const size_t shifts[2] = {n - n / 2, n / 2};
    for (size_t shift : shifts) {
        const size_t total = rows * n, sh = shift % n;
        std::vector<double> out(total, -1.0);
        std::vector<int> writes(total, 0);
        for_each_lane(g, [&](size_t first, size_t stride) {
            mf_lane_rotate<double, IDX>(InArr<double>{&in}, OutArr<double>{&out, &writes}, (IDX)total, (IDX)n, (IDX)sh, (IDX)first, (IDX)stride);
        });
        check_written_once(writes, "rotate", rows, n, shift);
        for (size_t r = 0; r < rows; ++r)
            for (size_t i = 0; i < n; ++i) { // the rotation of row r
                size_t src = i + sh;
                if (src >= n) src -= n;
                EXPECT(out[r * n + i] == in[r * n + src], "rotate %zu x %zu by %zu: row %zu point %zu", rows, n, shift, r, i);
            }
    }
}

template <typename IDX>
static void check_all()
{
    for (size_t P = 0; P <= 20; ++P)
        for (size_t F = 1; F <= 6; ++F)
            for (size_t H = 1; H <= 6; ++H)
                for (int pad = 0; pad < 2; ++pad) frames_case<IDX>(P, F, H, pad != 0, true);
    const size_t big_frames[][3] = {{1025, 256, 128}, {1000, 127, 1}, {70002, 3, 1}};
    for (const auto& c : big_frames)
        for (int pad = 0; pad < 2; ++pad) frames_case<IDX>(c[0], c[1], c[2], pad != 0, false);
    // a hop past the end of the signal (the launcher clamps it)
    frames_case<IDX>(10, 4, 1000, true, true);
    frames_case<IDX>(10, 4, 1000, false, true);

    for (size_t rows = 1; rows <= 20; ++rows)
        for (size_t F = 1; F <= 6; ++F)
            for (size_t H = 1; H <= 6; ++H) ola_case<IDX>(rows, F, H, true);
    const size_t big_ola[][3] = {{257, 100, 25}, {2, 4097, 4096}, {70000, 3, 1}};
    for (const auto& c : big_ola) ola_case<IDX>(c[0], c[1], c[2], false);

    for (size_t rows = 1; rows <= 5; ++rows)
        for (size_t points = 1; points <= 9; ++points) vectors_case<IDX>(rows, points);

    std::vector<size_t> ns;
    for (size_t n = 1; n <= 70; ++n) ns.push_back(n);
    for (size_t n : {127, 128, 129, 1023, 1024, 1025}) ns.push_back(n);
    for (size_t n : ns)
        for (size_t rows = 1; rows <= 3; ++rows) {
            if (n <= 70) { for (const auto& gr : GRIDS) moves_case<IDX>(rows, n, gr); }
            else { moves_case<IDX>(rows, n, GRIDS[4]); moves_case<IDX>(rows, n, GRIDS[5]); }
        }
}

// maps only: extents above 2^32 with 64-bit indices -- the position of a flat index, the advance by a grid stride and the
// sources, at the first and the last elements and at a row boundary in between
static void check_large()
{
    const size_t rows = 70000, width = 70002, total = rows * width; // > 2^32
    const size_t stride = (size_t)1024 * 256;
    const size_t starts[] = {0, 1, width - 1, width, (size_t(1) << 32) - 3, (size_t(1) << 32) + 5, total - stride - 1, total - 2 * stride};
    for (size_t o : starts) {
        MfPos<size_t> at = mf_pos<size_t>(o, width);
        const MfPos<size_t> step = mf_pos<size_t>(stride, width);
        for (int trip = 0; trip < 3 && o < total; ++trip, o += stride) {
            EXPECT(at.row == o / width && at.col == o % width, "position of %zu", o);
            EXPECT(mf_frame_src<size_t>(at.row, at.col, 3) == at.row * 3 + at.col, "frame source of %zu", o);
            EXPECT((o - at.col) + mf_rotate_src<size_t>(at.col, width, width / 2) == at.row * width + (at.col + width / 2) % width,
                   "rotate source of %zu", o);
            mf_advance<size_t>(&at, step, width);
        }
    }
    // overlap_add: outputs past 2^32 of 2^31 rows of 5 points, 3 apart
    const size_t R = size_t(1) << 31, F = 5, H = 3;
    const size_t outs[] = {(size_t(1) << 32) + 1, (R - 1) * H, (R - 1) * H + F - 1};
    for (size_t i : outs) {
        size_t lo = R, hi = 0;
        for (size_t r = i / H >= 4 ? i / H - 4 : 0; r <= i / H && r < R; ++r)
            if (i - r * H < F) { if (lo == R) lo = r; hi = r; }
        size_t r0, r1;
        mf_ola_rows<size_t>(i / H, i % H, R, F, H, &r0, &r1);
        EXPECT(r0 == lo && r1 == hi, "overlap_add rows of output %zu", i);
    }
    EXPECT(mf_frame_rows((size_t(1) << 33) + 1, 1024, 256, false) == ((size_t(1) << 33) + 1 - 1024) / 256 + 1, "rows above 2^32");
    EXPECT(mf_frame_rows((size_t(1) << 33) + 1, 1024, 256, true) == ((size_t(1) << 33) + 1 - 1024) / 256 + 2, "padded rows above 2^32");
    EXPECT(!mf_fits_32(total, 0) && !mf_fits_32(5, size_t(1) << 31) && mf_fits_32((size_t(1) << 31) - 1, 7), "index width");
    std::printf("maps only: %zu x %zu > 2^32, overlap_add of 2^31 rows\n", rows, width);
}

int main()
{
    check_all<unsigned>();
    check_all<size_t>();
    std::printf("from_frames: P 0..20 x F 1..6 x H 1..6 x pad_tail 0 1, (1025, 256, 128) (1000, 127, 1) (70002, 3, 1)\n");
    std::printf("overlap_add: rows 1..20 x F 1..6 x H 1..6, (257, 100, 25) (2, 4097, 4096) (70000, 3, 1)\n");
    std::printf("from_vectors: rows 1..5 x points 1..9\n");
    std::printf("zero_pad, rotate: row points 1..70 127 128 129 1023 1024 1025 x rows 1 2 3, End Surround Center\n");
    std::printf("32- and 64-bit indices\n");
    check_large();
    EXPECT(mf_ola_points(0, 5, 3) == 0 && mf_ola_points(1, 5, 3) == 5 && mf_ola_points(4, 5, 3) == 14, "overlap_add length");
    EXPECT(reads_out_of_bounds == 0, "%llu reads out of bounds", reads_out_of_bounds);
    EXPECT(writes_out_of_bounds == 0, "%llu writes out of bounds", writes_out_of_bounds);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
