// sim_mat_sym.cpp -- the index maps of mat_sym.hip (basic_dsp_amd/csrc/mat_sym_core.h) on the host, threads as loops.
//
//   mirror: every p = 1 .. 70, rows 1, 2, 3, rot in {0, p / 2}: the kernel's loop (flat index -> position, the source bin
//           of a position, the grid-stride advance) against a direct restatement of scale -> rotate -> mirror; every
//           output element written exactly once, nothing read or written out of bounds
//   crop:   the same for every odd N = 1 .. 139
//   first-bin rule: a table of hand cases
//
// Grids are chosen so that lanes run zero, one and several trips and the stride is smaller than, equal to and larger
// than a row.  g++ -O2 -std=c++17 (optionally -fsanitize=address,undefined) sim_mat_sym.cpp && ./a.out
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_sym_core.h"

using namespace bdsp;

struct Cx {
    double x, y;
};

static int failures = 0;
#define EXPECT(cond, ...)                                                                          \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                          \
    } while (0)

static const unsigned GRIDS[][2] = {{1, 1}, {1, 3}, {2, 4}, {1, 64}, {3, 7}, {5, 256}}; // {blocks, threads per block}

// k_sy_mirror_rows with threads as loops
template <typename IDX>
static void run_mirror(const std::vector<Cx>& in, std::vector<Cx>& out, std::vector<int>& writes, IDX rows, IDX p,
                       IDX rot, double scale, bool scaled, unsigned blocks, unsigned threads, int* flag)
{
    const IDX n = 2 * p - 1, total = rows * n;
    const IDX stride = (IDX)blocks * threads;
    for (unsigned b = 0; b < blocks; ++b)
        for (unsigned t = 0; t < threads; ++t) {
            IDX o = (IDX)b * threads + t;
            if (o >= total) continue;
            SyPos<IDX> at = sy_pos<IDX>(o, n);
            const SyPos<IDX> step = sy_stride<IDX>(stride, n);
            for (; o < total; o += stride) {
                EXPECT(at.row < rows && at.col < n && at.row * n + at.col == o, "position of %zu", (size_t)o);
                bool conj;
                const IDX bin = sy_mirror_bin<IDX>(at.col, p, rot, &conj);
                EXPECT(bin < p, "bin %zu of p %zu", (size_t)bin, (size_t)p);
                Cx z = in[(size_t)(at.row * p + bin)];
                if (scaled) { z.x = z.x * scale; z.y = z.y * scale; }
                if (flag && at.col == 0) {
                    double re1 = 0, im1 = 0;
                    if (p > 1) {
                        bool c1;
                        const IDX b1 = sy_mirror_bin<IDX>((IDX)1, p, rot, &c1);
                        EXPECT(b1 < p && !c1, "bin of h(1)");
                        Cx z1 = in[(size_t)(at.row * p + b1)];
                        if (scaled) { z1.x = z1.x * scale; z1.y = z1.y * scale; }
                        re1 = z1.x;
                        im1 = z1.y;
                    }
                    if (sy_first_bin_fails(z.x, z.y, re1, im1)) *flag |= 1;
                }
                if (conj) z.y = -z.y;
                out[(size_t)o] = z;
                ++writes[(size_t)o];
                sy_advance<IDX>(&at, step, n);
            }
        }
}

template <typename IDX>
static void check_mirror()
{
    for (IDX p = 1; p <= 70; ++p)
        for (IDX rows = 1; rows <= 3; ++rows)
            for (int shifted = 0; shifted < 2; ++shifted) {
                const IDX rot = shifted ? p / 2 : 0, n = 2 * p - 1;
                const double scale = shifted ? 1.0 / (double)p : 1.0;
                std::vector<Cx> in((size_t)(rows * p));
                for (size_t i = 0; i < in.size(); ++i) in[i] = Cx{(double)(3 * i + 1), (double)(7 * i + 2) * (i % 3 ? 1 : -1)};
                for (IDX r = 0; r < rows; ++r) in[(size_t)(r * p + rot)].y = 0; // the first bin after the rotation is real
                // direct restatement: scale, rotate, mirror -- three passes per row
                std::vector<Cx> ref((size_t)(rows * n));
                for (IDX r = 0; r < rows; ++r) {
                    std::vector<Cx> sc((size_t)p), h((size_t)p);
                    for (IDX j = 0; j < p; ++j) {
                        sc[(size_t)j] = in[(size_t)(r * p + j)];
                        if (shifted) { sc[(size_t)j].x = sc[(size_t)j].x * scale; sc[(size_t)j].y = sc[(size_t)j].y * scale; }
                    }
                    for (IDX j = 0; j < p; ++j) h[(size_t)j] = sc[(size_t)((j + rot) % p)];
                    for (IDX g = 0; g < n; ++g)
                        ref[(size_t)(r * n + g)] = g < p ? h[(size_t)g] : Cx{h[(size_t)(2 * p - 1 - g)].x, -h[(size_t)(2 * p - 1 - g)].y};
                }
                for (const auto& gr : GRIDS) {
                    std::vector<Cx> out((size_t)(rows * n), Cx{-1, -1});
                    std::vector<int> writes((size_t)(rows * n), 0);
                    int flag = 0;
                    run_mirror<IDX>(in, out, writes, rows, p, rot, scale, shifted != 0, gr[0], gr[1], &flag);
                    for (size_t i = 0; i < out.size(); ++i) {
                        EXPECT(writes[i] == 1, "mirror p %zu rows %zu rot %zu grid %ux%u: element %zu written %d times",
                               (size_t)p, (size_t)rows, (size_t)rot, gr[0], gr[1], i, writes[i]);
                        EXPECT(out[i].x == ref[i].x && out[i].y == ref[i].y, "mirror p %zu rows %zu rot %zu: element %zu",
                               (size_t)p, (size_t)rows, (size_t)rot, i);
                    }
                    EXPECT(flag == 0, "flag raised on real first bins, p %zu", (size_t)p);
                }
                // one row's first bin made imaginary: the flag rises whichever row it is
                for (IDX bad = 0; bad < rows; ++bad) {
                    std::vector<Cx> in2 = in;
                    in2[(size_t)(bad * p + rot)].y = 1.0e6;
                    std::vector<Cx> out((size_t)(rows * n));
                    std::vector<int> writes((size_t)(rows * n), 0);
                    int flag = 0;
                    run_mirror<IDX>(in2, out, writes, rows, p, rot, scale, shifted != 0, 2, 4, &flag);
                    EXPECT(flag == 1, "flag not raised, p %zu row %zu", (size_t)p, (size_t)bad);
                }
            }
}

template <typename IDX>
static void check_crop()
{
    for (IDX n = 1; n <= 139; n += 2)
        for (IDX rows = 1; rows <= 3; ++rows) {
            const IDX p = n / 2 + 1, total = rows * p;
            std::vector<double> in((size_t)(rows * n));
            for (size_t i = 0; i < in.size(); ++i) in[i] = (double)i + 0.5;
            for (const auto& gr : GRIDS) {
                std::vector<double> out((size_t)total, -1.0);
                std::vector<int> writes((size_t)total, 0);
                const IDX stride = (IDX)gr[0] * gr[1];
                for (unsigned b = 0; b < gr[0]; ++b)
                    for (unsigned t = 0; t < gr[1]; ++t) { // k_sy_crop_rows
                        IDX o = (IDX)b * gr[1] + t;
                        if (o >= total) continue;
                        SyPos<IDX> at = sy_pos<IDX>(o, p);
                        const SyPos<IDX> step = sy_stride<IDX>(stride, p);
                        for (; o < total; o += stride) {
                            const IDX src = sy_crop_src<IDX>(at.row, at.col, n);
                            EXPECT(at.row < rows && at.col < p && src < rows * n, "crop source of %zu", (size_t)o);
                            out[(size_t)o] = in[(size_t)src];
                            ++writes[(size_t)o];
                            sy_advance<IDX>(&at, step, p);
                        }
                    }
                for (IDX r = 0; r < rows; ++r)
                    for (IDX j = 0; j < p; ++j) {
                        const size_t i = (size_t)(r * p + j);
                        EXPECT(writes[i] == 1, "crop n %zu rows %zu: element %zu written %d times", (size_t)n, (size_t)rows, i, writes[i]);
                        EXPECT(out[i] == in[(size_t)(r * n + j)], "crop n %zu rows %zu: element %zu", (size_t)n, (size_t)rows, i);
                    }
            }
        }
}

static void check_predicate()
{
    struct Case { double re0, im0, re1, im1; bool fails; const char* what; };
    const Case cases[] = {
        {5.0, 0.0, 0.0, 0.0, false, "p == 1, real"},
        {5.0, 1.0, 0.0, 0.0, true, "p == 1, im 1 against |re0| 5"},
        {5.0, 4.0e-3, 0.0, 0.0, false, "p == 1, im below 1e-3 * |re0|"},
        {0.0, 1.0e-9, 0.0, 0.0, true, "p == 1, a zero spectrum with im above the absolute bound"},
        {3.0, 0.0, -2.0, 7.0, false, "an exact zero"},
        {3.0, -0.0, -2.0, 7.0, false, "a negative zero"},
        {0.0, 1.0e-11, 0.0, 0.0, false, "1e-11 is below the absolute bound whatever the scale"},
        {0.0, -1.0e-11, 0.0, 0.0, false, "-1e-11"},
        {1000.0, 0.9, 50.0, -50.0, false, "noise 0.9 below 1e-3 * 1100"},
        {1000.0, -1.2, 50.0, -50.0, true, "noise 1.2 above 1e-3 * 1100"},
        {-1000.0, 0.999, 0.0, 0.0, false, "the scale is |re0|, not re0"},
        {1.0e-8, 1.0e-9, 0.0, 0.0, true, "tiny spectrum, im above both bounds"},
        {1.0e-5, 5.0e-10, 0.0, 0.0, false, "im above 1e-10 but below 1e-3 * scale"},
        {2.0, 1.0, 400.0, 600.0, false, "neighbour bin carries the scale"},
    };
    for (const Case& c : cases)
        EXPECT(sy_first_bin_fails(c.re0, c.im0, c.re1, c.im1) == c.fails, "first-bin rule: %s", c.what);
    std::printf("first-bin rule: %zu hand cases\n", sizeof(cases) / sizeof(cases[0]));
}

int main()
{
    check_mirror<unsigned>();
    check_mirror<size_t>();
    std::printf("mirror: p 1..70, rows 1..3, rot 0 and p/2, 32- and 64-bit indices\n");
    check_crop<unsigned>();
    check_crop<size_t>();
    std::printf("crop: odd N 1..139, rows 1..3, 32- and 64-bit indices\n");
    check_predicate();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
