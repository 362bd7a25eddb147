// sim_mat_ew.cpp -- the maps of mat_ew.hip (basic_dsp_amd/csrc/mat_ew_core.h) on the host, threads as loops.
//
// Runs the loops of k_mw_cexp, k_mw_reverse and k_mw_smaller over the maps the kernels use, with the grids the
// launchers pick (a device of 256 compute units, and a tiny grid that makes every lane take many strides), and checks:
// every element is written exactly once, every read is in bounds, the phasor index of the mixer is the position in the
// row, the source of reverse is r * points + points - 1 - i, and the operand index of *_smaller is
// r * stride + (i mod ypoints).  One rows x points pair above 2^32 elements runs the maps alone, without data.
//
//   g++ -O2 -std=c++17 -o sim_mat_ew sim_mat_ew.cpp && ./sim_mat_ew        (prints OK)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_ew_core.h"

using namespace bdsp;
typedef unsigned long long u64;

static long long g_checks = 0;
#define CHECK(c, ...)                                                                      \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
    } while (0)

// ------------------------------------------------------------------------------------------- k_mw_cexp
// the launcher's grid: tiles_per_row x gy
static u64 cexp_gy(const MwCexpGeom& g, u64 cap)
{
    u64 gy = cap / g.tiles_per_row;
    if (gy > g.row_groups) gy = g.row_groups;
    if (gy > 65535) gy = 65535;
    return gy ? gy : 1;
}

static void sim_cexp(u64 rows, u64 points, u64 cap)
{
    const MwCexpGeom g = mw_cexp_geom(rows, points);
    const u64 gy = cexp_gy(g, cap), total = rows * points;
    std::vector<uint8_t> hits(total, 0);
    for (u64 bx = 0; bx < g.tiles_per_row; ++bx)
        for (u64 by = 0; by < gy; ++by)
            for (unsigned lane = 0; lane < MW_WG; ++lane) {
                unsigned sub;
                u64 k;
                if (!mw_cexp_lane(g, bx, lane, &sub, &k)) continue;
                CHECK(k < points, "cexp %llu x %llu: k %llu", rows, points, k);
                for (u64 rg = by; rg < g.row_groups; rg += 4 * gy)
                    for (int u = 0; u < 4; ++u) {
                        const u64 row = mw_cexp_row(g, rg + u * gy, sub);
                        if (!(row < g.rows)) continue;
                        const u64 at = row * g.points + k;
                        CHECK(at < total, "cexp %llu x %llu: element %llu out of bounds", rows, points, at);
                        CHECK(at % points == k, "cexp %llu x %llu: phasor index %llu at element %llu", rows, points, k, at);
                        CHECK(hits[at] == 0, "cexp %llu x %llu: element %llu written twice", rows, points, at);
                        hits[at] = 1;
                    }
            }
    for (u64 e = 0; e < total; ++e) CHECK(hits[e] == 1, "cexp %llu x %llu: element %llu not written", rows, points, e);
}

// ------------------------------------------------------------------------------------------- k_mw_reverse / k_mw_smaller
static unsigned flat_grid(u64 total, u64 cap)
{
    u64 blocks = (total + 255) / 256;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks ? blocks : 1);
}

template <typename IDX>
static void sim_reverse(u64 rows, u64 points, u64 cap)
{
    const u64 total64 = rows * points;
    const unsigned grid = flat_grid(total64, cap);
    const IDX total = (IDX)total64, stride = (IDX)grid * 256, s_i = (IDX)(((u64)grid * 256) % points);
    std::vector<uint8_t> hits(total64, 0);
    for (unsigned b = 0; b < grid; ++b)
        for (unsigned lane = 0; lane < 256; ++lane) {
            IDX o = (IDX)b * 256 + lane;
            if (o >= total) continue;
            IDX r, i;
            mw_flat_start<IDX>(o, (IDX)points, &r, &i);
            for (; o < total; o += stride) {
                const IDX src = mw_reverse_src<IDX>(o, (IDX)points, i);
                const u64 row = (u64)o / points, pos = (u64)o % points;
                CHECK((u64)src < total64, "reverse %llu x %llu: read %llu out of bounds", rows, points, (u64)src);
                CHECK((u64)src == row * points + (points - 1 - pos), "reverse %llu x %llu: element %llu reads %llu", rows, points, (u64)o, (u64)src);
                CHECK(hits[o] == 0, "reverse %llu x %llu: element %llu written twice", rows, points, (u64)o);
                hits[o] = 1;
                mw_flat_step<IDX>((IDX)points, 0, s_i, &r, &i);
            }
        }
    for (u64 e = 0; e < total64; ++e) CHECK(hits[e] == 1, "reverse %llu x %llu: element %llu not written", rows, points, e);
}

// ystride == ypoints: a matrix operand; 0: one vector for every row
template <typename IDX>
static void sim_smaller(u64 rows, u64 points, u64 ypoints, u64 ystride, u64 cap)
{
    const u64 total64 = rows * points, ytotal = ystride ? rows * ystride : ypoints;
    const unsigned grid = flat_grid(total64, cap);
    const u64 stride64 = (u64)grid * 256;
    const IDX total = (IDX)total64, stride = (IDX)stride64, s_r = (IDX)(stride64 / points), s_i = (IDX)(stride64 % points),
              s_j = (IDX)(stride64 % ypoints);
    std::vector<uint8_t> hits(total64, 0);
    for (unsigned b = 0; b < grid; ++b)
        for (unsigned lane = 0; lane < 256; ++lane) {
            IDX o = (IDX)b * 256 + lane;
            if (o >= total) continue;
            IDX r, i;
            mw_flat_start<IDX>(o, (IDX)points, &r, &i);
            IDX j = i % (IDX)ypoints;
            for (; o < total; o += stride) {
                const IDX q = mw_operand_index<IDX>(r, (IDX)ystride, j);
                const u64 row = (u64)o / points, pos = (u64)o % points;
                CHECK((u64)q < ytotal, "smaller %llu x %llu / %llu: operand read %llu out of bounds", rows, points, ypoints, (u64)q);
                CHECK((u64)q == row * ystride + pos % ypoints, "smaller %llu x %llu / %llu (stride %llu): element %llu reads %llu",
                      rows, points, ypoints, ystride, (u64)o, (u64)q);
                CHECK(hits[o] == 0, "smaller %llu x %llu: element %llu written twice", rows, points, (u64)o);
                hits[o] = 1;
                mw_flat_step<IDX>((IDX)points, s_r, s_i, &r, &i);
                j = mw_period_step<IDX>(j, s_j, (IDX)ypoints);
            }
        }
    for (u64 e = 0; e < total64; ++e) CHECK(hits[e] == 1, "smaller %llu x %llu: element %llu not written", rows, points, e);
}

static void sim_shape(u64 rows, u64 points, u64 cap)
{
    sim_cexp(rows, points, cap);
    // the launchers take 32-bit indices whenever mw_fits_32 allows
    CHECK(mw_fits_32(rows * points, rows * points), "%llu x %llu should fit 32-bit indices", rows, points);
    sim_reverse<unsigned>(rows, points, cap);
    sim_reverse<size_t>(rows, points, cap);
    u64 mid = 1; // a divisor of points strictly between 1 and points, if there is one
    for (u64 d = 2; d * d <= points; ++d)
        if (points % d == 0) mid = points / d;
    const u64 periods[3] = {1, mid, points};
    for (u64 yp : periods) {
        sim_smaller<unsigned>(rows, points, yp, yp, cap);
        sim_smaller<unsigned>(rows, points, yp, 0, cap);
        sim_smaller<size_t>(rows, points, yp, yp, cap);
        sim_smaller<size_t>(rows, points, yp, 0, cap);
    }
}

// rows x points above 2^32 elements: the maps alone, on sampled lanes and strides
static void sim_huge()
{
    const u64 rows = 70000, points = 70002, total = rows * points, yp = 18; // 70002 = 2 * 3 * 3 * 3889
    CHECK(total > (1ull << 32), "pair not above 2^32");
    CHECK(points % yp == 0, "period does not divide the row");
    CHECK(!mw_fits_32(total, 0), "a pair above 2^32 must take 64-bit indices");
    const u64 cap = 2048, stride = cap * 256, s_r = stride / points, s_i = stride % points, s_j = stride % yp;
    const u64 starts[] = {0, 1, 255, 256, 70001, 70002, stride - 1, stride / 2 + 12345};
    u64 last = 0;
    for (u64 o0 : starts) {
        size_t o = o0, r, i;
        mw_flat_start<size_t>(o, points, &r, &i);
        size_t j = i % yp;
        for (; o < total; o += stride) {
            CHECK(r == o / points && i == o % points, "huge: element %llu -> row %llu position %llu", (u64)o, (u64)r, (u64)i);
            CHECK(j == (o % points) % yp, "huge: element %llu period position %llu", (u64)o, (u64)j);
            const size_t src = mw_reverse_src<size_t>(o, points, i);
            CHECK(src == r * points + (points - 1 - i) && src < total, "huge: reverse source of %llu", (u64)o);
            CHECK(mw_operand_index<size_t>(r, yp, j) == r * yp + j && r * yp + j < rows * yp, "huge: operand of %llu", (u64)o);
            last = o;
            mw_flat_step<size_t>(points, s_r, s_i, &r, &i);
            j = mw_period_step<size_t>(j, s_j, yp);
        }
    }
    CHECK(last > (1ull << 32), "huge: the walk did not pass 2^32");
    // the mixer: 274 tiles per row; the last lane with a point of the last row sits above 2^32 and inside the matrix
    const MwCexpGeom g = mw_cexp_geom(rows, points);
    CHECK(g.tiles_per_row == (points + 255) / 256 && g.rps == 1 && g.row_groups == rows, "huge: mixer geometry");
    const u64 gy = cexp_gy(g, cap);
    u64 seen_rows = 0, top = 0;
    for (u64 bx : {0ull, 1ull, g.tiles_per_row - 1})
        for (unsigned lane : {0u, 1u, 112u, 113u, 255u}) {
            unsigned sub;
            u64 k;
            const bool has = mw_cexp_lane(g, bx, lane, &sub, &k);
            CHECK(has == (bx * 256 + lane < points), "huge: mixer lane %u of tile %llu", lane, bx);
            if (!has) continue;
            CHECK(k == bx * 256 + lane && sub == 0, "huge: mixer position");
            for (u64 by : {0ull, gy - 1})
                for (u64 rg = by; rg < g.row_groups; rg += 4 * gy)
                    for (int u = 0; u < 4; ++u) {
                        const u64 row = mw_cexp_row(g, rg + u * gy, sub);
                        if (!(row < g.rows)) continue;
                        const u64 at = row * g.points + k;
                        CHECK(at < total && at % points == k, "huge: mixer element %llu", at);
                        if (at > top) top = at;
                        ++seen_rows;
                    }
        }
    CHECK(top > (1ull << 32) && seen_rows > 0, "huge: the mixer did not pass 2^32");
    std::printf("maps only: 70000 x 70002 > 2^32 (64-bit indices, period %llu)\n", yp);
}

int main()
{
    std::vector<u64> pts;
    for (u64 p = 1; p <= 70; ++p) pts.push_back(p);
    for (u64 p : {127, 128, 129, 255, 256, 257, 1023, 1024, 1025}) pts.push_back(p);
    const u64 rows_of[] = {1, 2, 3, 257};
    for (u64 p : pts)
        for (u64 r : rows_of) {
            sim_shape(r, p, 2048); // the grid of a 256-CU device
            sim_shape(r, p, 3);    // three workgroups: every lane strides many times
        }
    std::printf("shapes: points 1..70 127 128 129 255 256 257 1023 1024 1025 x rows 1 2 3 257\n");
    sim_shape(70000, 3, 2048);
    sim_shape(70000, 3, 3);
    std::printf("shape: 70000 x 3 (85 rows side by side in a workgroup)\n");
    CHECK(mw_cexp_geom(70000, 3).rps == 85 && mw_cexp_geom(5, 255).rps == 1 && mw_cexp_geom(5, 256).tiles_per_row == 1 &&
          mw_cexp_geom(5, 257).tiles_per_row == 2 && mw_cexp_geom(9, 128).rps == 2, "mixer geometry");
    sim_huge();
    std::printf("%lld checks\nOK\n", g_checks);
    return 0;
}
