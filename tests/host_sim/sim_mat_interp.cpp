// sim_mat_interp.cpp -- the maps of mat_interp.hip (basic_dsp_amd/csrc/mat_interp_core.h) on the host, threads as loops.
//
//   conv:   k_mt_conv_direct's loop -- virtual block -> rows / tile, staging of the tile(s) with their circular halos
//           and of the weights into an LDS image, the accumulation over ascending k -- for points 1 .. 70, 255, 256, 257,
//           1023, 1024, 1025, rows 1, 2, 3, L in {0, 1, points / 2, points, 3 * points (clipped)}, real and complex rows,
//           real and complex weights, a budget that stages everything and budgets that force the one-output-per-lane
//           tiling and the unstaged variant: every output written exactly once, every LDS slot that is read lies inside
//           the allocation and was staged by this virtual block, every global read lies inside its row, results equal
//           to the plain double loop of y[i] = sum_k x[(i - L + k) mod N] w[k]
//   interp: the flat index -> (row, position) map of the batched interpolation kernels in 32 and 64 bits, including a
//           rows x dest_len pair whose product exceeds 2^32; the kernels' loop against the per-row loop of the vector
//           kernels for small shapes
//
// g++ -O2 -std=c++17 (optionally -fsanitize=address,undefined) sim_mat_interp.cpp && ./a.out
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../basic_dsp_amd/csrc/mat_interp_core.h"

using namespace bdsp;

static int failures = 0;
#define EXPECT(cond, ...)                                                                          \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                          \
    } while (0)

// ------------------------------------------------------------------------------------------------ convolution
struct ConvCase {
    size_t rows, n, l;
    bool cplx, cw;
};

// k_mt_conv_direct with threads as loops; `grid` workgroups of MT_WG lanes
static void run_conv(const ConvCase& c, const MtConvGeom& g, unsigned grid, const std::vector<double>& in,
                     const std::vector<double>& taps, std::vector<double>& out, std::vector<int>& writes)
{
    const unsigned E = c.cplx ? 2 : 1, WE = c.cw ? 2 : 1;
    const unsigned n = (unsigned)g.n, ntaps = 2 * (unsigned)g.l + 1;
    const size_t row_len = (size_t)g.n * E;
    const size_t lds_scalars = g.lds_bytes / sizeof(double);
    for (unsigned b = 0; b < grid; ++b) {
        std::vector<double> lds(lds_scalars, 0.0);
        std::vector<long long> epoch(lds_scalars, -1); // the virtual block that staged a slot
        double* xs = lds.data();
        double* ws = xs + g.x_scalars;
        if (g.staged) {
            EXPECT((size_t)g.x_scalars + (size_t)ntaps * WE == lds_scalars && g.x_scalars % 2 == 0, "LDS layout");
            for (unsigned t = 0; t < MT_WG; ++t)
                for (unsigned q = t; q < ntaps * WE; q += MT_WG) {
                    EXPECT(g.x_scalars + q < lds_scalars && q < taps.size(), "weight slot %u", q);
                    ws[q] = taps[q];
                    epoch[g.x_scalars + q] = 1ll << 62;
                }
        }
        for (unsigned long long vb = b; vb < g.nblocks; vb += grid) {
            unsigned long long row0;
            unsigned start, cnt;
            mt_conv_block(g, vb, &row0, &start, &cnt);
            EXPECT(row0 < g.rows && start < g.n && cnt >= 1 && (unsigned long long)start + cnt <= g.n, "block %llu", vb);
            const unsigned nseg = mt_conv_segments(g, row0);
            EXPECT(nseg >= 1 && nseg <= g.rpb && row0 + nseg <= g.rows, "segments of block %llu", vb);
            if (g.staged) {
                const unsigned first = mt_conv_first_src(g, start);
                EXPECT(first < n && (first + g.l) % g.n == start % g.n, "first source of block %llu", vb);
                const unsigned span = (cnt + ntaps - 1) * E;
                for (unsigned t = 0; t < MT_WG; ++t) // phase 1: staging
                    for (unsigned sg = 0; sg < nseg; ++sg)
                        for (unsigned q = t; q < span; q += MT_WG) {
                            const unsigned j = c.cplx ? q >> 1 : q;
                            const size_t src = (size_t)mt_conv_src(first, j, n) * E + (c.cplx ? (q & 1) : 0);
                            const size_t dst = (size_t)sg * g.seg_stride * E + q;
                            EXPECT(src < row_len, "staging reads scalar %zu of a row of %zu", src, row_len);
                            EXPECT(dst < g.x_scalars, "staging writes LDS scalar %zu of %u", dst, g.x_scalars);
                            if (src < row_len && dst < g.x_scalars) {
                                xs[dst] = in[(size_t)(row0 + sg) * row_len + src];
                                epoch[dst] = (long long)vb;
                            }
                        }
                for (unsigned t = 0; t < MT_WG; ++t) // phase 2: after the barrier
                    for (unsigned u = 0; u < g.per; ++u) {
                        unsigned sg, i;
                        if (!mt_conv_out(g, t + MT_WG * u, nseg, cnt, &sg, &i)) continue;
                        const unsigned at = sg * g.seg_stride + i;
                        double sre = 0, sim = 0;
                        for (unsigned k = 0; k < ntaps; ++k) {
                            const size_t xa = (size_t)(at + k) * E, wa = (size_t)g.x_scalars + (size_t)k * WE;
                            const bool ok = xa + E <= g.x_scalars && wa + WE <= lds_scalars;
                            EXPECT(ok, "LDS read at element %u + %u", at, k);
                            if (!ok) continue;
                            EXPECT(epoch[xa] == (long long)vb && epoch[xa + E - 1] == (long long)vb,
                                   "LDS element %u + %u was not staged by block %llu", at, k, vb);
                            const double w = ws[(size_t)k * WE], wi = c.cw ? ws[2 * k + 1] : 0.0;
                            const double xr = xs[xa], xi = c.cplx ? xs[xa + 1] : 0.0;
                            if (c.cw) { sre = sre + (xr * w - xi * wi); sim = sim + (xr * wi + xi * w); }
                            else { sre = sre + xr * w; sim = sim + xi * w; }
                        }
                        const size_t o = (size_t)(row0 + sg) * row_len + (size_t)(start + i) * E;
                        EXPECT(o + E <= out.size(), "output scalar %zu", o);
                        if (o + E > out.size()) continue;
                        out[o] = sre; ++writes[o];
                        if (c.cplx) { out[o + 1] = sim; ++writes[o + 1]; }
                    }
            } else {
                for (unsigned t = 0; t < MT_WG; ++t) {
                    unsigned sg, i;
                    if (!mt_conv_out(g, t, nseg, cnt, &sg, &i)) continue;
                    const long long points = (long long)g.n, L = (long long)g.l;
                    const size_t base = (size_t)(row0 + sg) * row_len;
                    const long long o = (long long)start + i;
                    long long p = (o - L) % points;
                    if (p < 0) p += points;
                    double sre = 0, sim = 0;
                    for (long long k = 0; k <= 2 * L; ++k) {
                        EXPECT(p >= 0 && p < points && (size_t)(k * WE + WE) <= taps.size(), "unstaged read %lld", p);
                        const double w = taps[(size_t)k * WE], wi = c.cw ? taps[2 * k + 1] : 0.0;
                        const double xr = in[base + (size_t)p * E], xi = c.cplx ? in[base + 2 * p + 1] : 0.0;
                        if (c.cw) { sre = sre + (xr * w - xi * wi); sim = sim + (xr * wi + xi * w); }
                        else { sre = sre + xr * w; sim = sim + xi * w; }
                        if (++p == points) p = 0;
                    }
                    const size_t oo = base + (size_t)o * E;
                    EXPECT(oo + E <= out.size(), "output scalar %zu", oo);
                    if (oo + E > out.size()) continue;
                    out[oo] = sre; ++writes[oo];
                    if (c.cplx) { out[oo + 1] = sim; ++writes[oo + 1]; }
                }
            }
        }
    }
}

static size_t conv_cases = 0, staged4 = 0, staged1 = 0, unstaged = 0;

static void check_conv_case(const ConvCase& c, size_t budget, unsigned grid)
{
    const unsigned E = c.cplx ? 2 : 1, WE = c.cw ? 2 : 1;
    const size_t ntaps = 2 * c.l + 1;
    std::vector<double> in(c.rows * c.n * E), taps(ntaps * WE);
    // small integers: every product and sum is exact in double, so the order of the sums cannot hide an index error
    for (size_t i = 0; i < in.size(); ++i) in[i] = (double)((i * 7 + 3) % 23) - 11.0;
    for (size_t i = 0; i < taps.size(); ++i) taps[i] = (double)((i * 5 + 1) % 13) - 6.0;
    const MtConvGeom g = mt_conv_geom(c.rows, c.n, c.l, E, WE, sizeof(double), budget);
    EXPECT(g.lds_bytes <= budget, "LDS bytes %zu above the budget %zu", g.lds_bytes, budget);
    EXPECT(g.tile >= 1 && g.rpb >= 1 && (size_t)g.rpb * g.tile <= (size_t)MT_WG * g.per, "tile %u x %u rows, %u per lane",
           g.tile, g.rpb, g.per);
    EXPECT(!g.staged || g.seg_stride == g.tile + 2 * c.l, "segment stride");
    if (!g.staged) ++unstaged; else if (g.per == 4) ++staged4; else ++staged1;
    std::vector<double> out(in.size(), -12345.0);
    std::vector<int> writes(in.size(), 0);
    run_conv(c, g, grid, in, taps, out, writes);
    for (size_t r = 0; r < c.rows; ++r)
        for (size_t i = 0; i < c.n; ++i) {
            double sre = 0, sim = 0;
            for (size_t k = 0; k < ntaps; ++k) {
                const long long m = ((long long)i - (long long)c.l + (long long)k) % (long long)c.n;
                const size_t p = (size_t)(m < 0 ? m + (long long)c.n : m);
                const double xr = in[(r * c.n + p) * E], xi = c.cplx ? in[(r * c.n + p) * E + 1] : 0.0;
                const double w = taps[k * WE], wi = c.cw ? taps[2 * k + 1] : 0.0;
                if (c.cw) { sre += xr * w - xi * wi; sim += xr * wi + xi * w; }
                else { sre += xr * w; sim += xi * w; }
            }
            const size_t o = (r * c.n + i) * E;
            EXPECT(writes[o] == 1 && (!c.cplx || writes[o + 1] == 1), "n %zu rows %zu L %zu: output (%zu, %zu) written %d times",
                   c.n, c.rows, c.l, r, i, writes[o]);
            EXPECT(out[o] == sre && (!c.cplx || out[o + 1] == sim), "n %zu rows %zu L %zu cplx %d cw %d staged %d: output (%zu, %zu)",
                   c.n, c.rows, c.l, (int)c.cplx, (int)c.cw, (int)g.staged, r, i);
        }
    ++conv_cases;
}

static void check_conv()
{
    std::vector<size_t> points;
    for (size_t n = 1; n <= 70; ++n) points.push_back(n);
    for (size_t n : {255, 256, 257, 1023, 1024, 1025}) points.push_back(n);
    // everything staged (the kernel's 64 KB: double scalars here, the largest window of the list is above it and falls
    // back by itself); 20 KB: the four-output tiling no longer fits where L is large; 0: nothing fits
    const size_t budgets[] = {64 * 1024, 20 * 1024, 0};
    const unsigned grids[] = {1, 2, 7};
    for (size_t n : points)
        for (size_t rows = 1; rows <= 3; ++rows) {
            const size_t ls[] = {0, 1, n / 2, n, 3 * n};
            for (size_t lraw : ls) {
                const size_t l = lraw > n ? n : lraw; // the host clips L to the row's points
                for (int kind = 0; kind < 3; ++kind) {
                    const ConvCase c{rows, n, l, kind > 0, kind == 2};
                    for (size_t b = 0; b < 3; ++b) {
                        if (n > 70 && l > 1 && (kind == 1 || b == 2) && n != 257) continue; // the long double loops once per path
                        check_conv_case(c, budgets[b], grids[(n + rows + b) % 3]);
                    }
                }
            }
        }
    // rows above one workgroup's share: 70 rows of 3 points (85 rows per virtual block) and 600 rows of 1 point
    check_conv_case(ConvCase{70, 3, 1, true, false}, 64 * 1024, 2);
    check_conv_case(ConvCase{600, 1, 1, false, false}, 64 * 1024, 2);
    EXPECT(staged4 > 0 && staged1 > 0 && unstaged > 0, "a variant was never taken: %zu %zu %zu", staged4, staged1, unstaged);
    std::printf("conv: points 1..70 255 256 257 1023 1024 1025, rows 1..3, L 0 1 n/2 n 3n: %zu cases (%zu four-output, %zu "
                "one-output, %zu unstaged)\n", conv_cases, staged4, staged1, unstaged);
}

// ------------------------------------------------------------------------------------------------ interpolation
template <typename IDX>
static void check_flat_small()
{
    const unsigned grids[][2] = {{1, 1}, {1, 3}, {2, 4}, {3, 7}, {5, 256}};
    for (IDX dest_len = 1; dest_len <= 40; ++dest_len)
        for (IDX rows = 1; rows <= 3; ++rows)
            for (const auto& gr : grids) {
                const IDX total = rows * dest_len, stride = (IDX)gr[0] * gr[1];
                std::vector<int> writes((size_t)total, 0);
                for (unsigned b = 0; b < gr[0]; ++b)
                    for (unsigned t = 0; t < gr[1]; ++t)
                        for (IDX o = (IDX)b * gr[1] + t; o < total; o += stride) {
                            IDX row, n;
                            mt_flat_pos<IDX>(o, dest_len, &row, &n);
                            EXPECT(row < rows && n < dest_len && row * dest_len + n == o, "flat %zu", (size_t)o);
                            ++writes[(size_t)o];
                        }
                for (size_t i = 0; i < writes.size(); ++i) EXPECT(writes[i] == 1, "flat element %zu written %d times", i, writes[i]);
            }
}

static void check_flat_large()
{
    // 70 000 rows x 70 001 outputs = 4 900 070 000 > 2^32: only the 64-bit map is right, and the launcher's predicate
    // keeps the 32-bit kernels away from it
    const size_t rows = 70000, dest_len = 70001, total = rows * dest_len;
    EXPECT(total > (size_t(1) << 32), "the large pair is not large");
    EXPECT(!mt_fits_32(rows * 1000, total) && !mt_fits_32(total, 10) && mt_fits_32(1000, (size_t(1) << 31) - 1),
           "32-bit predicate");
    const size_t probes[] = {0, 1, dest_len - 1, dest_len, dest_len + 1, (size_t(1) << 32) - 1, size_t(1) << 32,
                             (size_t(1) << 32) + 1, total - dest_len - 1, total - dest_len, total - 1};
    for (size_t o : probes) {
        size_t row, n;
        mt_flat_pos<size_t>(o, dest_len, &row, &n);
        EXPECT(row < rows && n < dest_len && row * dest_len + n == o, "64-bit flat %zu", o);
    }
    size_t row, n;
    mt_flat_pos<size_t>(total - 1, dest_len, &row, &n);
    EXPECT(row == rows - 1 && n == dest_len - 1, "last element");
    unsigned r32, n32; // what 32 bits would have made of an index above 2^32
    mt_flat_pos<unsigned>((unsigned)((size_t(1) << 32) + 5), (unsigned)dest_len, &r32, &n32);
    EXPECT(r32 == 0 && n32 == 5, "the 32-bit map wraps, as expected");
}

// the matrix kernels' loop against the vector kernels' loop, row by row, bit for bit
template <typename T>
static void check_interp_values()
{
    const struct { size_t rows, n; T factor, delay; } cases[] = {
        {3, 1, (T)2.0, (T)0}, {3, 2, (T)3.0, (T)0}, {5, 3, (T)0.5, (T)0}, {5, 7, (T)4.0, (T)0}, {5, 7, (T)3.0, (T)0},
        {4, 5, (T)3.0, (T)0.25}, {3, 100, (T)2.5, (T)0}, {2, 513, (T)0.5, (T)0}};
    for (const auto& c : cases) {
        std::vector<T> in(c.rows * c.n);
        for (size_t i = 0; i < in.size(); ++i) in[i] = (T)((i * 37 + 11) % 101) / (T)7 - (T)5;
        T v = (T)(c.n - 1) * c.factor; // interpolate_real_len
        const size_t dest_len = (size_t)(sizeof(T) == 4 ? roundf((float)v) : round((double)v)) + 1;
        long long start, tail;
        interp_hermite_regions<T>(dest_len, c.factor, c.delay, &start, &tail);
        EXPECT(start >= 0 && start <= tail && tail <= (long long)dest_len, "regions %lld %lld of %zu", start, tail, dest_len);
        for (int hermite = 0; hermite < 2; ++hermite) {
            std::vector<T> out(c.rows * dest_len, (T)-777);
            const size_t total = out.size(), stride = 3 * 64;
            for (size_t t = 0; t < stride; ++t)
                for (size_t o = t; o < total; o += stride) { // k_mt_interp_*
                    size_t row, n;
                    mt_flat_pos<size_t>(o, dest_len, &row, &n);
                    const T* rp = in.data() + row * c.n;
                    out[o] = hermite ? interp_hermite_value<T>(rp, (long long)c.n, (long long)n, c.factor, c.delay, start, tail)
                                     : interp_lin_value<T>(rp, (long long)c.n, (long long)dest_len, (long long)n, c.factor, c.delay);
                }
            for (size_t r = 0; r < c.rows; ++r)
                for (size_t n = 0; n < dest_len; ++n) { // k_interp_* on the row alone
                    const T* rp = in.data() + r * c.n;
                    const T ref = hermite ? interp_hermite_value<T>(rp, (long long)c.n, (long long)n, c.factor, c.delay, start, tail)
                                          : interp_lin_value<T>(rp, (long long)c.n, (long long)dest_len, (long long)n, c.factor, c.delay);
                    EXPECT(out[r * dest_len + n] == ref, "interp rows %zu n %zu hermite %d: (%zu, %zu)", c.rows, c.n, hermite, r, n);
                }
        }
    }
}

int main()
{
    check_conv();
    check_flat_small<unsigned>();
    check_flat_small<size_t>();
    check_flat_large();
    std::printf("interp flat map: dest_len 1..40, rows 1..3, 32- and 64-bit indices; 70000 x 70001 > 2^32\n");
    check_interp_values<float>();
    check_interp_values<double>();
    std::printf("interp values: matrix loop equals the per-row loop, f32 and f64\n");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
