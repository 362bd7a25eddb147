// sim_mat_interpf.cpp -- the matrix kernels of interpolatef (basic_dsp_amd/csrc/interp.hip) on the host, threads as loops
// over the maps of basic_dsp_amd/csrc/interp_core.h.
//
//   integer   k_mat_interpf_inner (virtual block -> (row, tile or edge workgroup), the tile's re-laid-out tap table, its x
//             window, the accumulation, the rotated output staging with the packet and the scalar store) and
//             k_mat_interpf_table (restaging when the row changes), with one tap table for all rows and with one per row
//   scalar    the flat walk of k_mat_interpf_scalar / _scalar_v2 / _frac_pk in 32 and 64 bits, the wrap-around reads and
//             the single-base-pointer reads of the packed kernel
//
// Checked: every output of every row is written exactly once; every global read of row r lies inside row r; every LDS
// slot that is read was staged by the current virtual block (inner) or for the current row (table); on the integer path
// the values equal the reference's two formulas (interp.hip's header) on small integers, where every product and sum is
// exact.  Cases: rows 1, 2, 3 and 70 000; points 1 .. 70, 255 .. 257, 1023 .. 1025; factors 2, 3, 4, 5, 8; L in {0, 1,
// points / 2} (above 1000 points the last with two rows only); grids smaller than the number of virtual blocks, so a
// workgroup crosses rows; a rows x new_points product above 2^32.
//
// g++ -O2 -std=c++17 (optionally -fsanitize=address,undefined) sim_mat_interpf.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../basic_dsp_amd/csrc/interp_core.h"

using namespace bdsp;

static int failures = 0;
#define EXPECT(cond, ...)                                                                          \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                          \
    } while (0)

struct IntCase {
    size_t rows;
    long long points;
    int f, L, E, QB, VN; // VN: scalars per 16-byte packet (4: f32, 2: f64)
    bool per_row_taps;
    unsigned grid;
};

// an LDS image whose slots remember who staged them
struct Lds {
    std::vector<double> v;
    std::vector<long long> tag;
    explicit Lds(size_t n) : v(n, 0.0), tag(n, -1) {}
    void put(size_t at, double x, long long who)
    {
        EXPECT(at < v.size(), "LDS write %zu of %zu", at, v.size());
        if (at < v.size()) { v[at] = x; tag[at] = who; }
    }
    double get(size_t at, long long who) const
    {
        EXPECT(at < v.size(), "LDS read %zu of %zu", at, v.size());
        if (at >= v.size()) return 0.0;
        EXPECT(tag[at] == who, "LDS slot %zu was staged by %lld, read for %lld", at, tag[at], who);
        return v[at];
    }
};

struct Mat {
    const IntCase& c;
    long long new_points;
    std::vector<double> x, taps, y;
    std::vector<int> writes;
    size_t tab;
    Mat(const IntCase& cc, long long np) : c(cc), new_points(np)
    {
        tab = (size_t)(2 * c.L + 1) * c.f;
        x.resize(c.rows * c.points * c.E);
        for (size_t i = 0; i < x.size(); ++i) x[i] = (double)((i * 7 + 3) % 23) - 11.0;
        taps.resize((c.per_row_taps ? c.rows : 1) * tab);
        for (size_t i = 0; i < taps.size(); ++i) taps[i] = (double)((i * 5 + 1) % 13) - 6.0;
        y.assign(c.rows * new_points * c.E, -12345.0);
        writes.assign(y.size(), 0);
    }
    // scalar `e` of point p of row r; the read must stay inside the row
    double in(size_t r, long long p, int e) const
    {
        EXPECT(p >= 0 && p < c.points, "row %zu: read of point %lld of %lld", r, p, c.points);
        if (p < 0 || p >= c.points) return 0.0;
        return x[(r * c.points + p) * c.E + e];
    }
    void out(size_t r, long long scalar, double v)
    {
        EXPECT(scalar >= 0 && scalar < new_points * c.E, "row %zu: write of scalar %lld of %lld", r, scalar, new_points * c.E);
        if (scalar < 0 || scalar >= new_points * c.E) return;
        const size_t at = r * new_points * c.E + scalar;
        y[at] = v;
        ++writes[at];
    }
};

// interp_table_walk of workgroup `block` of `nblocks` on row r; lt: the staged table, tagged `who`
static void table_walk(Mat& m, size_t r, const Lds& lds, long long who, long long skip_lo, long long skip_hi, unsigned block,
                       unsigned nblocks)
{
    const IntCase& c = m.c;
    const int ntaps = 2 * c.L + 1;
    const long long scalar_len = (long long)ntaps * c.f, nskip = if_skip_count(skip_lo, skip_hi);
    for (unsigned t = 0; t < IF_WG; ++t)
        for (long long g = (long long)block * IF_WG + t; g < m.new_points - nskip; g += (long long)nblocks * IF_WG) {
            const long long i = if_edge_output(g, skip_lo, nskip);
            double s[2] = {0, 0};
            if (if_is_edge(i, scalar_len, m.new_points)) {
                const size_t tb = (size_t)(i % c.f) * ntaps;
                long long pos = if_edge_start(i, c.f, c.L, c.points);
                for (int k = 0; k < ntaps; ++k) {
                    pos = if_wrap_next(pos, c.points);
                    for (int e = 0; e < c.E; ++e) s[e] += m.in(r, pos, e) * lds.get(tb + k, who);
                }
            } else {
                const long long end = if_inner_end(i, c.f, c.L);
                const size_t tb = (size_t)if_inner_shift(i, c.f) * ntaps;
                for (int k = ntaps - 1; k >= 0; --k)
                    for (int e = 0; e < c.E; ++e) s[e] += m.in(r, end - 1 - k, e) * lds.get(tb + k, who);
            }
            for (int e = 0; e < c.E; ++e) m.out(r, i * c.E + e, s[e]);
        }
}

// interp_inner_tile: positions [q0, min(q0 + TILE, q_hi)) of row r
static void inner_tile(Mat& m, size_t r, Lds& lds, long long who, const double* taps, long long q0, long long q_hi)
{
    const IntCase& c = m.c;
    const int F = c.f, E = c.E, QB = c.QB, L = c.L, ntaps = 2 * L + 1, TILE = 256 * QB;
    const size_t lt = 0, lx = lt + ((F * (ntaps + 1) + 3) & ~3), lo = lx + (((TILE + 2 * L + 2) * E + 3) & ~3);
    for (unsigned t = 0; t < IF_WG; ++t) {
        for (int k = t; k < (ntaps + 1) * F; k += 256) {
            const int j = k / F, sidx = k % F;
            double w = 0;
            if (sidx == 0) { if (j <= 2 * L) w = taps[2 * L - j]; }
            else if (j >= 1) w = taps[(F - sidx) * ntaps + 2 * L + 1 - j];
            lds.put(lt + k, w, who);
        }
        const int span = if_tile_span(TILE, L);
        const long long xbase = if_tile_xbase(q0, L);
        EXPECT(xbase >= 0, "tile window starts at %lld", xbase);
        for (int k = t; k < span * E; k += 256) {
            const long long g = xbase * E + k;
            lds.put(lx + k, g < c.points * E ? m.in(r, g / E, (int)(g % E)) : 0.0, who);
        }
    }
    // after the barrier
    const long long nq = if_tile_nq(q0, q_hi, TILE);
    const long long out0 = q0 * F * E, nout = nq * F * E;
    const int VN = c.VN, PER_THREAD = QB * F * E;
    const bool packets = (F * E) % VN == 0;
    const int PP = packets ? PER_THREAD / VN : 0;
    for (unsigned t = 0; t < IF_WG; ++t) {
        std::vector<double> flat(PER_THREAD, 0.0);
        for (int k = 0; k < QB; ++k)
            for (int j = 0; j <= 2 * L + 1; ++j)
                for (int s = 0; s < F; ++s)
                    for (int e = 0; e < E; ++e)
                        flat[(k * F + s) * E + e] += lds.get(lx + (size_t)(QB * t + k + j) * E + e, who) * lds.get(lt + j * F + s, who);
        if (packets) {
            for (int part = 0; part < PP; ++part)
                for (int e = 0; e < VN; ++e) lds.put(lo + (size_t)if_lo_slot((int)t, part, PP) * VN + e, flat[part * VN + e], who);
        } else {
            for (int k = 0; k < PER_THREAD; ++k) lds.put(lo + (size_t)t * PER_THREAD + k, flat[k], who);
        }
    }
    // after the second barrier
    const bool aligned = ((long long)(r * m.new_points * E) + out0) % VN == 0; // y itself is 16-byte aligned
    for (unsigned t = 0; t < IF_WG; ++t) {
        if (packets && aligned) {
            EXPECT(nout % VN == 0, "a tile ends inside a packet");
            for (long long k = t; k < nout / VN; k += 256) {
                const int q = (int)(k / PP), part = (int)(k % PP);
                for (int e = 0; e < VN; ++e) m.out(r, out0 + k * VN + e, lds.get(lo + (size_t)if_lo_slot(q, part, PP) * VN + e, who));
            }
        } else if (packets) {
            for (long long k = t; k < nout; k += 256) {
                const int pk = (int)(k / VN), e = (int)(k % VN);
                const int q = pk / PP, part = pk % PP;
                m.out(r, out0 + k, lds.get(lo + (size_t)if_lo_slot(q, part, PP) * VN + e, who));
            }
        } else {
            for (long long k = t; k < nout; k += 256) m.out(r, out0 + k, lds.get(lo + k, who));
        }
    }
}

static size_t int_cases = 0, blocked_cases = 0, table_cases = 0, unaligned_tiles = 0, crossings = 0;

static void check_int_case(const IntCase& c)
{
    long long new_points = c.points * c.f;
    if (c.E == 1) new_points += new_points % 2; // interpolatef_new_len: an odd scalar count is made even
    const bool has_blocked = c.f == 2 || c.f == 3 || c.f == 4 || c.f == 8;
    const IfGeom g = if_geom(c.points, new_points, c.L, c.f, 256u * c.QB, has_blocked, 1u << 20);
    Mat m(c, new_points);
    const int ntaps = 2 * c.L + 1, TILE = 256 * c.QB;
    const size_t tile_lds = ((c.f * (ntaps + 1) + 3) & ~3) + (((TILE + 2 * c.L + 2) * c.E + 3) & ~3) + (size_t)TILE * c.f * c.E;
    const size_t tap_stride = c.per_row_taps ? m.tab : 0;
    if (g.blocked) {
        ++blocked_cases;
        EXPECT(g.inner_blocks >= 1 && g.q_lo >= ntaps && g.q_hi * c.f + g.scalar_len <= new_points, "geometry");
        const unsigned per_row = g.inner_blocks + g.edge_blocks;
        const size_t total = c.rows * per_row;
        for (unsigned b = 0; b < c.grid; ++b) {
            Lds lds(tile_lds > m.tab ? tile_lds : m.tab);
            size_t last_row = ~(size_t)0;
            for (size_t vb = b; vb < total; vb += c.grid) {
                size_t row;
                unsigned k;
                if_block(vb, per_row, &row, &k);
                EXPECT(row < c.rows && k < per_row && row * per_row + k == vb, "block %zu", vb);
                if (last_row != ~(size_t)0 && last_row != row) ++crossings;
                last_row = row;
                const double* tr = m.taps.data() + row * tap_stride;
                if (k < g.inner_blocks) {
                    const long long q0 = if_tile_q0(g, k);
                    if (((long long)(row * new_points * c.E) + q0 * c.f * c.E) % c.VN != 0) ++unaligned_tiles;
                    inner_tile(m, row, lds, (long long)vb, tr, q0, g.q_hi);
                } else {
                    for (size_t q = 0; q < m.tab; ++q) lds.put(q, tr[q], (long long)vb);
                    table_walk(m, row, lds, (long long)vb, g.q_lo * c.f, g.q_hi * c.f, k - g.inner_blocks, g.edge_blocks);
                }
            }
        }
    } else {
        ++table_cases;
        const unsigned bpr = g.edge_blocks;
        const size_t total = c.rows * bpr, none = ~(size_t)0;
        for (unsigned b = 0; b < c.grid; ++b) {
            Lds lds(m.tab);
            size_t staged = none;
            for (size_t vb = b; vb < total; vb += c.grid) {
                size_t row;
                unsigned k;
                if_block(vb, bpr, &row, &k);
                EXPECT(row < c.rows && k < bpr, "block %zu", vb);
                const size_t want = tap_stride ? row : 0;
                if (staged != want) {
                    if (staged != none) ++crossings;
                    for (size_t q = 0; q < m.tab; ++q) lds.put(q, m.taps[want * tap_stride + q], (long long)want);
                    staged = want;
                }
                table_walk(m, row, lds, (long long)want, -1, -1, k, bpr);
            }
        }
    }
    // the reference's two formulas
    const long long N = c.points, scalar_len = (long long)ntaps * c.f;
    for (size_t r = 0; r < c.rows; ++r) {
        const double* tr = m.taps.data() + r * tap_stride;
        for (long long i = 0; i < new_points; ++i)
            for (int e = 0; e < c.E; ++e) {
                double ref = 0;
                if (i < scalar_len || i + scalar_len >= new_points || new_points < 2 * scalar_len) {
                    for (int k = 0; k < ntaps; ++k) {
                        long long p = (i / c.f - c.L + 1 + k) % N;
                        if (p < 0) p += N;
                        ref += m.x[(r * N + p) * c.E + e] * tr[(i % c.f) * ntaps + k];
                    }
                } else {
                    const long long cc = (i + c.f - 1) / c.f;
                    for (int k = 0; k < ntaps; ++k) ref += m.x[(r * N + cc + c.L - 1 - k) * c.E + e] * tr[((c.f - i % c.f) % c.f) * ntaps + k];
                }
                const size_t at = (r * new_points + i) * c.E + e;
                EXPECT(m.writes[at] == 1, "points %lld rows %zu f %d L %d: output (%zu, %lld) written %d times", c.points, c.rows, c.f,
                       c.L, r, i, m.writes[at]);
                EXPECT(m.y[at] == ref, "points %lld rows %zu f %d L %d E %d QB %d blocked %d: output (%zu, %lld) = %g, expected %g",
                       c.points, c.rows, c.f, c.L, c.E, c.QB, (int)g.blocked, r, i, m.y[at], ref);
            }
    }
    ++int_cases;
}

static void check_integer()
{
    std::vector<long long> points;
    for (long long n = 1; n <= 70; ++n) points.push_back(n);
    for (long long n : {255, 256, 257, 1023, 1024, 1025}) points.push_back(n);
    const int factors[] = {2, 3, 4, 5, 8};
    const int qbs[] = {1, 2, 4};
    const unsigned grids[] = {1, 2, 5};
    size_t n = 0;
    for (long long p : points)
        for (size_t rows = 1; rows <= 3; ++rows)
            for (int f : factors) {
                const long long ls[] = {0, 1, p / 2};
                for (long long l : ls) {
                    ++n;
                    if (p > 1000 && l > 1 && rows != 2) continue; // the thousand-tap double loops once per factor
                    IntCase c{rows, p, f, (int)l, (int)(1 + n % 2), qbs[n % 3], (n / 2) % 2 ? 4 : 2, (n / 3) % 2 == 0, grids[(n / 5) % 3]};
                    check_int_case(c);
                }
            }
    // 70 000 rows: more rows than a grid dimension holds, every workgroup crosses rows thousands of times
    check_int_case(IntCase{70000, 3, 2, 0, 1, 1, 4, true, 7});
    check_int_case(IntCase{70000, 2, 5, 1, 2, 1, 2, false, 3});
    EXPECT(blocked_cases > 0 && table_cases > 0 && unaligned_tiles > 0 && crossings > 0, "a variant was never taken: %zu %zu %zu %zu",
           blocked_cases, table_cases, unaligned_tiles, crossings);
    std::printf("integer: points 1..70 255 256 257 1023 1024 1025, rows 1..3 and 70000, factors 2 3 4 5 8, L 0 1 n/2: %zu cases "
                "(%zu blocked, %zu table; %zu tiles on unaligned rows, %zu row crossings)\n",
                int_cases, blocked_cases, table_cases, unaligned_tiles, crossings);
}

// ------------------------------------------------------------------------------------------------ scalar paths
static size_t fast_reads = 0, wrapped = 0;

template <typename IDX>
static void check_scalar_case(size_t rows, long long points, double factor, int L, unsigned grid)
{
    if (L > points / 2) L = (int)(points / 2);
    long long new_points = (long long)std::llround((double)points * factor);
    new_points += new_points % 2;
    if (new_points == 0) return;
    const int ntaps = 2 * L + 1;
    std::vector<int> writes(rows * (size_t)new_points, 0);
    const IDX width = (IDX)new_points, nrows = (IDX)rows;
    const long long stride = (long long)grid * IF_WG;
    for (unsigned b = 0; b < grid; ++b)
        for (unsigned t = 0; t < IF_WG; ++t) {
            IfPos<IDX> at = if_pos<IDX>((IDX)(b * IF_WG + t), width);
            const IfPos<IDX> step = if_pos<IDX>((IDX)stride, width);
            for (; at.row < nrows; if_advance<IDX>(&at, step, width)) {
                EXPECT(at.col < width, "column %llu of %lld", (unsigned long long)at.col, new_points);
                const long long i = (long long)at.col;
                const long long rounded = (long long)std::floor((double)i / factor);
                const long long p0 = if_scalar_start(rounded, L, points);
                EXPECT(p0 >= 0 && p0 < points, "start %lld of %lld", p0, points);
                if (!if_frac_wraps(p0, ntaps, points)) { // the packed kernel's single base pointer: x[p0 + 1 .. p0 + ntaps]
                    EXPECT(p0 + ntaps < points, "fast read of point %lld of %lld", p0 + ntaps, points);
                    ++fast_reads;
                } else ++wrapped;
                long long pos = p0;
                for (int k = 0; k < ntaps; ++k) {
                    pos = if_wrap_next(pos, points);
                    EXPECT(pos >= 0 && pos < points, "read of point %lld of %lld", pos, points);
                }
                const size_t o = (size_t)at.row * (size_t)new_points + (size_t)i;
                EXPECT(o < writes.size(), "output %zu", o);
                if (o < writes.size()) ++writes[o];
            }
        }
    for (size_t o = 0; o < writes.size(); ++o)
        EXPECT(writes[o] == 1, "rows %zu points %lld factor %g: output %zu written %d times", rows, points, factor, o, writes[o]);
}

static void check_scalar()
{
    std::vector<long long> points;
    for (long long n = 1; n <= 70; ++n) points.push_back(n);
    for (long long n : {255, 256, 257, 1023, 1024, 1025}) points.push_back(n);
    const double factors[] = {0.5, 1.5, 13.0 / 6.0, 48.0 / 44.1, 2.0};
    const unsigned grids[] = {1, 2, 3};
    size_t n = 0;
    for (long long p : points)
        for (size_t rows = 1; rows <= 3; ++rows)
            for (double f : factors) {
                const long long ls[] = {0, 1, p / 2};
                for (long long l : ls) {
                    ++n;
                    check_scalar_case<unsigned>(rows, p, f, (int)l, grids[n % 3]);
                    check_scalar_case<size_t>(rows, p, f, (int)l, grids[(n + 1) % 3]);
                }
            }
    check_scalar_case<unsigned>(70000, 3, 1.5, 1, 2);
    check_scalar_case<size_t>(70000, 3, 1.5, 1, 2);
    EXPECT(fast_reads > 0 && wrapped > 0, "fast %zu wrapped %zu", fast_reads, wrapped);
    // 70 000 rows x 70 002 outputs = 4 900 140 000 > 2^32: only the 64-bit walk is right, and the launcher's predicate keeps
    // the 32-bit kernels away from it
    const size_t rows = 70000, np = 70002, total = rows * np, stride = 2048 * 256;
    EXPECT(total > (size_t(1) << 32), "the large pair is not large");
    EXPECT(!if_fits_32(1000, total, rows, stride) && !if_fits_32(total, 10, rows, stride) &&
           !if_fits_32(1000, (size_t(1) << 31) - 5, 10, stride) && if_fits_32(1000, (size_t(1) << 30), 70000, stride), "32-bit predicate");
    const IfPos<size_t> step = if_pos<size_t>(stride, np);
    const size_t probes[] = {0, 1, np - 1, np, np + 1, (size_t(1) << 32) - 1, size_t(1) << 32, (size_t(1) << 32) + 1,
                             total - np - 1, total - np, total - stride - 1};
    for (size_t o : probes) {
        IfPos<size_t> at = if_pos<size_t>(o, np);
        EXPECT(at.row < rows && at.col < np && at.row * np + at.col == o, "64-bit flat %zu", o);
        if_advance<size_t>(&at, step, np);
        EXPECT(at.col < np && at.row * np + at.col == o + stride, "64-bit advance from %zu", o);
    }
    IfPos<size_t> last = if_pos<size_t>(total - 1, np);
    EXPECT(last.row == rows - 1 && last.col == np - 1, "last element");
    if_advance<size_t>(&last, step, np);
    EXPECT(last.row >= rows, "the walk ends past the last row");
    std::printf("scalar: points 1..70 255 256 257 1023 1024 1025, rows 1..3 and 70000, 32- and 64-bit walks; 70000 x 70002 > 2^32\n");
}

int main()
{
    check_integer();
    check_scalar();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
