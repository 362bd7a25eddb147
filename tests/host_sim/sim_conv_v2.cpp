// sim_conv_v2.cpp -- the second-generation overlap-save block kernel (basic_dsp_amd/csrc/conv_v2_impl.h,
// k_overlap_save_v2) on the host: the plan and the index functions of conv_v2_core.h, the same text the library
// compiles, with workgroups and threads as loops, and the block chain the kernel composes from fft_core.h.
//
// GEOMETRY.  For every case of the sweep (dispatch groups x CU counts x tap counts x vector lengths x complex / real
// x batch x partial runs x shares) the plan is computed and every workgroup of its grid walks the kernel's two loops:
//   * grid is a multiple of 8 groups; every wrap-around index and every interior id is taken by exactly one workgroup;
//     the two maps (index -> vector, block) together reach every block [b0, b1) of every vector exactly once;
//   * every interior block's window and its stored rows lie inside its vector (four comparisons per block).
// Which ELEMENTS a block reads and writes depends on (taps, n, real, batch, partial run) alone, not on which workgroup
// takes it, so the element level runs once per such geometry and not once per CU count, group count and share: every
// block's loads and stores are made thread by thread (256 threads x 16 rows) on arrays that refuse every read
// outside [0, n) of the block's vector and count every store; afterwards every output in [b0 U V, min(b1 U V, n)) of
// every vector has been written exactly once and nothing else has (U = 2 real blocks per kernel block for real data).
// Blocks taken once each (per case) times stores made once each (per geometry) is the per-case statement.  The two
// largest lengths (300 V + 5 and 2200 V + 1: several rounds of a full grid at 256 and 304 CUs) skip the element level.
//
// NUMBERS.  For every `taps` and `len` line of tests/conv_v2_shapes.txt, for complex data with the taps transformed
// in the block (hs_is_taps) and with a prepared spectrum delayed by the phase table, and for real pairs; in f32 (exchange
// A in the conflict-free layout, FMA twiddles in registers) and f64 (stage-2 table in LDS, two held stage-3 values):
// the wrap-around blocks at both ends of the vector and, where the length has one, the middle interior block run load ->
// forward -> x H -> inverse with PRUNE -> store of rows R0 .. 15, the stores are counted against the outputs the block
// owes, and the result is compared with the direct circular convolution y[i] = sum_k x[(i + ceil(M/2) - 1 - k) mod n] h[k]
// in long double.  The data are f32 values in both precisions, so one reference serves both.  Bound: rel-L2 over the
// outputs of a case's blocks 1e-6 (f32) / 1e-12 (f64), the project's figures for one convolution ("f32 FFT /
// convolution").
//
// g++ -O2 -std=c++17 (optionally -fsanitize=address,undefined) sim_conv_v2.cpp && ./a.out ../conv_v2_shapes.txt
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "../../basic_dsp_amd/csrc/conv_v2_core.h"

using namespace bdsp;

static const long double PI_L = 3.14159265358979323846264338327950288L;
static constexpr int L = CONV_V2_L;
static long long g_fail = 0;
static void fail(const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0)
{
    if (++g_fail <= 20) printf("FAIL %s (%lld %lld %lld %lld)\n", what, a, b, c, d);
}

static unsigned long long g_seed = 0x2545F4914F6CDD1Dull;
static double noise()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (double)(g_seed >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

// ------------------------------------------------------------------ memory that checks
// `batch` vectors of n elements; reads outside [0, n) of the vector are refused, stores are counted
template <typename E>
struct Checked {
    size_t n, batch;
    std::vector<E> d;
    std::vector<unsigned char> cnt;
    long long bad_reads = 0, bad_writes = 0;
    Checked(size_t n_, size_t batch_) : n(n_), batch(batch_), d(n_ * batch_), cnt(n_ * batch_, 0) {}
    E rd(size_t vec, long long i)
    {
        if (vec >= batch || i < 0 || i >= (long long)n) { ++bad_reads; return E{}; }
        return d[vec * n + (size_t)i];
    }
    void wr(size_t vec, long long i, E v)
    {
        if (vec >= batch || i < 0 || i >= (long long)n) { ++bad_writes; return; }
        d[vec * n + (size_t)i] = v;
        if (cnt[vec * n + (size_t)i] < 255) ++cnt[vec * n + (size_t)i];
    }
};

template <typename T> struct Regs { cpx<T> v[16]; };

// what the kernel reads of its arguments for loads and stores
struct Geom {
    unsigned n, taps, r0, V, OV;
    long long in_off;
};
static Geom geom_of(size_t n, size_t taps)
{
    Geom g;
    g.n = (unsigned)n; g.taps = (unsigned)taps; g.r0 = conv_v2_r0(taps);
    g.V = (unsigned)L - 256u * g.r0; g.OV = 256u * g.r0;
    g.in_off = conv_v2_in_off(g.taps);
    return g;
}

// ---- the loads and stores of k_overlap_save_v2, thread by thread.  For complex data X is Checked<cpx<T>>, for real
// data Checked<T> (the kernel reads x and y as arrays of T then).
template <typename T>
static void wrap_load(Checked<cpx<T>>& x, const Geom& g, unsigned vec, unsigned b, std::vector<Regs<T>>& regs)
{
    const long long sb = conv_v2_window_start((long long)b, g.V, g.in_off, g.n);
    for (unsigned ut = 0; ut < 256; ++ut) {
        const unsigned idx = (unsigned)sb + ut;
        if (g.n >= (unsigned)L) {
            for (int r = 0; r < 16; ++r) {
                unsigned i = idx + 256u * r;
                if (i >= g.n) i -= g.n;
                regs[ut].v[r] = x.rd(vec, i);
            }
        } else {
            for (int r = 0; r < 16; ++r) regs[ut].v[r] = x.rd(vec, (idx + 256u * r) % g.n);
        }
    }
}
template <typename T>
static void wrap_store(Checked<cpx<T>>& y, const Geom& g, unsigned vec, unsigned b, const std::vector<Regs<T>>& regs)
{
    const long long obase = conv_v2_obase((long long)b, g.V, g.OV);
    const unsigned lim = conv_v2_store_limit(g.n, obase);
    for (unsigned ut = 0; ut < 256; ++ut)
        for (int r = (int)g.r0; r < 16; ++r) {
            const unsigned np = ut + 256u * r;
            if (np < lim) y.wr(vec, obase + np, regs[ut].v[r]);
        }
}
template <typename T>
static void wrap_load(Checked<T>& x, const Geom& g, unsigned vec, unsigned b, std::vector<Regs<T>>& regs)
{
    for (int half = 0; half < 2; ++half) {
        const long long sb = conv_v2_window_start((long long)(2 * b + half), g.V, g.in_off, g.n);
        for (unsigned ut = 0; ut < 256; ++ut)
            for (int r = 0; r < 16; ++r) {
                const T s = x.rd(vec, (long long)(((unsigned long long)sb + ut + 256u * r) % g.n));
                if (half) regs[ut].v[r].y = s; else regs[ut].v[r].x = s;
            }
    }
}
template <typename T>
static void wrap_store(Checked<T>& y, const Geom& g, unsigned vec, unsigned b, const std::vector<Regs<T>>& regs)
{
    for (int half = 0; half < 2; ++half) {
        const long long obase = conv_v2_obase((long long)(2 * b + half), g.V, g.OV);
        const unsigned lim = conv_v2_store_limit(g.n, obase);
        for (unsigned ut = 0; ut < 256; ++ut)
            for (int r = (int)g.r0; r < 16; ++r) {
                const unsigned np = ut + 256u * r;
                if (np < lim) y.wr(vec, obase + np, half ? regs[ut].v[r].y : regs[ut].v[r].x);
            }
    }
}
template <typename T>
static void interior_load(Checked<cpx<T>>& x, const Geom& g, unsigned vec, unsigned b, std::vector<Regs<T>>& regs)
{
    const long long off = (long long)b * g.V + g.in_off;
    for (unsigned ut = 0; ut < 256; ++ut)
        for (int r = 0; r < 16; ++r) regs[ut].v[r] = x.rd(vec, off + (ut + 256u * r));
}
template <typename T>
static void interior_store(Checked<cpx<T>>& y, const Geom& g, unsigned vec, unsigned b, const std::vector<Regs<T>>& regs)
{
    const long long off = conv_v2_obase((long long)b, g.V, g.OV);
    for (unsigned ut = 0; ut < 256; ++ut)
        for (int r = (int)g.r0; r < 16; ++r) y.wr(vec, off + (ut + 256u * r), regs[ut].v[r]);
}
template <typename T>
static void interior_load(Checked<T>& x, const Geom& g, unsigned vec, unsigned b, std::vector<Regs<T>>& regs)
{
    const long long off = (long long)(2 * b) * g.V + g.in_off;
    for (unsigned ut = 0; ut < 256; ++ut)
        for (int r = 0; r < 16; ++r) regs[ut].v[r] = cpx<T>{x.rd(vec, off + (ut + 256u * r)), x.rd(vec, off + (g.V + ut + 256u * r))};
}
template <typename T>
static void interior_store(Checked<T>& y, const Geom& g, unsigned vec, unsigned b, const std::vector<Regs<T>>& regs)
{
    const long long off = conv_v2_obase((long long)(2 * b), g.V, g.OV);
    for (unsigned ut = 0; ut < 256; ++ut)
        for (int r = (int)g.r0; r < 16; ++r) {
            y.wr(vec, off + (ut + 256u * r), regs[ut].v[r].x);
            y.wr(vec, off + (g.V + ut + 256u * r), regs[ut].v[r].y);
        }
}

// ------------------------------------------------------------------ geometry
static const int SHARE_DEFAULT = -1;
struct Share { int a, b; };

// element level: every block of the plan, loads and stores thread by thread
template <typename E>
static void elements_once(const ConvV2Plan& p, const Geom& g, size_t batch, bool real)
{
    Checked<E> x(g.n, batch), y(g.n, batch);
    std::vector<Regs<float>> regs(256);
    for (unsigned vec = 0; vec < batch; ++vec)
        for (long long b = p.b0; b < p.b1; ++b) {
            if (b >= p.lo && b < p.hi) { interior_load(x, g, vec, (unsigned)b, regs); interior_store(y, g, vec, (unsigned)b, regs); }
            else { wrap_load(x, g, vec, (unsigned)b, regs); wrap_store(y, g, vec, (unsigned)b, regs); }
        }
    if (x.bad_reads || y.bad_writes) fail("element out of its vector", g.n, g.taps, x.bad_reads, y.bad_writes);
    const long long U = real ? 2 : 1;
    const long long first = p.b0 * U * g.V, end = std::min<long long>(p.b1 * U * g.V, g.n);
    for (unsigned vec = 0; vec < batch; ++vec)
        for (long long i = 0; i < (long long)g.n; ++i) {
            const int want = i >= first && i < end ? 1 : 0;
            if (y.cnt[vec * g.n + i] != want) { fail("store count", g.n, g.taps, i, y.cnt[vec * g.n + i]); return; }
        }
}

// block level: the kernel's two loops for every workgroup of the grid
static void blocks_once(const ConvV2Plan& p, const Geom& g, size_t batch, bool real, unsigned groups)
{
    ConvV2Args<float> a{};
    conv_v2_set_geometry(a, p, g.n, g.taps, batch, groups);
    const bool batched = real || batch > 1; // (launch_v2: the batched instantiation serves real data)
    const long long U = real ? 2 : 1;
    if (p.grid == 0 || p.grid % (8 * groups) != 0 || p.gs * groups != p.grid) fail("grid", p.grid, groups);
    if (!(p.b0 <= p.lo && p.lo <= p.hi && p.hi <= p.b1)) fail("interior range", p.b0, p.lo, p.hi, p.b1);
    // every interior block's window and stored rows inside its vector
    for (long long b = p.lo; b < p.hi; ++b) {
        const long long first_read = U * b * g.V + g.in_off, last_read = (U * b + U - 1) * g.V + g.in_off + L;
        const long long first_store = conv_v2_obase(U * b, g.V, g.OV) + g.OV, last_store = conv_v2_obase(U * b + U - 1, g.V, g.OV) + L;
        if (first_read < 0 || last_read > (long long)g.n || first_store < 0 || last_store > (long long)g.n) fail("interior window", g.n, g.taps, b);
    }
    const unsigned nblk = (unsigned)(p.b1 - p.b0), ni = a.nb_hi - a.nb_lo, total = ni * a.batch;
    std::vector<unsigned char> taken((size_t)nblk * batch, 0), id_taken(total, 0);
    const unsigned G = p.grid;
    for (unsigned wg = 0; wg < G; ++wg) {
        {
            const unsigned nw = conv_v2_wrap_count(a.b_first, a.nb_lo, a.nb_hi, a.b_end), total_w = nw * a.batch;
            for (unsigned w = wg; w < total_w; w += G) {
                const unsigned vec = w / nw, k = w % nw;
                const unsigned b = conv_v2_wrap_block(k, a.b_first, a.nb_lo, a.nb_hi);
                if (vec >= batch || b < a.b_first || b >= a.b_end || (b >= a.nb_lo && b < a.nb_hi)) { fail("wrap index", w, vec, b); continue; }
                ++taken[(size_t)vec * nblk + (b - a.b_first)];
            }
        }
        const unsigned gs = G / a.groups;
        const unsigned grp = wg / gs;
        if (grp >= a.groups) continue;
        const unsigned lo = conv_v2_group_lo(grp, a.na, a.nbb);
        const unsigned hi = conv_v2_group_hi(grp, a.groups, a.na, a.nbb, total);
        if (lo > hi || hi > total) { fail("group range", grp, lo, hi, total); continue; }
        const unsigned w2 = xcd_contiguous(wg - grp * gs, gs);
        if (w2 >= gs) { fail("xcd_contiguous", wg, w2, gs); continue; }
        for (unsigned id = lo + w2; id < hi; id += gs) {
            unsigned vec, b;
            if (batched) conv_v2_split_id<true>(id, ni, a.nb_lo, vec, b); else conv_v2_split_id<false>(id, ni, a.nb_lo, vec, b);
            ++id_taken[id];
            if (vec >= batch || b < a.nb_lo || b >= a.nb_hi) { fail("interior id", id, vec, b); continue; }
            ++taken[(size_t)vec * nblk + (b - a.b_first)];
        }
    }
    for (unsigned id = 0; id < total; ++id)
        if (id_taken[id] != 1) { fail("interior id taken", id, id_taken[id], g.n, g.taps); break; }
    for (size_t i = 0; i < taken.size(); ++i)
        if (taken[i] != 1) { fail("block taken", (long long)i, taken[i], g.n, g.taps); break; }
}

static std::vector<size_t> sweep_taps()
{
    std::vector<size_t> t = {1, 2, 18};
    for (size_t k = 1; k <= 12; ++k) { // either side of every row boundary: R0 steps between 256 k + 1 and 256 k + 2
        t.push_back(256 * k);
        t.push_back(256 * k + 1);
        if (k < 12) t.push_back(256 * k + 2); // (3073 is the largest filter the kernel takes)
    }
    return t;
}

static long long geometry(const std::vector<Share>& overrides)
{
    long long cases = 0, geometries = 0;
    const unsigned group_counts[] = {3, 2};
    const int cu_counts[] = {1, 8, 256, 304};
    const size_t partial[5][2] = {{0, 0}, {1, 0}, {0, 2}, {2, 3}, {3, 1}}; // (first_block, nblocks); 0 blocks = all the rest
    std::vector<Share> shares = {{SHARE_DEFAULT, SHARE_DEFAULT}};
    shares.insert(shares.end(), overrides.begin(), overrides.end());
    for (size_t taps : sweep_taps()) {
        const long long V = L - 256 * (long long)conv_v2_r0(taps);
        std::vector<std::pair<long long, bool>> lens; // (n, with the element level)
        lens.push_back({(long long)taps, true});
        for (long long a : {1, 2, 5})
            for (long long c : {-1, 0, 1}) lens.push_back({a * V + c, true});
        for (long long a : {1, 2, 3})
            for (long long c : {-1, 0, 1}) lens.push_back({a * 4096 + c, true});
        lens.push_back({5 * V + 7, true});
        lens.push_back({9 * V + 7, true});
        lens.push_back({300 * V + 5, false});
        lens.push_back({2200 * V + 1, false});
        for (auto [n, with_elements] : lens) {
            if (n < (long long)taps) continue; // (the library refuses filters longer than the vector)
            const Geom g = geom_of((size_t)n, taps);
            for (int real = 0; real < 2; ++real)
                for (size_t batch : {(size_t)1, (size_t)3})
                    for (const auto& pr : partial) {
                        bool first = true;
                        ConvV2Plan ref{};
                        for (unsigned groups : group_counts)
                            for (int cus : cu_counts)
                                for (const Share& sh : shares) {
                                    ++cases;
                                    const ConvV2Plan p = conv_v2_plan((size_t)n, taps, batch, pr[0], pr[1], real != 0, cus, groups, sh.a, sh.b);
                                    if (p.status == CONV_V2_PLAN_TOO_MANY) { fail("too many blocks", n, (long long)taps); continue; }
                                    if (first) {
                                        ref = p; first = false;
                                        if (p.status == CONV_V2_PLAN_RUN && with_elements) {
                                            ++geometries;
                                            if (real) elements_once<float>(p, g, batch, true); else elements_once<cpx<float>>(p, g, batch, false);
                                        }
                                    }
                                    // the blocks and their split into interior and wrap-around do not depend on the machine
                                    if (p.status != ref.status || p.b0 != ref.b0 || p.b1 != ref.b1 || p.lo != ref.lo || p.hi != ref.hi || p.r0 != ref.r0 || p.V != ref.V)
                                        fail("plan depends on the machine", n, (long long)taps, cus, groups);
                                    if (p.status == CONV_V2_PLAN_NOTHING) {
                                        const long long U = real ? 2 : 1, nb_all = ((n + V - 1) / V + U - 1) / U;
                                        if ((long long)pr[0] < nb_all) fail("nothing to do", n, (long long)taps, (long long)pr[0]);
                                        continue;
                                    }
                                    blocks_once(p, g, batch, real != 0, groups);
                                }
                    }
        }
    }
    printf("geometry: %lld cases (%lld element-level geometries), %lld failures\n", cases, geometries, g_fail);
    return cases;
}

// ------------------------------------------------------------------ numbers: the block chain
template <typename T>
struct Chain {
    using C = cpx<T>;
    using F = WgFft<T, L, 256>;
    static constexpr bool F32 = sizeof(T) == 4;
    static constexpr int TW3_HELD = 2;
    std::vector<C> wtab, lds;
    std::vector<C> tw2f, tw3f, tw3q; // per thread: 8, 8 (f32) and 2 (f64) values
    std::vector<Regs<T>> hreg;
    Chain() : wtab(L), lds(F32 ? (size_t)F::LDS_ELEMS3 : (size_t)F::LDS_ELEMS + 16 * 17), tw2f(256 * 8), tw3f(256 * 8), tw3q(256 * 2), hreg(256)
    {
        for (int m = 0; m < L; ++m) wtab[m] = C{(T)cosl(-2.0L * PI_L * m / L), (T)sinl(-2.0L * PI_L * m / L)};
        auto tww = [&](int mm) { return wtab[mm]; };
        C* tw2l = lds.data() + F::LDS_ELEMS;
        for (int t = 0; t < 256; ++t) {
            if (F32) {
                F::template load_twiddles16_fma<16>(&tw2f[8 * t], t, tww);
                F::template load_twiddles16_fma<256>(&tw3f[8 * t], t, tww);
            } else {
                if (t < 128) {
                    const int k = t >> 3, j = t & 7, e = 16 * k;
                    tw2l[k * 9 + j] = wtab[j == 0 ? 8 * e : j == 1 ? 4 * e : j == 2 ? 2 * e : j == 3 ? 2 * e + L / 8 : e + (j - 4) * (L / 16)];
                }
                tw3q[2 * t] = wtab[2 * t];
                tw3q[2 * t + 1] = wtab[t];
            }
        }
    }
    template <int DIR, int P> void stage3(C (&v)[16], int t)
    {
        if (F32) dft16_tw<DIR, P>(&v[0], &tw3f[8 * t]);
        else {
            C tl[8];
            expand_twiddles16_fma<TW3_HELD>(&tw3q[2 * t], tl);
            dft16_tw<DIR, P>(&v[0], tl);
        }
    }
    template <int DIR> void stage2(C (&v)[16], int t)
    {
        if (F32) dft16_tw<DIR>(&v[0], &tw2f[8 * t]);
        else {
            const C* tw2p = lds.data() + F::LDS_ELEMS + (t & 15) * 9;
            C tl[8];
            for (int j = 0; j < 8; ++j) tl[j] = tw2p[j];
            dft16_tw<DIR>(&v[0], tl);
        }
    }
    // the kernel's forward (DIR = -1, P = 0) and inverse (DIR = 1, P = PRUNE) lambdas; a barrier is the end of a loop over t
    template <int DIR, int P> void transform1(std::vector<Regs<T>>& regs)
    {
        auto tww = [&](int mm) { return wtab[mm]; };
        C* l = lds.data();
        for (int t = 0; t < 256; ++t) F::template compute<16, 1, DIR>(regs[t].v, t, tww);
        for (int t = 0; t < 256; ++t) { if (F32) F::scatter_a3(regs[t].v, t, l); else F::scatter_a(regs[t].v, t, l); }
        for (int t = 0; t < 256; ++t) {
            if (F32) F::gather_a3(regs[t].v, t, l); else F::gather_a(regs[t].v, t, l);
            stage2<DIR>(regs[t].v, t);
        }
        for (int t = 0; t < 256; ++t) { if (F32) F::scatter_b3(regs[t].v, t, l); else F::scatter_b(regs[t].v, t, l); }
        for (int t = 0; t < 256; ++t) {
            F::gather_b(regs[t].v, t, l);
            stage3<DIR, P>(regs[t].v, t);
        }
    }
    void forward(std::vector<Regs<T>>& regs) { transform1<-1, 0>(regs); }
    void inverse(std::vector<Regs<T>>& regs, unsigned r0)
    {
        switch (r0 <= 8 ? r0 : 0) { // PRUNE
        case 0: transform1<1, 0>(regs); break;
        case 1: transform1<1, 1>(regs); break;
        case 2: transform1<1, 2>(regs); break;
        case 3: transform1<1, 3>(regs); break;
        case 4: transform1<1, 4>(regs); break;
        case 5: transform1<1, 5>(regs); break;
        case 6: transform1<1, 6>(regs); break;
        case 7: transform1<1, 7>(regs); break;
        default: transform1<1, 8>(regs); break;
        }
    }
    // the filter spectrum, delayed by d samples, x 1/L, in register r of thread t: H'[t + 256 r].  hs: the taps (complex,
    // or real when `real`), or for prepared the unscaled, undelayed spectrum
    void set_filter(const Geom& g, const std::vector<C>& hs_c, const std::vector<T>& hs_r, bool real, bool hs_is_taps)
    {
        const T hscale = (T)1 / (T)L;
        const unsigned d = conv_v2_delay(g.OV, g.taps);
        if (hs_is_taps) {
            std::vector<Regs<T>> hv(256);
            for (unsigned ut = 0; ut < 256; ++ut)
                for (int r = 0; r < 16; ++r) {
                    const unsigned i = ut + 256u * r;
                    const bool in = i >= d && i - d < g.taps;
                    if (real) hv[ut].v[r] = in ? C{hs_r.at(i - d), (T)0} : C{(T)0, (T)0};
                    else hv[ut].v[r] = in ? hs_c.at(i - d) : C{(T)0, (T)0};
                }
            forward(hv);
            for (unsigned ut = 0; ut < 256; ++ut)
                for (int r = 0; r < 16; ++r) hreg[ut].v[r] = C{hv[ut].v[r].x * hscale, hv[ut].v[r].y * hscale};
        } else {
            for (unsigned ut = 0; ut < 256; ++ut)
                for (int r = 0; r < 16; ++r) {
                    const unsigned k = ut + 256u * r;
                    const C hv = hs_c.at(k);
                    hreg[ut].v[r] = cmul(C{hv.x * hscale, hv.y * hscale}, wtab[(k * d) & (L - 1)]);
                }
        }
    }
    // what bdsp_hip_dev_conv_prepare leaves: the L-point transform of the zero-padded taps in natural order, in T
    std::vector<C> prepare(const std::vector<C>& taps)
    {
        std::vector<Regs<T>> hv(256);
        for (unsigned ut = 0; ut < 256; ++ut)
            for (int r = 0; r < 16; ++r) {
                const unsigned i = ut + 256u * r;
                hv[ut].v[r] = i < taps.size() ? taps[i] : C{(T)0, (T)0};
            }
        forward(hv);
        std::vector<C> out(L);
        for (unsigned ut = 0; ut < 256; ++ut)
            for (int r = 0; r < 16; ++r) out[ut + 256u * r] = hv[ut].v[r];
        return out;
    }
    void transform(std::vector<Regs<T>>& regs, unsigned r0)
    {
        forward(regs);
        for (int t = 0; t < 256; ++t)
            for (int r = 0; r < 16; ++r) regs[t].v[r] = cmul(regs[t].v[r], hreg[t].v[r]);
        inverse(regs, r0);
    }
};

struct CL { long double x, y; };
// outputs [first, end) of the circular convolution, long double; complex (interleaved) or real data
static std::vector<CL> direct(const std::vector<float>& x, const std::vector<float>& h, bool real, long long n, long long m, long long first, long long end)
{
    std::vector<CL> out((size_t)(end - first));
    std::vector<long double> xl(x.begin(), x.end()), hl(h.begin(), h.end());
    const long long shift = (m + 1) / 2 - 1;
    for (long long i = first; i < end; ++i) {
        long long pos = ((i + shift) % n + n) % n;
        long double sr = 0, si = 0;
        if (real) {
            const long double* xp = xl.data();
            for (long long k = 0; k < m; ++k) {
                sr += xp[pos] * hl[k];
                pos = pos > 0 ? pos - 1 : n - 1;
            }
        } else {
            const long double* xp = xl.data();
            for (long long k = 0; k < m; ++k) {
                const long double ar = xp[2 * pos], ai = xp[2 * pos + 1], br = hl[2 * k], bi = hl[2 * k + 1];
                sr += ar * br - ai * bi;
                si += ar * bi + ai * br;
                pos = pos > 0 ? pos - 1 : n - 1;
            }
        }
        out[(size_t)(i - first)] = CL{sr, si};
    }
    return out;
}

struct NumCase {
    std::vector<float> x, h;                      // complex interleaved or real
    std::map<long long, std::vector<CL>> ref;     // per block: its outputs
};
static double g_worst[2] = {0, 0};
static long long g_blocks = 0;

// one block of one vector through the chain; adds the squared error and the squared reference of its outputs to num, den
template <typename T>
static void run_block(Chain<T>& ch, const Geom& g, const NumCase& nc, bool real, bool interior, unsigned b, const std::vector<CL>& ref,
                      long double& num, long double& den)
{
    std::vector<Regs<T>> regs(256);
    const long long U = real ? 2 : 1;
    const long long first = (long long)b * U * g.V, end = std::min<long long>((long long)(b + 1) * U * g.V, g.n);
    long long bad = 0, miscounted = 0;
    if (real) {
        Checked<T> x(g.n, 1), y(g.n, 1);
        for (size_t i = 0; i < g.n; ++i) x.d[i] = (T)nc.x[i];
        if (interior) interior_load(x, g, 0, b, regs); else wrap_load(x, g, 0, b, regs);
        ch.transform(regs, g.r0);
        if (interior) interior_store(y, g, 0, b, regs); else wrap_store(y, g, 0, b, regs);
        bad = x.bad_reads + y.bad_writes;
        for (long long i = 0; i < (long long)g.n; ++i) {
            if (y.cnt[i] != (i >= first && i < end ? 1 : 0)) ++miscounted;
            if (i >= first && i < end) {
                const long double dx = (long double)y.d[i] - ref[i - first].x;
                num += dx * dx; den += ref[i - first].x * ref[i - first].x;
            }
        }
    } else {
        Checked<cpx<T>> x(g.n, 1), y(g.n, 1);
        for (size_t i = 0; i < g.n; ++i) x.d[i] = cpx<T>{(T)nc.x[2 * i], (T)nc.x[2 * i + 1]};
        if (interior) interior_load(x, g, 0, b, regs); else wrap_load(x, g, 0, b, regs);
        ch.transform(regs, g.r0);
        if (interior) interior_store(y, g, 0, b, regs); else wrap_store(y, g, 0, b, regs);
        bad = x.bad_reads + y.bad_writes;
        for (long long i = 0; i < (long long)g.n; ++i) {
            if (y.cnt[i] != (i >= first && i < end ? 1 : 0)) ++miscounted;
            if (i >= first && i < end) {
                const long double dx = (long double)y.d[i].x - ref[i - first].x, dy = (long double)y.d[i].y - ref[i - first].y;
                num += dx * dx + dy * dy; den += ref[i - first].x * ref[i - first].x + ref[i - first].y * ref[i - first].y;
            }
        }
    }
    ++g_blocks;
    if (bad || miscounted) fail("numbers: stores against the outputs owed", g.n, g.taps, bad, miscounted);
}

template <typename T>
static void numbers_for(Chain<T>& ch, const Geom& g, const NumCase& nc, bool real, const std::vector<std::pair<unsigned, bool>>& blocks,
                        const std::map<long long, std::vector<CL>>& refs)
{
    using C = cpx<T>;
    std::vector<C> hc;
    std::vector<T> hr;
    if (real) { hr.assign(nc.h.begin(), nc.h.end()); }
    else for (size_t k = 0; k < g.taps; ++k) hc.push_back(C{(T)nc.h[2 * k], (T)nc.h[2 * k + 1]});
    for (int prepared = 0; prepared < (real ? 1 : 2); ++prepared) { // (real data come with taps only)
        if (prepared) ch.set_filter(g, ch.prepare(hc), hr, false, false);
        else ch.set_filter(g, hc, hr, real, true);
        // rel-L2 over the outputs of the case's blocks together, the norm the project's bound for a convolution is stated
        // in (one output alone can be small by cancellation while its error follows |x| |h|: 5 V + 7 and 2 V + 1 leave
        // the last block 7 outputs and 1)
        long double num = 0, den = 0;
        for (auto [b, interior] : blocks) run_block<T>(ch, g, nc, real, interior, b, refs.at(b), num, den);
        const double err = den > 0 ? (double)sqrtl(num / den) : (num > 0 ? 1.0 : 0.0);
        const int pi = sizeof(T) == 4 ? 0 : 1;
        if (err > g_worst[pi]) g_worst[pi] = err;
        const double bound = pi == 0 ? 1e-6 : 1e-12;
        if (!(err <= bound)) {
            ++g_fail;
            printf("FAIL numbers %s %s %s n=%u taps=%u R0=%u: rel-L2 %.3e > %.0e\n", pi ? "f64" : "f32", real ? "real" : "complex",
                   prepared ? "prepared" : "taps", g.n, g.taps, g.r0, err, bound);
        }
    }
}

struct LenLine { bool is_taps; long long a, c; unsigned from_r0; };

static void numbers(const std::vector<size_t>& taps_list, const std::vector<LenLine>& lens)
{
    Chain<float> c32;
    Chain<double> c64;
    bool seen_r0[13] = {false};
    for (size_t taps : taps_list) {
        const unsigned r0 = conv_v2_r0(taps);
        if (r0 <= 12) seen_r0[r0] = true;
        const long long V = L - 256 * (long long)r0;
        for (const LenLine& ll : lens) {
            if (r0 < ll.from_r0) continue;
            const long long n = ll.is_taps ? (long long)taps : ll.a * V + ll.c;
            if (n < (long long)taps) continue;
            const Geom g = geom_of((size_t)n, taps);
            for (int real = 0; real < 2; ++real) {
                const ConvV2Plan p = conv_v2_plan((size_t)n, taps, 1, 0, 0, real != 0, 256, 3, -1, -1);
                if (p.status != CONV_V2_PLAN_RUN) { fail("numbers: plan", n, (long long)taps); continue; }
                // the wrap-around blocks at both ends (the first starts before the vector, the last runs past it and is
                // short) and the middle one of the interior blocks
                std::vector<std::pair<unsigned, bool>> blocks;
                if (p.lo > 0) blocks.push_back({0u, false});
                if (p.b1 - 1 >= p.hi && (p.b1 - 1 > 0 || p.lo == 0)) blocks.push_back({(unsigned)(p.b1 - 1), false});
                if (blocks.empty()) { fail("numbers: no wrap-around block", n, (long long)taps); continue; }
                if (p.hi > p.lo) blocks.push_back({(unsigned)(p.lo + (p.hi - p.lo) / 2), true});
                else if (!ll.is_taps && (ll.a >= 9 || (ll.a >= 5 && !(real && r0 >= 11)))) fail("numbers: no interior block", n, (long long)taps, real);
                NumCase nc;
                const size_t e = real ? 1 : 2;
                nc.x.resize(e * (size_t)n);
                nc.h.resize(e * taps);
                for (auto& v : nc.x) v = (float)(10.0 * noise());
                for (auto& v : nc.h) v = (float)(noise() / (double)taps);
                const long long U = real ? 2 : 1;
                for (auto [b, interior] : blocks) {
                    (void)interior;
                    const long long first = (long long)b * U * V, end = std::min<long long>((long long)(b + 1) * U * V, n);
                    nc.ref[b] = direct(nc.x, nc.h, real != 0, n, (long long)taps, first, end);
                }
                numbers_for<float>(c32, g, nc, real != 0, blocks, nc.ref);
                numbers_for<double>(c64, g, nc, real != 0, blocks, nc.ref);
            }
        }
    }
    for (unsigned r = 1; r <= 12; ++r)
        if (!seen_r0[r]) fail("numbers: an R0 without a shape", r);
    printf("numbers: %lld blocks\n", g_blocks);
    printf("numbers: worst rel-L2 per case: f32 %.3e (bound 1e-06), f64 %.3e (bound 1e-12)\n", g_worst[0], g_worst[1]);
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: sim_conv_v2 conv_v2_shapes.txt [geometry|numbers]\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<size_t> taps_list;
    std::vector<LenLine> lens;
    std::vector<Share> overrides;
    char line[512];
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        long long a = 0, b = 0, c = 0;
        if (!strncmp(line, "taps ", 5)) {
            if (sscanf(line + 5, "%lld %lld %lld", &a, &b, &c) != 3) { fail("shapes: taps line"); continue; }
            // the file states R0 and d: they must be the header's
            if ((long long)conv_v2_r0((size_t)a) != b || (long long)conv_v2_delay(256u * (unsigned)b, (unsigned)a) != c) fail("shapes: R0 / d", a, b, c);
            taps_list.push_back((size_t)a);
        } else if (!strncmp(line, "len taps", 8)) lens.push_back({true, 0, 0, 0});
        else if (!strncmp(line, "len ", 4)) {
            const int k = sscanf(line + 4, "%lld %lld %lld", &a, &b, &c);
            if (k < 2) { fail("shapes: len line"); continue; }
            lens.push_back({false, a, b, k == 3 ? (unsigned)c : 0u});
        } else if (!strncmp(line, "share ", 6)) {
            if (sscanf(line + 6, "%lld %lld", &a, &b) != 2) { fail("shapes: share line"); continue; }
            // bdsp_hip_dev_convolve_ex's refusal rule (capi.cpp)
            if (a < 1 || b < 0 || a + b > 99) fail("shapes: a share the library refuses", a, b);
            overrides.push_back({(int)a, (int)b});
        } else fail("shapes: unknown line");
    }
    fclose(f);
    const bool only_geometry = argc > 2 && !strcmp(argv[2], "geometry"), only_numbers = argc > 2 && !strcmp(argv[2], "numbers");
    if (!only_numbers) geometry(overrides);
    if (!only_geometry) numbers(taps_list, lens);
    printf("%lld failures\n", g_fail);
    printf(g_fail ? "FAIL\n" : "ok\n");
    return g_fail ? 1 : 0;
}
