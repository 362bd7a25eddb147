// Host-side checks of the global passes of a power-of-two transform above 4096 points (k_fft_pass, fft_impl.h).
// The rule that picks what is launched -- plan, route of every pass, buffer order, the facade's operations as options --
// is basic_dsp_amd/csrc/fft_plan_core.h, compiled here with the host compiler; the kernel's index maps are walked with
// threads as loops and an array as LDS, through the WgFft templates of fft_core.h the kernel itself calls (as
// sim_fft.cpp does for the workgroup transform).
//   1  tests/fft_pass_shapes.txt against the rule at 256 CUs; every route class the rule can produce has a line
//   2  launch parameters of every route of a sweep
//   3  one pass of every tile against the Stockham iteration it is documented to be (fft_impl.h, above k_fft_pass), with
//      the XCD tile remap and the two shift renamings (every point loaded and stored exactly once); the window lattice
//   4  numbers: whole transforms of 2^13, 2^14 and 2^16 points and 64 x 64 x 64 points against a long double transform
// usage: sim_fft_passes tests/fft_pass_shapes.txt
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../basic_dsp_amd/csrc/fft_core.h"
#include "../../basic_dsp_amd/csrc/fft_plan_core.h"

using namespace bdsp;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (++g_fail <= 40) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                          \
    } while (0)

constexpr int CUS = 256; // the table is written for an MI355X

// ================================================================================================ 1  the route table
static std::string variant_of(const FftPassRoute& r)
{
    std::string v = r.gen ? "gen" : r.simple ? "simple" : r.win_fixed == 0 ? "win0" : r.win_fixed == 2 ? "win2" : "opts";
    if (r.ntl) v += "+ntl";
    return v;
}
static std::string route_text(const FftPlan& p)
{
    if (p.passes == 1) return "wg4";
    std::string s;
    for (int i = 0; i < p.passes; ++i) {
        char b[64];
        snprintf(b, sizeof b, "%s%dx%d:%s", i ? " " : "", p.r[i].rp, p.r[i].w, variant_of(p.r[i]).c_str());
        s += b;
    }
    return s;
}
// a class = one k_fft_pass instantiation: precision, tile, lane map, variant, direction (or the one-workgroup kernel)
static std::string class_of(size_t esz, const FftPassRoute& r)
{
    char b[96];
    snprintf(b, sizeof b, "f%d %dx%d %s %s %s", (int)esz * 8, r.rp, r.w, r.rowmap ? "first" : "later", variant_of(r).c_str(),
             r.dir < 0 ? "fwd" : "inv");
    return b;
}
static void classes_of(size_t esz, const FftPlan& p, bool inverse, std::set<std::string>& out)
{
    if (p.passes == 1) { out.insert(std::string("f32 wg4 ") + (inverse ? "inv" : "fwd")); return; }
    for (int i = 0; i < p.passes; ++i) out.insert(class_of(esz, p.r[i]));
}
struct Options { // what one transform is asked to do
    bool inverse = false, scaled = false;
    unsigned flags = 0;
    int window_id = -1;
    size_t in_stride = 0, out_stride = 0; // 0: n
};
static FftPlan plan_of(size_t esz, size_t n, size_t batch, int cus, const Options& o)
{
    return fft_plan(esz, n, batch, cus, o.flags, o.scaled, o.window_id, o.in_stride ? o.in_stride : n, o.out_stride ? o.out_stride : n,
                    0, o.inverse);
}
template <typename T>
static Options facade(bool inverse, bool shift, int window, bool real, size_t n)
{
    const FftOpArgs<T> a = fft_op_args<T>(inverse, shift, window, real, n);
    Options o;
    o.inverse = inverse; o.flags = a.flags; o.scaled = a.in_scale != (T)1; o.window_id = a.window_id;
    return o;
}
static Options facade_any(size_t esz, bool inverse, bool shift, int window, bool real, size_t n)
{
    return esz == 4 ? facade<float>(inverse, shift, window, real, n) : facade<double>(inverse, shift, window, real, n);
}
// bdsp_hip_dev_fft (capi.cpp): public flags, scale, facade window id
static Options b3(unsigned pub, bool scaled, int window)
{
    Options o;
    o.inverse = (pub & BDSP_FFT_INVERSE) != 0;
    o.flags = pub & (BDSP_FFT_SHIFT_OUT | BDSP_FFT_SHIFT_IN | BDSP_FFT_MAGNITUDE);
    o.scaled = scaled;
    double alpha;
    if (window >= 0) map_window<double>(window, &o.window_id, &alpha);
    return o;
}
static int window_by_name(const std::string& s)
{
    if (s == "triangular") return 0;
    if (s == "hamming") return 1;
    if (s == "blackman_harris") return 2;
    if (s == "rectangular") return 3;
    if (s == "hann") return 4;
    return -2;
}
// the operation of a vec / mat line
static bool parse_op(const std::string& op, size_t esz, size_t n, Options* o)
{
    std::string name = op, arg;
    const size_t colon = op.find(':');
    if (colon != std::string::npos) { name = op.substr(0, colon); arg = op.substr(colon + 1); }
    bool real = false;
    if (name.rfind("real_", 0) == 0) { real = true; name = name.substr(5); }
    int window = -1;
    if (name == "windowed_fft" || name == "windowed_ifft") {
        window = window_by_name(arg);
        if (window < 0) return false;
    } else if (!arg.empty()) return false;
    if (name == "plain_fft") *o = facade_any(esz, false, false, -1, real, n);
    else if (name == "fft") *o = facade_any(esz, false, true, -1, real, n);
    else if (name == "windowed_fft") *o = facade_any(esz, false, true, window, real, n);
    else if (name == "plain_ifft") *o = facade_any(esz, true, false, -1, real, n);
    else if (name == "ifft") *o = facade_any(esz, true, true, -1, real, n);
    else if (name == "windowed_ifft") *o = facade_any(esz, true, true, window, real, n);
    // op_custom_windowed (capi.cpp): the table multiply is a launch of its own before fft() / after ifft()
    else if (name == "windowed_custom_fft") *o = facade_any(esz, false, true, -1, real, n);
    else if (name == "windowed_custom_ifft") *o = facade_any(esz, true, true, -1, real, n);
    else return false;
    return true;
}
static bool parse_kv(const std::string& s, std::map<std::string, std::string>& kv)
{
    size_t p = 0;
    while (p < s.size()) {
        size_t c = s.find(',', p);
        if (c == std::string::npos) c = s.size();
        const std::string item = s.substr(p, c - p);
        const size_t e = item.find('=');
        if (e == std::string::npos) return false;
        kv[item.substr(0, e)] = item.substr(e + 1);
        p = c + 1;
    }
    return true;
}

static const char* buffers_text(int order) { return order == FFT_BUF_ABA ? "aba" : order == FFT_BUF_ABB ? "abb" : "abab"; }

static void check_table(const char* path, std::set<std::string>& witnessed)
{
    FILE* f = fopen(path, "r");
    if (!f) { printf("FAIL cannot open %s\n", path); ++g_fail; return; }
    char buf[512];
    int lineno = 0, lines = 0;
    std::set<std::string> seen;
    while (fgets(buf, sizeof buf, f)) {
        ++lineno;
        std::vector<std::string> w;
        for (char* t = strtok(buf, " \t\r\n"); t; t = strtok(nullptr, " \t\r\n")) w.push_back(t);
        if (w.empty() || w[0][0] == '#') continue;
        ++lines;
        size_t arrow = 0;
        while (arrow < w.size() && w[arrow] != "->") ++arrow;
        if (arrow != 5 || w.size() < 8) { CHECK(false, "line %d: not `dtype bits batch entry op -> route buffers`", lineno); continue; }
        const size_t esz = w[0] == "f32" ? 4 : w[0] == "f64" ? 8 : 0;
        const int bits = atoi(w[1].c_str());
        const size_t batch = (size_t)atoll(w[2].c_str());
        CHECK(esz && bits >= 13 && bits <= 23 && batch >= 1, "line %d: dtype / bits (13..23) / batch", lineno);
        if (!esz || bits < 13 || bits > 23 || batch < 1) continue;
        const size_t n = size_t(1) << bits;
        const std::string key = w[0] + " " + w[1] + " " + w[2] + " " + w[3] + " " + w[4];
        CHECK(seen.insert(key).second, "line %d: repeated", lineno);
        bool cu = w.back() == "cu256";
        const size_t end = w.size() - (cu ? 1 : 0);
        std::string stated;
        for (size_t i = arrow + 1; i + 1 < end; ++i) stated += (i > arrow + 1 ? " " : "") + w[i];
        const std::string stated_buf = w[end - 1];
        Options o;
        std::string want_buf;
        bool ok = true;
        if (w[3] == "vec" || w[3] == "mat") {
            ok = parse_op(w[4], esz, n, &o) && (w[3] == "mat" || batch == 1);
        } else if (w[3] == "dev") {
            std::map<std::string, std::string> kv;
            ok = parse_kv(w[4], kv) && kv.count("flags") && kv.count("scale") && kv.count("window") && kv.size() == 3 &&
                 (kv["scale"] == "1" || kv["scale"] == "1/n");
            if (ok) o = b3((unsigned)atoi(kv["flags"].c_str()), kv["scale"] != "1", atoi(kv["window"].c_str()));
        } else if (w[3] == "conv") {
            // conv_long_dev (capi.cpp): blocks of L = next_pow2(4 (M-1)) >= 8192 points, V = L - (M-1) apart, all blocks of the
            // signal in one strided forward transform
            std::map<std::string, std::string> kv;
            ok = parse_kv(w[4], kv) && kv.count("taps") && kv.count("points") && kv.size() == 2;
            if (ok) {
                const size_t taps = (size_t)atoll(kv["taps"].c_str()), points = (size_t)atoll(kv["points"].c_str());
                size_t L = 8192;
                while (L < 4 * (taps - 1)) L <<= 1;
                const size_t V = L - (taps - 1);
                ok = taps > 3073 && taps <= points && points <= (size_t(1) << 22) && L == n && (points + V - 1) / V == batch;
                o.in_stride = V;
                want_buf = "xba"; // the extended signal, scratch, result
                CHECK(plan_pass_count(n, esz) == 2, "line %d: conv lines are two-pass lengths", lineno);
            }
        } else ok = false;
        CHECK(ok, "line %d: entry / operation not understood or inconsistent: %s", lineno, key.c_str());
        if (!ok) continue;
        const FftPlan p = plan_of(esz, n, batch, CUS, o);
        if (want_buf.empty()) want_buf = p.passes == 1 ? "aa" : buffers_text(fft_buffer_order(esz, n, o.flags));
        const std::string got = route_text(p);
        CHECK(got == stated && want_buf == stated_buf, "line %d: %s: stated `%s %s`, the rule gives `%s %s`", lineno, key.c_str(),
              stated.c_str(), stated_buf.c_str(), got.c_str(), want_buf.c_str());
        // CU-dependent lines say so: the route differs at some other CU count
        bool dep = false;
        for (int c : {1, 8, 64, 104, 304, 1024}) dep = dep || route_text(plan_of(esz, n, batch, c, o)) != got;
        CHECK(dep == cu, "line %d: %s: cu256 mark %s", lineno, key.c_str(), dep ? "missing" : "not needed");
        classes_of(esz, p, o.inverse, witnessed);
    }
    fclose(f);
    printf("table: %d lines, %d route classes witnessed\n", lines, (int)witnessed.size());
}

// ================================================================================================ 2  sweep of the rule
static void check_launch(size_t esz, size_t n, size_t batch, const FftPlan& p)
{
    CHECK(p.passes >= 1 && p.passes <= 3, "passes %d", p.passes);
    if (p.passes < 2) return;
    size_t prod = 1;
    for (int i = 0; i < p.passes; ++i) {
        const FftPassRoute& r = p.r[i];
        prod *= (size_t)r.rp;
        CHECK(pass_tile_built(esz, r.rp, r.w), "f%d n=%zu: tile %dx%d is not instantiated", (int)esz * 8, n, r.rp, r.w);
        CHECK(!pass_first_only_rt(r.rp) || i == 0, "f%d n=%zu: first-only tile %dx%d as pass %d", (int)esz * 8, n, r.rp, r.w, i);
        CHECK(r.rowmap == (i == 0) && r.last == (i == p.passes - 1), "first / last flags");
        CHECK(r.lds_bytes <= 160 * 1024, "f%d %dx%d: %zu bytes of LDS", (int)esz * 8, r.rp, r.w, r.lds_bytes);
        CHECK(r.grid * (size_t)r.w * (size_t)r.rp == n * batch && r.grid > 0, "f%d n=%zu batch=%zu %dx%d: grid %zu", (int)esz * 8, n, batch, r.rp, r.w, r.grid);
        CHECK(r.threads <= 1024 && r.threads == r.w * (r.rp / 16) && r.threads % 64 == 0, "threads %d", r.threads);
        CHECK(r.tiles_per_vec * batch == r.grid, "tiles per vector");
        CHECK(!(r.gen && (r.simple || r.ntl || r.split || r.win_fixed >= 0)), "gen excludes the other variants");
        CHECK(!(r.simple && r.win_fixed >= 0), "simple excludes a window");
        CHECK(r.win_fixed < 0 || r.split, "fixed windows on split tiles only");
        CHECK(!(r.split && r.lds_twiddles), "a split tile has no room for the table");
        CHECK(!r.ntl || (r.rowmap && esz == 8), "non-temporal loads: f64 first passes");
        CHECK(i == 0 || i == p.passes - 1 || r.simple, "a middle pass looks at no option");
    }
    CHECK(prod == n, "f%d n=%zu: the super-radices multiply to %zu", (int)esz * 8, n, prod);
}

static std::vector<Options> all_options(size_t esz, size_t n)
{
    std::vector<Options> v;
    // the facade (op_fft, capi.cpp): six operations, five windows, complex and real vectors
    for (int real = 0; real < 2; ++real)
        for (int inverse = 0; inverse < 2; ++inverse)
            for (int shift = 0; shift < 2; ++shift)
                for (int window = -1; window <= 4; ++window) v.push_back(facade_any(esz, inverse, shift, window, real, n));
    // B3 (bdsp_hip_dev_fft): every public flag combination, with and without a scale, every window id
    for (unsigned pub = 0; pub < 16; ++pub)
        for (int scaled = 0; scaled < 2; ++scaled)
            for (int window = -1; window <= 5; ++window) v.push_back(b3(pub, scaled, window));
    // the library's own callers of fft_two_buffers: real-part output of an inverse transform (sifft, interpolation,
    // resampling), inverse + fft_shift + scale (correlation)
    for (int scaled = 0; scaled < 2; ++scaled) {
        Options o;
        o.inverse = true; o.scaled = scaled; o.flags = FFT_OUT_REAL;
        v.push_back(o);
        o.flags = BDSP_FFT_SHIFT_OUT;
        v.push_back(o);
    }
    // overlapping windows of a signal (conv_long_dev and the host-slice convolution): strided input, forward
    Options o;
    o.in_stride = n - 3073;
    v.push_back(o);
    return v;
}

static void sweep(const std::set<std::string>& witnessed)
{
    std::set<std::string> all, low; // every class; those the sweep itself reaches at or below 2^23 points
    size_t plans = 0;
    for (size_t esz : {size_t(4), size_t(8)})
        for (int bits = 13; bits <= 30; ++bits)
            for (size_t batch : {size_t(1), size_t(3), size_t(8), size_t(64), size_t(4096)}) {
                const size_t n = size_t(1) << bits;
                for (const Options& o : all_options(esz, n))
                    for (int cus : {CUS, 8, 304}) {
                        const FftPlan p = plan_of(esz, n, batch, cus, o);
                        check_launch(esz, n, batch, p);
                        CHECK(p.passes == 1 || p.passes == plan_pass_count(n, esz), "the pass count depends on n and the precision only");
                        ++plans;
                        if (cus != CUS) continue;
                        classes_of(esz, p, o.inverse, all);
                        if (bits <= 23) classes_of(esz, p, o.inverse, low);
                    }
            }
    int missing = 0, high = 0;
    for (const std::string& c : all) {
        if (!low.count(c)) { ++high; printf("class reachable above 2^23 points only: %s\n", c.c_str()); continue; }
        if (!witnessed.count(c)) { ++missing; CHECK(false, "no line of the table reaches the class `%s`", c.c_str()); }
    }
    for (const std::string& c : witnessed) CHECK(all.count(c), "the table reaches a class the sweep does not: %s", c.c_str());
    printf("sweep: %zu plans, %d route classes, %d without a witness at or below 2^23 points, %d without a line\n", plans,
           (int)all.size(), high, missing);
    CHECK(plan_pass_count(size_t(1) << 31, 4) == 0, "above 2^30 points there is no plan");
}

// ================================================================================================ 3  one pass on the host
typedef long double ld;
struct cld { ld x, y; };
static void fft_ld(std::vector<cld>& a, int dir) // iterative radix-2, long double, unnormalised
{
    const size_t n = a.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    const ld pi = acosl(-1.0L);
    for (size_t len = 2; len <= n; len <<= 1) {
        std::vector<cld> w(len / 2);
        for (size_t k = 0; k < len / 2; ++k) w[k] = {cosl(2 * pi * k / len), dir * sinl(2 * pi * k / len)};
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const cld u = a[i + k], v = a[i + k + len / 2];
                const cld t = {v.x * w[k].x - v.y * w[k].y, v.x * w[k].y + v.y * w[k].x};
                a[i + k] = {u.x + t.x, u.y + t.y};
                a[i + k + len / 2] = {u.x - t.x, u.y - t.y};
            }
    }
}

template <typename T>
static cpx<T> unit_root_host(size_t e, size_t n) // the kernel's unit_root: exp(-2 pi i e / n), rounded once
{
    const ld a = 2 * acosl(-1.0L) * (ld)e / (ld)n;
    return cpx<T>{(T)cosl(a), (T)-sinl(a)};
}
template <typename T>
static std::vector<cpx<T>> twiddle_table_host(int n)
{
    std::vector<cpx<T>> t(n);
    for (int m = 0; m < n; ++m) t[m] = unit_root_host<T>((size_t)m, (size_t)n);
    return t;
}

struct PassOpts {
    bool shift_in = false, shift_out = false, last = false;
};

// k_fft_pass, plain I/O (no GEN), with threads as loops: the same statements in the same order, `tid` looped between
// the barriers.  SPLIT as the kernel derives it.  Returns through dst; load_idx / store_idx (optional) record the global
// index every (block, thread, register) touched.
template <typename T, int RP, int W, int DIR, bool ROWMAP>
static void sim_pass(const cpx<T>* src, cpx<T>* dst, size_t n, size_t nsg, size_t batch, const PassOpts& o,
                     std::vector<size_t>* load_idx = nullptr, std::vector<size_t>* store_idx = nullptr)
{
    constexpr int NT = RP / 16;
    constexpr int CS = col_stride(RP, W);
    constexpr int THREADS = W * NT;
    using F = WgFft<T, RP, NT>;
    using P = Radix16Plan<RP>;
    constexpr bool SPLIT = pass_split_exchange<T, RP, W, false>();
    static_assert(F::LDS_ELEMS <= CS, "a column fits its LDS region");
    const std::vector<cpx<T>> wtab = twiddle_table_host<T>(RP);
    auto tw = [&](int m) { return wtab[m]; };
    const size_t tiles_per_vec = (n / RP) / W;
    const size_t grid = tiles_per_vec * batch;
    std::vector<std::array<cpx<T>, 16>> regs(THREADS);
    std::vector<cpx<T>> lds((size_t)W * CS);
    std::vector<T> ldsr((size_t)W * CS);
    if (load_idx) load_idx->assign(grid * THREADS * 16, (size_t)-1);
    if (store_idx) store_idx->assign(grid * THREADS * 16, (size_t)-1);
    for (size_t blk = 0; blk < grid; ++blk) {
        const size_t vec = blk / tiles_per_vec;
        size_t tile = blk % tiles_per_vec;
        if ((tiles_per_vec & 7) == 0) tile = (tile & 7) * (tiles_per_vec >> 3) + (tile >> 3);
        const size_t j0 = tile * W;
        const size_t stride_in = n / RP;
        // ---- load
        for (int tid = 0; tid < THREADS; ++tid) {
            cpx<T>(&v)[16] = *reinterpret_cast<cpx<T>(*)[16]>(regs[tid].data());
            const int c = tid % W, ti = tid / W;
            const size_t j = j0 + c;
            const cpx<T>* in = src + vec * n + j;
            const int rx = (ROWMAP && o.shift_in) ? 8 : 0;
            for (int r = 0; r < 16; ++r) {
                const size_t off = (size_t)(ti + (r ^ rx) * NT) * stride_in;
                v[r] = in[off];
                if (load_idx) (*load_idx)[(blk * THREADS + tid) * 16 + r] = vec * n + j + off;
            }
            if (!ROWMAP) {
                const size_t k = j % nsg;
                const size_t q = k * (n / (nsg * RP));
                const cpx<T> bs = unit_root_host<T>(((size_t)ti * q) & (n - 1), n);
                const cpx<T> d1 = unit_root_host<T>(((size_t)NT * q) & (n - 1), n);
                for (int r = 0; r < 16; ++r) v[r] = twmul<DIR>(v[r], bs);
                const cpx<T> held[2] = {cmul(d1, d1), d1};
                cpx<T> t8[8];
                expand_twiddles16_fma<2>(held, t8);
                dft16_tw<DIR>(&v[0], t8);
            } else {
                F::template compute<16, 1, DIR>(v, ti, tw);
            }
        }
        // ---- RP-point sub-FFT of every column
        auto ids = [&](int tid, int& c, int& ti, int& c2, int& t2) {
            c = tid % W; ti = tid / W;
            c2 = ROWMAP ? tid / NT : tid % W;
            t2 = ROWMAP ? tid % NT : tid / W;
        };
        if constexpr (SPLIT) {
            for (int part = 0; part < 2; ++part) {
                for (int tid = 0; tid < THREADS; ++tid) {
                    int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                    cpx<T>* v = regs[tid].data();
                    if (part == 0) F::template scatter<16, 1>(PartRef<cpx<T>, false>{v}, ti, ldsr.data() + (size_t)c * CS);
                    else F::template scatter<16, 1>(PartRef<cpx<T>, true>{v}, ti, ldsr.data() + (size_t)c * CS);
                }
                // (the gather of the real parts writes v[].x only: the imaginary parts are still there for their scatter)
                for (int tid = 0; tid < THREADS; ++tid) {
                    int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                    cpx<T>* v = regs[tid].data();
                    if (part == 0) F::template gather<P::R2>(PartRef<cpx<T>, false>{v}, t2, ldsr.data() + (size_t)c2 * CS);
                    else F::template gather<P::R2>(PartRef<cpx<T>, true>{v}, t2, ldsr.data() + (size_t)c2 * CS);
                }
            }
        } else {
            for (int tid = 0; tid < THREADS; ++tid) {
                int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                cpx<T>(&v)[16] = *reinterpret_cast<cpx<T>(*)[16]>(regs[tid].data());
                F::template scatter<16, 1>(v, ti, lds.data() + (size_t)c * CS);
            }
            for (int tid = 0; tid < THREADS; ++tid) {
                int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                cpx<T>(&v)[16] = *reinterpret_cast<cpx<T>(*)[16]>(regs[tid].data());
                F::template gather<P::R2>(v, t2, lds.data() + (size_t)c2 * CS);
            }
        }
        for (int tid = 0; tid < THREADS; ++tid) {
            int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
            cpx<T>(&v)[16] = *reinterpret_cast<cpx<T>(*)[16]>(regs[tid].data());
            F::template compute<P::R2, 16, DIR>(v, t2, tw);
        }
        if constexpr (P::R3 > 1) {
            if constexpr (SPLIT) {
                for (int part = 0; part < 2; ++part) {
                    for (int tid = 0; tid < THREADS; ++tid) {
                        int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                        cpx<T>* v = regs[tid].data();
                        if (part == 0) F::template scatter<P::R2, 16>(PartRef<cpx<T>, false>{v}, t2, ldsr.data() + (size_t)c2 * CS);
                        else F::template scatter<P::R2, 16>(PartRef<cpx<T>, true>{v}, t2, ldsr.data() + (size_t)c2 * CS);
                    }
                    for (int tid = 0; tid < THREADS; ++tid) {
                        int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                        cpx<T>* v = regs[tid].data();
                        if (part == 0) F::template gather<P::R3>(PartRef<cpx<T>, false>{v}, t2, ldsr.data() + (size_t)c2 * CS);
                        else F::template gather<P::R3>(PartRef<cpx<T>, true>{v}, t2, ldsr.data() + (size_t)c2 * CS);
                    }
                }
            } else {
                for (int tid = 0; tid < THREADS; ++tid) {
                    int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                    cpx<T>(&v)[16] = *reinterpret_cast<cpx<T>(*)[16]>(regs[tid].data());
                    F::template scatter<P::R2, 16>(v, t2, lds.data() + (size_t)c2 * CS);
                }
                for (int tid = 0; tid < THREADS; ++tid) {
                    int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                    cpx<T>(&v)[16] = *reinterpret_cast<cpx<T>(*)[16]>(regs[tid].data());
                    F::template gather<P::R3>(v, t2, lds.data() + (size_t)c2 * CS);
                }
            }
            for (int tid = 0; tid < THREADS; ++tid) {
                int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
                cpx<T>(&v)[16] = *reinterpret_cast<cpx<T>(*)[16]>(regs[tid].data());
                F::template compute<P::R3, 16 * P::R2, DIR>(v, t2, tw);
            }
        }
        // ---- autosorted store
        constexpr int RL = P::R3 > 1 ? P::R3 : P::R2;
        constexpr int NSL = RP / RL;
        for (int tid = 0; tid < THREADS; ++tid) {
            int c, ti, c2, t2; ids(tid, c, ti, c2, t2);
            const cpx<T>* v = regs[tid].data();
            const size_t jj = j0 + c2;
            const size_t base = (jj / nsg) * nsg * RP + (jj % nsg);
            cpx<T>* out = dst + vec * n + base;
            const int sx = (o.last && !ROWMAP && o.shift_out) ? RL / 2 : 0;
            for (int b = 0; b < 16 / RL; ++b)
                for (int r = 0; r < RL; ++r) {
                    const size_t off = (size_t)F::template out_index<RL, NSL>(t2, b, r ^ sx) * nsg;
                    out[off] = v[b * RL + r];
                    if (store_idx) (*store_idx)[(blk * THREADS + tid) * 16 + b * RL + r] = vec * n + base + off;
                }
        }
    }
}

template <typename T>
static void fill_random(std::vector<cpx<T>>& x, unsigned seed)
{
    srand(seed);
    for (auto& v : x) v = {(T)(rand() / (double)RAND_MAX * 20 - 10), (T)(rand() / (double)RAND_MAX * 20 - 10)};
}

// The Stockham iteration a pass is documented to be, in long double, from the same input:
//   column j, k = j mod nsg: v[row] = in[j + row n/RP] w_{nsg RP}^{row k}; v = DFT_RP(v); out[(j/nsg) nsg RP + k + row nsg] = v[row]
// with the ifft_shift of the input (a rotation by n/2 before) and the fft_shift of the output (a rotation by n/2 after).
template <typename T>
static double pass_error(const std::vector<cpx<T>>& in, const std::vector<cpx<T>>& got, int rp, size_t n, size_t nsg, size_t batch,
                         int dir, bool shift_in, bool shift_out)
{
    const ld pi = acosl(-1.0L);
    ld num = 0, den = 0;
    std::vector<cld> col((size_t)rp);
    for (size_t vec = 0; vec < batch; ++vec)
        for (size_t j = 0; j < n / rp; ++j) {
            const size_t k = j % nsg;
            for (int row = 0; row < rp; ++row) {
                size_t i = j + (size_t)row * (n / rp);
                if (shift_in) i = (i + n / 2) % n;
                const ld a = dir * 2 * pi * (ld)(((size_t)row * k) % (nsg * rp)) / (ld)(nsg * rp);
                const ld c = cosl(a), s = sinl(a);
                const cpx<T> x = in[vec * n + i];
                col[row] = {x.x * c - x.y * s, x.x * s + x.y * c};
            }
            fft_ld(col, dir);
            for (int row = 0; row < rp; ++row) {
                size_t p = (j / nsg) * nsg * rp + k + (size_t)row * nsg;
                if (shift_out) p = (p + n / 2) % n;
                const cpx<T> g = got[vec * n + p];
                const ld dx = g.x - col[row].x, dy = g.y - col[row].y;
                num += dx * dx + dy * dy;
                den += col[row].x * col[row].x + col[row].y * col[row].y;
            }
        }
    return (double)sqrtl(num / den);
}

static bool is_permutation(const std::vector<size_t>& idx, size_t total)
{
    if (idx.size() != total) return false;
    std::vector<char> hit(total, 0);
    for (size_t i : idx) {
        if (i >= total || hit[i]) return false;
        hit[i] = 1;
    }
    return true;
}

static double g_worst_pass[2] = {0, 0};

template <typename T, int RP, int W, bool ROWMAP>
static void check_tile()
{
    // eight tiles per vector (the XCD remap is on), two vectors.  combo 0: forward; a later pass over two groups of
    // nsg = 4 W columns.  combo 1: inverse with the shift; a later pass as the LAST one (nsg RP = n: only there is r ^ sx a
    // rotation of the result, and only there does a workgroup read and write the same index set -- the in-place last
    // pass of a -> b -> b).
    const size_t batch = 2;
    const size_t n = (size_t)8 * W * RP;
    const double tol = sizeof(T) == 4 ? 1e-6 : 1e-12;
    std::vector<cpx<T>> in(n * batch), out(n * batch);
    fill_random<T>(in, (unsigned)(RP * 31 + W + (ROWMAP ? 7 : 0)));
    for (int combo = 0; combo < 2; ++combo) {
        const size_t nsg = ROWMAP ? 1 : combo == 0 ? (size_t)4 * W : n / RP;
        PassOpts o;
        o.last = true;
        o.shift_in = combo == 1 && ROWMAP;
        o.shift_out = combo == 1 && !ROWMAP;
        std::vector<size_t> li, si;
        std::fill(out.begin(), out.end(), cpx<T>{0, 0});
        if (combo == 0) sim_pass<T, RP, W, -1, ROWMAP>(in.data(), out.data(), n, nsg, batch, o, &li, &si);
        else sim_pass<T, RP, W, 1, ROWMAP>(in.data(), out.data(), n, nsg, batch, o, &li, &si);
        CHECK(is_permutation(li, n * batch), "f%d %dx%d %s: every input point is loaded exactly once", (int)sizeof(T) * 8, RP, W, ROWMAP ? "first" : "later");
        CHECK(is_permutation(si, n * batch), "f%d %dx%d %s: every output point is stored exactly once", (int)sizeof(T) * 8, RP, W, ROWMAP ? "first" : "later");
        if (!ROWMAP && combo == 1) {
            const size_t per = (size_t)W * RP;
            for (size_t blk = 0; blk < li.size() / per; ++blk) {
                std::vector<size_t> a(li.begin() + blk * per, li.begin() + (blk + 1) * per), b(si.begin() + blk * per, si.begin() + (blk + 1) * per);
                std::sort(a.begin(), a.end());
                std::sort(b.begin(), b.end());
                CHECK(a == b, "f%d %dx%d last: block %zu reads and writes different index sets", (int)sizeof(T) * 8, RP, W, blk);
            }
        }
        const double e = pass_error<T>(in, out, RP, n, nsg, batch, combo == 0 ? -1 : 1, o.shift_in, o.shift_out);
        g_worst_pass[sizeof(T) == 8] = std::max(g_worst_pass[sizeof(T) == 8], e);
        CHECK(e < tol, "f%d %dx%d %s %s: one pass against the Stockham iteration: rel-L2 %.3e", (int)sizeof(T) * 8, RP, W,
              ROWMAP ? "first" : "later", combo ? "inverse + shift" : "forward", e);
    }
    // the XCD remap is a bijection on the tiles of a vector, and the identity where their count is no multiple of 8
    for (size_t tpv : {size_t(8), size_t(16), size_t(64), size_t(4), size_t(12), size_t(1)}) {
        std::vector<char> hit(tpv, 0);
        bool ok = true;
        for (size_t t = 0; t < tpv; ++t) {
            size_t tile = t;
            if ((tpv & 7) == 0) tile = (tile & 7) * (tpv >> 3) + (tile >> 3);
            else ok = ok && tile == t;
            ok = ok && tile < tpv && !hit[tile];
            if (tile < tpv) hit[tile] = 1;
        }
        CHECK(ok, "XCD remap of %zu tiles", tpv);
    }
    // without the remap's condition met: four tiles per vector (one tile's columns per group of nsg)
    {
        const size_t n4 = (size_t)4 * W * RP, nsg4 = ROWMAP ? 1 : (size_t)W;
        std::vector<cpx<T>> in4(n4), out4(n4);
        fill_random<T>(in4, 99u + RP);
        PassOpts o;
        o.last = true;
        sim_pass<T, RP, W, -1, ROWMAP>(in4.data(), out4.data(), n4, nsg4, 1, o);
        const double e = pass_error<T>(in4, out4, RP, n4, nsg4, 1, -1, false, false);
        g_worst_pass[sizeof(T) == 8] = std::max(g_worst_pass[sizeof(T) == 8], e);
        CHECK(e < tol, "f%d %dx%d %s, four tiles: rel-L2 %.3e", (int)sizeof(T) * 8, RP, W, ROWMAP ? "first" : "later", e);
    }
}

// The window lattice: pass_window16 is handed the point i0 of a thread and a function lattice(reg) -> m and takes register
// `reg` to hold point i0 + m n/16 (mirrored for m >= 8).  First pass: i0 = j + ti n/RP, lattice(r) = r ^ rx; last pass:
// i0 = jj + t2 nsg, lattice(reg) = reg / RL + ((reg % RL) ^ sx) (16 / RL) (fft_impl.h, the two lambdas).  The element a
// register holds sits, in the vector the window is defined on, where io_load reads it (after ifft_shift: the window
// multiplies what was loaded, at the index it was loaded from) and where io_store puts it (after fft_shift).
template <int RP, int W>
static void check_window_lattice()
{
    constexpr int NT = RP / 16;
    using F = WgFft<float, RP, NT>;
    using P = Radix16Plan<RP>;
    constexpr int RL = P::R3 > 1 ? P::R3 : P::R2;
    constexpr int NSL = RP / RL;
    for (int bits_more : {3, 5}) {
        const size_t n = (size_t)RP * W << bits_more;
        for (int shift = 0; shift < 2; ++shift) {
            // first pass
            const size_t stride_in = n / RP;
            const int rx = shift ? 8 : 0;
            for (size_t tile : {size_t(0), n / RP / W - 1})
                for (int tid = 0; tid < W * NT; ++tid) {
                    const int c = tid % W, ti = tid / W;
                    const size_t j = tile * W + c;
                    const size_t i0 = j + (size_t)ti * stride_in;
                    CHECK(i0 < n / 16, "%dx%d first: i0 %zu", RP, W, i0);
                    for (int r = 0; r < 16; ++r) {
                        const int m = r ^ rx;
                        const size_t loaded = j + (size_t)(ti + (r ^ rx) * NT) * stride_in; // k_fft_pass's load of register r
                        CHECK(loaded == i0 + (size_t)m * (n / 16), "%dx%d first, shift %d: register %d", RP, W, shift, r);
                        // ... and the ifft_shift itself: register r is input point i of the transform (WgFft::in_index) and is
                        // read from (i + n/2) mod n, as io_load does
                        const size_t i = j + (size_t)F::template in_index<16>(ti, 0, r) * stride_in;
                        CHECK(loaded == (shift ? (i + n / 2) % n : i), "%dx%d first: r ^ rx is a rotation by n/2", RP, W);
                    }
                }
            // last pass: nsg = n / RP
            const size_t nsg = n / RP;
            const int sx = shift ? RL / 2 : 0;
            for (size_t tile : {size_t(0), nsg / W - 1})
                for (int tid = 0; tid < W * NT; ++tid) {
                    const int c2 = tid % W, t2 = tid / W;
                    const size_t jj = tile * W + c2;
                    const size_t base = (jj / nsg) * nsg * RP + (jj % nsg);
                    const size_t i0 = jj + (size_t)t2 * nsg;
                    CHECK(i0 < n / 16, "%dx%d last: i0 %zu", RP, W, i0);
                    for (int reg = 0; reg < 16; ++reg) {
                        const int b = reg / RL, r = reg % RL;
                        const int m = reg / RL + ((reg % RL) ^ sx) * (16 / RL);
                        const size_t stored = base + (size_t)F::template out_index<RL, NSL>(t2, b, r ^ sx) * nsg;
                        CHECK(stored == i0 + (size_t)m * (n / 16), "%dx%d last, shift %d: register %d", RP, W, shift, reg);
                        // ... and the fft_shift itself: the unshifted position of the same register, rotated by n/2
                        const size_t plain = base + (size_t)F::template out_index<RL, NSL>(t2, b, r) * nsg;
                        if (shift) CHECK(stored == (plain + n / 2) % n, "%dx%d last: r ^ sx is a rotation by n/2", RP, W);
                    }
                }
        }
    }
}

// ================================================================================================ 4  whole transforms
template <typename T>
static double transform_error(const std::vector<cpx<T>>& x, const std::vector<cpx<T>>& got, int dir)
{
    std::vector<cld> ref(x.size());
    for (size_t i = 0; i < x.size(); ++i) ref[i] = {x[i].x, x[i].y};
    fft_ld(ref, dir);
    ld num = 0, den = 0;
    for (size_t i = 0; i < x.size(); ++i) {
        const ld dx = got[i].x - ref[i].x, dy = got[i].y - ref[i].y;
        num += dx * dx + dy * dy;
        den += ref[i].x * ref[i].x + ref[i].y * ref[i].y;
    }
    return (double)sqrtl(num / den);
}
template <typename T, int RP, int W, int DIR>
static void run_pass(const std::vector<cpx<T>>& a, std::vector<cpx<T>>& b, size_t n, size_t nsg, bool last)
{
    PassOpts o;
    o.last = last;
    if (nsg == 1) sim_pass<T, RP, W, DIR, true>(a.data(), b.data(), n, nsg, 1, o);
    else sim_pass<T, RP, W, DIR, false>(a.data(), b.data(), n, nsg, 1, o);
}
template <typename T, int DIR>
static double whole(int bits)
{
    const size_t n = size_t(1) << bits;
    std::vector<cpx<T>> x(n), a(n), b(n);
    fill_random<T>(x, 1000u + bits + (DIR > 0 ? 50 : 0));
    int rp[3], w[3];
    const int passes = plan_passes(n, 1, sizeof(T), CUS, rp, w);
    // the plain variants of the plans of these lengths
    if (bits == 13) { // 128 x 32, 64 x 64
        if (passes != 2 || rp[0] != 128 || w[0] != 32 || rp[1] != 64 || w[1] != 64) { CHECK(false, "plan of 2^13"); return 1; }
        run_pass<T, 128, 32, DIR>(x, a, n, 1, false);
        run_pass<T, 64, 64, DIR>(a, b, n, 128, true);
    } else if (bits == 14) { // 128 x 32 twice
        if (passes != 2 || rp[0] != 128 || w[0] != 32 || rp[1] != 128 || w[1] != 32) { CHECK(false, "plan of 2^14"); return 1; }
        run_pass<T, 128, 32, DIR>(x, a, n, 1, false);
        run_pass<T, 128, 32, DIR>(a, b, n, 128, true);
    } else if (bits == 16) { // 256 x 16 twice
        if (passes != 2 || rp[0] != 256 || w[0] != 16 || rp[1] != 256 || w[1] != 16) { CHECK(false, "plan of 2^16"); return 1; }
        run_pass<T, 256, 16, DIR>(x, a, n, 1, false);
        run_pass<T, 256, 16, DIR>(a, b, n, 256, true);
    } else { // 64 x 64 x 64: three passes, a -> b -> a -> b
        std::vector<cpx<T>> c(n);
        run_pass<T, 64, 64, DIR>(x, a, n, 1, false);
        run_pass<T, 64, 64, DIR>(a, c, n, 64, false);
        run_pass<T, 64, 64, DIR>(c, b, n, 64 * 64, true);
    }
    return transform_error<T>(x, b, DIR);
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: %s fft_pass_shapes.txt\n", argv[0]); return 2; }
    std::set<std::string> witnessed;
    check_table(argv[1], witnessed);
    sweep(witnessed);

    // every tile launch_pass_rp instantiates, in both lane maps (4096 x 4: first pass only, f32 only)
    check_tile<float, 64, 64, true>();    check_tile<float, 64, 64, false>();
    check_tile<float, 128, 32, true>();   check_tile<float, 128, 32, false>();
    check_tile<float, 256, 16, true>();   check_tile<float, 256, 16, false>();
    check_tile<float, 512, 8, true>();    check_tile<float, 512, 8, false>();
    check_tile<float, 1024, 4, true>();   check_tile<float, 1024, 4, false>();
    check_tile<float, 1024, 8, true>();   check_tile<float, 1024, 8, false>();
    check_tile<float, 2048, 4, true>();   check_tile<float, 2048, 4, false>();
    check_tile<float, 4096, 4, true>();
    // f64: the index maps are the f32 ones except on the split tiles, which cross real and imaginary parts separately
    static_assert(pass_split_exchange<double, 2048, 4, false>() && pass_split_exchange<double, 1024, 8, false>(), "split tiles");
    static_assert(!pass_split_exchange<double, 1024, 4, false>() && !pass_split_exchange<double, 512, 8, false>() &&
                  !pass_split_exchange<float, 4096, 4, false>(), "whole-complex tiles");
    check_tile<double, 1024, 8, true>();  check_tile<double, 1024, 8, false>();
    check_tile<double, 2048, 4, true>();  check_tile<double, 2048, 4, false>();
    check_tile<double, 256, 16, true>();  check_tile<double, 256, 16, false>();
    check_tile<double, 128, 32, true>();  check_tile<double, 128, 32, false>();
    printf("tiles: 23 (tile, lane map) pairs, worst rel-L2 of one pass: f32 %.3e (bound 1e-06), f64 %.3e (bound 1e-12)\n",
           g_worst_pass[0], g_worst_pass[1]);
    check_window_lattice<64, 64>();
    check_window_lattice<128, 32>();
    check_window_lattice<256, 16>();
    check_window_lattice<512, 8>();
    check_window_lattice<1024, 4>();
    check_window_lattice<1024, 8>();
    check_window_lattice<2048, 4>();
    check_window_lattice<4096, 4>();
    printf("window lattice: 8 tiles\n");

    double w32 = 0, w64 = 0;
    for (int bits : {13, 14, 16, 18}) {
        const double f32f = whole<float, -1>(bits), f32i = whole<float, 1>(bits), f64f = whole<double, -1>(bits), f64i = whole<double, 1>(bits);
        printf("numbers: %s points: f32 fwd %.3e inv %.3e, f64 fwd %.3e inv %.3e\n", bits == 18 ? "64 x 64 x 64" : bits == 13 ? "2^13" : bits == 14 ? "2^14" : "2^16",
               f32f, f32i, f64f, f64i);
        w32 = std::max(w32, std::max(f32f, f32i));
        w64 = std::max(w64, std::max(f64f, f64i));
    }
    printf("numbers: worst rel-L2 per transform: f32 %.3e (bound 1e-06), f64 %.3e (bound 1e-12)\n", w32, w64);
    CHECK(w32 < 1e-6 && w64 < 1e-12, "whole transforms against the long double transform");
    printf("%d failures\n", g_fail);
    printf(g_fail ? "FAIL\n" : "ok\n");
    return g_fail ? 1 : 0;
}
