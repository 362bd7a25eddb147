// conv_v2_core.h -- the schedule of the second-generation overlap-save block kernel (conv_v2_impl.h) as host+device
// functions without a HIP runtime call: the plan conv_v2_run launches with (which blocks of a vector are interior and
// which go through the wrap-around code, pairs of real blocks, partial runs, the grid and its shrink for small
// problems, the skewed shares of the dispatch groups) and the index pieces k_overlap_save_v2 is written with.
// tests/host_sim/sim_conv_v2.cpp compiles this text with the host compiler and runs the kernel's loops with workgroups
// and threads as loops (tests/test_conv_v2_abi.py); the library compiles the same text.
#pragma once
#include <cstddef>

#include "fft_core.h"

namespace bdsp {

constexpr int CONV_V2_L = 4096;     // points per block transform
constexpr unsigned CONV_V2_MAX_R0 = 12; // the kernel is instantiated for R0 = 1 .. 12: taps - 1 <= 3 L / 4

// R0 = ceil((M-1)/256): the rows of a block's result that the filter's history occupies (one row for M <= 1 as well)
BDSP_HD unsigned conv_v2_r0(size_t taps) { return taps <= 1 ? 1u : (unsigned)((taps - 1 + 255) / 256); }

template <typename T>
struct ConvV2Args {
    const cpx<T>* x;
    cpx<T>* y;
    const cpx<T>* hs;   // taps (hs_is_taps) or the UNSCALED, undelayed L-point spectrum of the taps
    const cpx<T>* wtab; // exp(-2 pi i m / 4096)
    unsigned n;      // points per vector
    unsigned taps;
    unsigned b_first, b_end; // blocks of each vector to compute
    unsigned nb_lo, nb_hi;   // the interior ones among them: window inside [0, n), all V outputs below n
    unsigned batch;
    unsigned na, nbb;        // interior blocks (all vectors together) given to dispatch groups 0 and 1
    int hs_is_taps;
    unsigned groups;         // dispatch groups = workgroups per CU: 3 (f32), 2 (f64)
};

// ------------------------------------------------------------------ the plan of one launch
enum { CONV_V2_PLAN_RUN = 0, CONV_V2_PLAN_NOTHING = 1, CONV_V2_PLAN_TOO_MANY = 2 };
struct ConvV2Plan {
    int status;              // CONV_V2_PLAN_*; everything below r0 and V is set for CONV_V2_PLAN_RUN only
    unsigned r0;
    long long V;             // outputs per (real) block: L - 256 r0
    long long b0, b1;        // blocks [b0, b1) of every vector; with real data a block is a PAIR of real blocks
    long long lo, hi;        // the interior ones: [lo, hi), b0 <= lo <= hi <= b1
    unsigned grid, gs;       // workgroups, and workgroups per dispatch group
    unsigned long long na, nbb; // interior blocks (all vectors together) of dispatch groups 0 and 1
};

// Blocks [first_block, first_block + nblocks) (nblocks = 0: all from first_block on) of every vector of the batch, on
// `cus` compute units with `groups` workgroups each; share_a / share_b: the percentages of the rounds given to
// dispatch groups 0 and 1, share_a <= 0 for the defaults (share_b is read for three groups only).
BDSP_HD ConvV2Plan conv_v2_plan(size_t points, size_t taps, size_t batch, size_t first_block, size_t nblocks, bool real,
                                int cus, unsigned groups, int share_a, int share_b)
{
    constexpr long long L = CONV_V2_L;
    ConvV2Plan p{};
    p.r0 = conv_v2_r0(taps);
    p.V = L - 256 * (long long)p.r0;
    const long long V = p.V;
    const long long U = real ? 2 : 1; // real blocks per kernel block
    const long long nb_all = (((long long)points + V - 1) / V + U - 1) / U;
    long long b0 = (long long)first_block, b1 = nblocks ? b0 + (long long)nblocks : nb_all;
    if (b1 > nb_all) b1 = nb_all;
    if (b0 >= b1 || batch == 0) { p.status = CONV_V2_PLAN_NOTHING; return p; }
    const long long in_off = -(long long)(taps / 2);
    // interior blocks: window [bV + in_off, + L) inside [0, n) (then all V outputs are below n as well, see below)
    long long lo = b0, hi = b1;
    // (a pair is interior when both of its real blocks are: the first one's window start and the last one's end decide)
    while (lo < hi && lo * U * V + in_off < 0) ++lo;
    while (hi > lo && ((hi * U - 1) * V + in_off + L > (long long)points || (hi * U - 1) * V + V > (long long)points)) --hi;
    if ((unsigned long long)(b1 - b0) * batch >= (1ull << 32) || batch > 0xffffffffull) { p.status = CONV_V2_PLAN_TOO_MANY; return p; }
    p.b0 = b0; p.b1 = b1; p.lo = lo; p.hi = hi;
    // grid: `groups` workgroups per CU, a multiple of 8 * groups so that every dispatch group is a multiple of 8
    const unsigned long long interior = (unsigned long long)(hi - lo) * batch;
    const unsigned long long wrap = (unsigned long long)((lo - b0) + (b1 - hi)) * batch;
    const unsigned Q = 8 * groups;
    unsigned grid = (unsigned)cus * groups;
    grid -= grid % Q;
    if (grid < Q) grid = Q;
    if (interior + wrap < grid) { // a small problem: no more workgroups than blocks (each one transforms the taps first)
        grid = (unsigned)((interior + wrap + Q - 1) / Q * Q);
        if (grid < Q) grid = Q;
    }
    const unsigned gs = grid / groups;
    // shares in whole rounds of gs blocks.  Three groups: ~43 % / ~37 % / rest (measured optimum 9 / 8 / 4.3 rounds of
    // 21.3); two groups: ~55 % / rest (12 of 21.3 rounds measured best for two workgroups per CU)
    const unsigned long long rounds = (interior + gs - 1) / gs;
    const unsigned long long pa = share_a > 0 ? (unsigned long long)share_a : (groups == 3 ? 43 : 55);
    const unsigned long long pb = groups == 3 ? (share_a > 0 ? (unsigned long long)share_b : 37) : 0;
    unsigned long long ra = (rounds * pa + 50) / 100, rb = (rounds * pb + 50) / 100;
    if (rounds && ra == 0) ra = 1;
    unsigned long long na = ra * gs, nbb = rb * gs;
    if (na > interior) na = interior;
    if (na + nbb > interior) nbb = interior - na;
    p.grid = grid; p.gs = gs; p.na = na; p.nbb = nbb;
    return p;
}

// the plan's part of the kernel's arguments (the pointers and hs_is_taps are the caller's)
template <typename T>
BDSP_HD void conv_v2_set_geometry(ConvV2Args<T>& a, const ConvV2Plan& p, size_t points, size_t taps, size_t batch, unsigned groups)
{
    a.groups = groups;
    a.n = (unsigned)points;
    a.taps = (unsigned)taps;
    a.b_first = (unsigned)p.b0; a.b_end = (unsigned)p.b1;
    a.nb_lo = (unsigned)p.lo; a.nb_hi = (unsigned)p.hi;
    a.batch = (unsigned)batch;
    a.na = (unsigned)p.na;
    a.nbb = (unsigned)p.nbb;
}

// ------------------------------------------------------------------ the kernel's index pieces
// k_overlap_save_v2 (conv_v2_impl.h) calls these, except where the call changed hipcc's instructions for the kernel: there
// it keeps the expression inline and names the function that repeats it -- conv_v2_in_off, conv_v2_wrap_count,
// conv_v2_wrap_block, conv_v2_store_limit, conv_v2_group_lo and conv_v2_group_hi.  Change both sides together.
BDSP_HD unsigned xcd_contiguous(unsigned bid, unsigned g)
{
    // workgroup w runs on XCD w % 8 (observed; only speed depends on it): give every XCD a contiguous run of the
    // blocks of a round, so that the M-1 input samples neighbouring blocks share are an L2 hit
    return (g & 7) == 0 ? (bid & 7) * (g >> 3) + (bid >> 3) : bid;
}

// the taps are delayed by d = 256 R0 - (M-1) samples, so that a block's first valid output is z[256 R0]
BDSP_HD unsigned conv_v2_delay(unsigned ov, unsigned taps) { return ov - (taps - 1); }
// block b's window starts at sample b V + in_off of its vector
BDSP_HD long long conv_v2_in_off(unsigned taps) { return -(long long)(taps / 2); }

// blocks outside [nb_lo, nb_hi) go through the wrap-around code: nw per vector, the ones before nb_lo first
BDSP_HD unsigned conv_v2_wrap_count(unsigned b_first, unsigned nb_lo, unsigned nb_hi, unsigned b_end)
{
    return (nb_lo - b_first) + (b_end - nb_hi);
}
BDSP_HD unsigned conv_v2_wrap_block(unsigned k, unsigned b_first, unsigned nb_lo, unsigned nb_hi)
{
    return k < nb_lo - b_first ? b_first + k : nb_hi + (k - (nb_lo - b_first));
}
// first sample of (real) block blk's window, wrapped into [0, n)
BDSP_HD long long conv_v2_window_start(long long blk, unsigned V, long long in_off, unsigned n)
{
    long long sb = (blk * V + in_off) % (long long)n;
    if (sb < 0) sb += n;
    return sb;
}
// z[np], OV <= np < OV + V, of (real) block blk is output obase + np; only outputs below n exist: np < lim
BDSP_HD long long conv_v2_obase(long long blk, unsigned V, unsigned ov) { return blk * V - ov; }
BDSP_HD unsigned conv_v2_store_limit(unsigned n, long long obase)
{
    const long long room = (long long)n - obase;
    return room <= 0 ? 0u : (room > CONV_V2_L ? (unsigned)CONV_V2_L : (unsigned)room);
}

// dispatch group grp takes the interior ids [lo, hi) of the `total` = (nb_hi - nb_lo) batch
BDSP_HD unsigned conv_v2_group_lo(unsigned grp, unsigned na, unsigned nbb) { return grp == 0 ? 0u : (grp == 1 ? na : na + nbb); }
BDSP_HD unsigned conv_v2_group_hi(unsigned grp, unsigned groups, unsigned na, unsigned nbb, unsigned total)
{
    return grp == 0 ? na : ((grp == 1 && groups == 3) ? na + nbb : total);
}
// interior id -> vector and block (the single-vector instantiation has no division)
template <bool BATCHED>
BDSP_HD void conv_v2_split_id(unsigned id, unsigned ni, unsigned nb_lo, unsigned& vec, unsigned& b)
{
    vec = 0; b = nb_lo + id;
    if (BATCHED) { vec = id / ni; b = nb_lo + id % ni; }
}

} // namespace bdsp
