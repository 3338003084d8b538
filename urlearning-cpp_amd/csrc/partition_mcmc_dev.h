// partition_mcmc_dev.h -- the arithmetic of the partition MCMC
// (partition_mcmc.hip, ulg_partition_mcmc_*, ulg_partition_score; contract:
// include/ulg.h, "Partition MCMC"): the eligibility of a stored parent set
// under an ordered partition, a variable's term, the plan of a step's move
// from its draws, what the plan makes of a variable's part and of a part's
// mask, and ln rho.  Host and device, as order_mcmc_dev.h is, whose draw,
// accept rule, two-word sum and term expression it reuses: it compiles under
// hipcc and under a plain C++ compiler (host/partition_mcmc_check.cpp).  Every
// path uses these definitions.
#pragma once

#include "order_mcmc_dev.h"

namespace ulg {

constexpr uint32_t kPartAuxDomain = 65;  // u_acc and the split mask; 0 is the move, 1 + v a record's parent set of v (v <= 62)
constexpr double kPartLn2 = 0.693147180559945309417232121458;

// A stored set P of a variable whose allowed parents are A (the union of the
// parts before its own) and whose required parents are R (the part just
// before; 0 in part 0, where A = 0 too and only the empty set passes).
ULG_POST_HD bool part_eligible(uint64_t P, uint64_t A, uint64_t R) { return !(P & ~A) && (R == 0 || (P & R) != 0); }

// a_v = ln T_v over the entries [b, e): mcmc_term_serial with the test above
ULG_POST_HD double part_term_serial(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t A, uint64_t R) {
    double m = -INFINITY;
    for (int64_t i = b; i < e; ++i)
        if (part_eligible(sets[i], A, R) && (double)scores[i] > m) m = (double)scores[i];
    if (!(m > -INFINITY)) return -INFINITY;
    LxCount T{0, 0};
    for (int64_t i = b; i < e; ++i)
        if (part_eligible(sets[i], A, R)) T = lx_add(T, LxCount{post_weight_q((double)scores[i] - m), 0});
    return mcmc_term(m, T);
}

// The part masks of a row of part indices; returns m, or 0 when the row does
// not use exactly the indices 0 .. m-1 (mask: n words at least).
ULG_POST_HD int part_masks(int n, const uint8_t *part_of, uint64_t *mask) {
    for (int j = 0; j < n; ++j) mask[j] = 0;
    int m = 0;
    for (int v = 0; v < n; ++v) {
        if (part_of[v] >= n) return 0;
        mask[part_of[v]] |= 1ull << v;
        if (part_of[v] + 1 > m) m = part_of[v] + 1;
    }
    for (int j = 0; j < m; ++j)
        if (!mask[j]) return 0;
    return m;
}

// ---- a step's move.  The operations a plan can hold:
enum PartOp { kPartSwap = 0, kPartToPart = 1, kPartToGap = 2, kPartSplit = 3, kPartJoin = 4 };

// What the draws make of the state (part_of[n], mask[m]).  A relocation is
// planned in two stages: v leaves part a (the part is deleted when `emptied`,
// the parts behind it move down), then joins part b or becomes a singleton
// before part b, b counted among the parts that are left.
struct PartPlan {
    int op;
    bool noop;     // the step proposes nothing: rejected, delta reads -inf
    int v, w;      // swap: the two variables; relocation: v
    int a, b;      // swap: the parts of v and w; relocation: above; split, join: a = j
    bool emptied;  // relocation: v was a singleton
    uint64_t low;  // split: L = B_j & r, which stays at index j; B_j & ~L goes to j + 1
    int m, m_new;  // parts before and after
    int k;         // split: |B_j|; join: |B_j| + |B_j+1|
};

// w: the draw of domain 0; r: the split mask of domain kPartAuxDomain
ULG_POST_HD PartPlan part_plan(const uint32_t w[4], uint64_t r, int n, int m, const uint8_t *part_of, const uint64_t *mask) {
    PartPlan pl;
    pl.op = kPartSwap, pl.noop = true, pl.v = pl.w = pl.a = pl.b = pl.k = 0, pl.emptied = false, pl.low = 0, pl.m = pl.m_new = m;
    if (n < 2) return pl;
    const uint32_t kind = w[0] >> 30;
    if (kind == 0) {
        pl.v = (int)post_mulhi32(w[1], (uint32_t)n);
        const int wp = (int)post_mulhi32(w[2], (uint32_t)(n - 1));
        pl.w = wp + (wp >= pl.v ? 1 : 0);
        pl.a = part_of[pl.v], pl.b = part_of[pl.w];
        pl.noop = pl.a == pl.b;
    } else if (kind < 3) {
        pl.v = (int)post_mulhi32(w[1], (uint32_t)n);
        const int tau = (int)post_mulhi32(w[2], (uint32_t)(2 * m + 1));
        pl.a = part_of[pl.v];
        pl.emptied = mask[pl.a] == 1ull << pl.v;
        const int e = pl.emptied ? 1 : 0;
        if (tau & 1) {
            const int k = (tau - 1) / 2;
            pl.op = kPartToPart;
            pl.noop = k == pl.a;
            pl.b = k - (e && k > pl.a ? 1 : 0);
            pl.m_new = m - e;
        } else {
            const int g = tau / 2;
            pl.op = kPartToGap;
            pl.b = g - (e && g > pl.a ? 1 : 0);
            pl.noop = e && pl.b == pl.a;  // gaps j and j + 1 of a singleton's own part
            pl.m_new = m - e + 1;
        }
    } else {
        pl.a = (int)post_mulhi32(w[1], (uint32_t)m);
        if ((w[0] >> 29) & 1u) {
            pl.op = kPartSplit;
            pl.low = mask[pl.a] & r;
            pl.noop = pl.low == 0 || pl.low == mask[pl.a];
            pl.k = __builtin_popcountll(mask[pl.a]);
            pl.m_new = m + 1;
        } else {
            pl.op = kPartJoin;
            pl.noop = pl.a == m - 1;
            if (!pl.noop) pl.k = __builtin_popcountll(mask[pl.a] | mask[pl.a + 1]);
            pl.m_new = m - 1;
        }
    }
    if (pl.noop) pl.m_new = m;
    return pl;
}

// The part of variable u, in part p before, after the plan's move (not a no-op)
ULG_POST_HD int part_new_index(const PartPlan &pl, int u, int p) {
    switch (pl.op) {
        case kPartSwap: return u == pl.v ? pl.b : u == pl.w ? pl.a : p;
        case kPartToPart: return u == pl.v ? pl.b : p - (pl.emptied && p > pl.a ? 1 : 0);
        case kPartToGap: {
            if (u == pl.v) return pl.b;
            const int p1 = p - (pl.emptied && p > pl.a ? 1 : 0);
            return p1 + (p1 >= pl.b ? 1 : 0);
        }
        case kPartSplit: return p < pl.a ? p : p > pl.a ? p + 1 : ((pl.low >> u) & 1ull) ? pl.a : pl.a + 1;
        default: return p - (p > pl.a ? 1 : 0);
    }
}

// The mask of part i < m_new after the move, from the masks before it
ULG_POST_HD uint64_t part_new_mask(const PartPlan &pl, int i, const uint64_t *mask) {
    const uint64_t bv = 1ull << pl.v;
    switch (pl.op) {
        case kPartSwap: {
            const uint64_t flip = bv ^ (1ull << pl.w);
            return i == pl.a || i == pl.b ? mask[i] ^ flip : mask[i];
        }
        case kPartToPart: {
            const uint64_t x = mask[i + (pl.emptied && i >= pl.a ? 1 : 0)] & ~bv;
            return i == pl.b ? x | bv : x;
        }
        case kPartToGap: {
            if (i == pl.b) return bv;
            const int i1 = i - (i > pl.b ? 1 : 0);
            return mask[i1 + (pl.emptied && i1 >= pl.a ? 1 : 0)] & ~bv;
        }
        case kPartSplit: return i < pl.a ? mask[i] : i == pl.a ? pl.low : i == pl.a + 1 ? mask[pl.a] & ~pl.low : mask[i - 1];
        default: return i < pl.a ? mask[i] : i == pl.a ? mask[pl.a] | mask[pl.a + 1] : mask[i + 1];
    }
}

// ln rho of a move that is not a no-op: the proposal's Hastings ratio.
//   swap        1: the same ordered pair undoes it.
//   relocation  (2m + 1) / (2m' + 1): S -> S' is possible iff the two agree
//               after deleting some v; the number of such v is the same from
//               either side, and for each exactly one tau does it.
//   split       2^k m / (m + 1): one of m parts, one of 2^k subsets, against
//               one of m + 1 joins;  join: 2^-k m / (m - 1), its inverse.
ULG_POST_HD double part_log_rho(const PartPlan &pl) {
    switch (pl.op) {
        case kPartSwap: return 0.0;
        case kPartToPart:
        case kPartToGap: return log((double)(2 * pl.m + 1) / (double)(2 * pl.m_new + 1));
        case kPartSplit: return (double)pl.k * kPartLn2 + log((double)pl.m / (double)(pl.m + 1));
        default: return -(double)pl.k * kPartLn2 + log((double)pl.m / (double)(pl.m - 1));
    }
}

}  // namespace ulg
