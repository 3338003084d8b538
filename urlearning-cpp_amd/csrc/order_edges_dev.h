// order_edges_dev.h -- the arithmetic of the Rao-Blackwellised edge posterior
// of an order (order_edges.hip, ulg_order_edges; contract: include/ulg.h):
// the conversion of a two-word sum, the fixed-point ratio g = floor(N / T 2^40)
// and one variable's whole row over its list, one entry after the other.  Host
// and device, as order_mcmc_dev.h is, whose weight, two-word add and maximum
// rule it reuses: it compiles under hipcc and under a plain C++ compiler
// (host/order_edges_check.cpp).  Every path uses these definitions.
#pragma once

#include "order_mcmc_dev.h"

namespace ulg {

constexpr int kEdgeBits = 40;                     // g = floor(p 2^40): p = 1 is 2^40 exactly
constexpr int64_t kEdgeMaxOrders = 1ll << 22;     // orders of one call: a group's sum stays below 2^62

// y(X) = X 2^-52 for X = lo + 2^64 hi: the conversion of mcmc_term, word by word
ULG_POST_HD double edge_y(LxCount X) { return ldexp((double)X.hi, 12) + ldexp((double)X.lo, -52); }

// g = floor(y(N) / y(T) 2^40) for 0 <= N <= T, T > 0: one IEEE division.  Both
// conversions are monotone, so y(N) <= y(T), the quotient is at most 1 and
// g <= 2^40, with equality iff y(N) = y(T) (N = T gives it to the bit).  N = 0
// gives 0.
ULG_POST_HD uint64_t edge_g(LxCount N, LxCount T) {
    if (!(N.lo | N.hi)) return 0;
    return (uint64_t)floor(ldexp(edge_y(N) / edge_y(T), kEdgeBits));
}

// One variable's row: over its list entries [b, e) with predecessor set U,
// g[u] = edge_g(N_u, T) for u < n, where T is the term's sum (mcmc_term_serial)
// and N_u the sum of the same weights over the compatible entries that hold u.
// A u outside U is held by no compatible entry: N_u = 0, g[u] = 0.  false, and
// g all 0, without a compatible entry (the term is -inf).  The check program
// and the tests' restatement; the kernel strides the list by lanes, lane u
// owning N_u -- the integers are the same.  Nw, Tw (may be null): the sums
// themselves, N_u at Nw[u].
ULG_POST_HD bool edge_row_serial(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t U, int n, uint64_t *g,
                                 LxCount *Nw, LxCount *Tw) {
    for (int u = 0; u < n; ++u) g[u] = 0;
    double m = -INFINITY;
    for (int64_t i = b; i < e; ++i)
        if (!(sets[i] & ~U) && (double)scores[i] > m) m = (double)scores[i];
    if (!(m > -INFINITY)) return false;
    LxCount T{0, 0};
    LxCount N[kMcmcMaxVars + 1];
    for (int u = 0; u <= kMcmcMaxVars; ++u) N[u] = LxCount{0, 0};
    for (int64_t i = b; i < e; ++i) {
        if (sets[i] & ~U) continue;
        const LxCount q{post_weight_q((double)scores[i] - m), 0};
        T = lx_add(T, q);
        for (uint64_t S = sets[i]; S; S &= S - 1) {
            const int u = __builtin_ctzll(S);
            N[u] = lx_add(N[u], q);
        }
    }
    for (int u = 0; u < n; ++u) {
        g[u] = edge_g(N[u], T);
        if (Nw) Nw[u] = N[u];
    }
    if (Tw) *Tw = T;
    return true;
}

}  // namespace ulg
