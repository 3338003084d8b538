// disc_prune.h -- the subset-rank arithmetic of the discrete scorer's prune
// pass (disc.hip disc_prune_kernel), usable from host and device:
// host/prune_check.cpp checks it against brute-force enumeration without a GPU.
//
// Slab (i, L) of the slot table holds variable i's sets of L parents in colex
// order over its compact candidate positions 0 .. m - 1: the set
// c_0 < ... < c_{L-1} has rank sum_j C(c_j, j + 1).  Without its member c_t it
// is a set of L - 1 positions whose rank in slab (i, L - 1) is
//     sum_{j<t} C(c_j, j + 1) + sum_{j>t} C(c_j, j).
// The colex unrank peels c_{L-1}, c_{L-2}, ... off the rank; what is left of
// the rank after peeling c_t is the first sum, and the second grows by
// C(c_t, t) per peeled member, so all L ranks come out of the one unrank loop
// with no per-thread array.
#pragma once

#include <cstdint>

#include "score_plan.h"  // ULG_HD

namespace ulg {

// prune(): scores within 2 * FLT_EPSILON count as equal (compareSecond,
// score_calculator.cpp:137-148)
constexpr float kPruneTwoEps = 2.3841858e-07f;

// The set of rank r among the L-subsets of 0 .. m - 1 (L <= m, r < C(m, L)):
// calls f(t, c_t, rank of the set without c_t in layer L - 1) for
// t = L - 1 down to 0.  binom: [64][64], C(a, b) at a * 64 + b.
template <class F>
ULG_HD inline void for_each_subset_rank(const uint64_t *binom, int m, int L, uint64_t r, F f) {
    uint64_t suf = 0;
    int c = m - 1;
    for (int e = L; e >= 1; --e) {
        while (c > e - 1 && binom[c * 64 + e] > r) --c;
        r -= binom[c * 64 + e];              // now sum_{j < e-1} C(c_j, j + 1)
        f(e - 1, c, r + suf);
        suf += binom[c * 64 + (e - 1)];
        --c;
    }
}

}  // namespace ulg
