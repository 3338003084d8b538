// order_sumtables_dev.h -- the arithmetic of the order MCMC's dense log-sum
// tables (order_sumtables.hip, option "mcmc_tables", ulg_order_mcmc_table;
// contract: include/ulg.h, "Order MCMC over log-sum tables"): the table of a
// variable built one slot after the other -- every entry's score at the index
// of its own set, -inf elsewhere, and K_v subset-sum butterfly rounds of
// post_logaddexp in ascending order.  The candidate set, ranks and indices are
// order_tables_dev.h's.  Host and device: it compiles under hipcc and under a
// plain C++ compiler (host/order_sumtables_check.cpp).  Every path uses these
// definitions.
#pragma once

#include "order_tables_dev.h"

namespace ulg {

// Round j for the slot x that has bit j: the log-sum over the subsets of x
// with bits 0 .. j free is post_logaddexp of the two with bit j fixed.  A round
// reads slots without bit j and writes slots with it, so within a round the
// slots may be taken in any order; the rounds themselves ascend.
ULG_POST_HD double ost_round(double with_bit, double without_bit) { return post_logaddexp(with_bit, without_bit); }

ULG_POST_HD void ost_butterfly_serial(double *L, int K) {
    const int64_t slots = ot_slots(K);
    for (int j = 0; j < K; ++j)
        for (int64_t x = 0; x < slots; ++x)
            if ((x >> j) & 1) L[x] = ost_round(L[x], L[x ^ ((int64_t)1 << j)]);
}

// L[0 .. 2^K) of the entries [b, e) with candidates C, K = |C|: every slot
// -inf, every entry's score as a double at the index of its own set (distinct
// sets: distinct slots), then the rounds.  L[x] = ln of the sum of exp(s_i)
// over the entries inside ot_expand(C, x), -inf exactly without one.
ULG_POST_HD void ost_build_serial(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t C, double *L) {
    const int K = ot_popcount(C);
    for (int64_t x = 0; x < ot_slots(K); ++x) L[x] = -INFINITY;
    for (int64_t i = b; i < e; ++i) L[ot_index(C, sets[i])] = (double)scores[i];
    ost_butterfly_serial(L, K);
}

}  // namespace ulg
