// order_tables_dev.h -- the arithmetic of the order search's dense
// candidate-set tables (order_tables.hip, option "search_tables",
// ulg_order_search_table; contract: include/ulg.h, "Order search"): the
// candidate set C_v of a variable, the rank of a candidate inside it, the
// table index of a predecessor set and its inverse, the bit a neighbour swap
// adds or takes, and the table's build one slot after the other -- a scatter of
// os_entry_key and K_v subset-maximum butterfly rounds.  Host and device, as
// order_search_dev.h is, whose key it tabulates: it compiles under hipcc and
// under a plain C++ compiler (host/order_tables_check.cpp).  Every path uses
// these definitions.
#pragma once

#include "order_search_dev.h"

namespace ulg {

constexpr int kTableMaxK = 26;  // 2^26 slots of 8 B: 512 MB for one variable
constexpr int kTableLdsK = 13;  // 2^13 slots of 8 B: the 64 KB of LDS one workgroup builds a table or a tile in

// C_v: the OR of the stored sets of entries [b, e)
ULG_POST_HD uint64_t ot_candidates(const uint64_t *sets, int64_t b, int64_t e) {
    uint64_t C = 0;
    for (int64_t i = b; i < e; ++i) C |= sets[i];
    return C;
}

ULG_POST_HD int ot_popcount(uint64_t x) { return __builtin_popcountll(x); }

// rank_v(u): the members of C below u
ULG_POST_HD int ot_rank(uint64_t C, int u) { return ot_popcount(C & ((1ull << u) - 1ull)); }

// the index bit of variable u in v's table: 1 << rank_v(u), 0 when u is no candidate
ULG_POST_HD uint32_t ot_bit(uint64_t C, int u) { return ((C >> u) & 1ull) ? 1u << ot_rank(C, u) : 0u; }

// idx_v(U) = the sum over u in U & C of 1 << rank_v(u): the bits of U at C's members, squeezed together
ULG_POST_HD uint32_t ot_index(uint64_t C, uint64_t U) {
    uint32_t idx = 0;
    for (uint64_t m = U & C; m; m &= m - 1ull) idx |= 1u << ot_popcount(C & ((m & (~m + 1ull)) - 1ull));
    return idx;
}

// ... and its inverse: the x-selected members of C
ULG_POST_HD uint64_t ot_expand(uint64_t C, uint32_t x) {
    uint64_t U = 0;
    for (uint64_t m = C; m && x; m &= m - 1ull, x >>= 1)
        if (x & 1u) U |= m & (~m + 1ull);
    return U;
}

// the slots of a table of K candidates
ULG_POST_HD int64_t ot_slots(int K) { return (int64_t)1 << K; }

// Round j of the butterfly for the slot x that has bit j: the maximum over the
// subsets of x with bits 0 .. j free is the greater of the two with bit j fixed.
// A maximum of integers: the same table whatever the order of rounds and slots.
ULG_POST_HD void ot_butterfly_serial(uint64_t *T, int K) {
    const int64_t slots = ot_slots(K);
    for (int j = 0; j < K; ++j)
        for (int64_t x = 0; x < slots; ++x)
            if (((x >> j) & 1) && T[x ^ ((int64_t)1 << j)] > T[x]) T[x] = T[x ^ ((int64_t)1 << j)];
}

// T[0 .. 2^K) of the entries [b, e) with candidates C, K = |C|: every slot 0,
// every entry's key at the index of its own set (distinct sets: distinct
// slots), then the rounds.  T[x] = os_best_serial(.., ot_expand(C, x)).
ULG_POST_HD void ot_build_serial(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t C, uint64_t *T) {
    const int K = ot_popcount(C);
    for (int64_t x = 0; x < ot_slots(K); ++x) T[x] = 0;
    for (int64_t i = b; i < e; ++i) {
        uint32_t bits;
        __builtin_memcpy(&bits, &scores[i], 4);
        T[ot_index(C, sets[i])] = os_entry_key(bits, (uint32_t)(i - b));
    }
    ot_butterfly_serial(T, K);
}

}  // namespace ulg
