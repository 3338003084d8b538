// order_picktables_dev.h -- the arithmetic of a record's DAG drawn from the
// order MCMC's tables (order_picktables.hip, option "mcmc_table_picks",
// ulg_order_mcmc_stage_table; contract: include/ulg.h, "Order MCMC: a record's
// DAG from the tables"): how many 6-bit chunks a table index has, the stage
// tables -- the log-sum table as it stands before rounds 6, 12, 18 and 24 of
// its ascending butterfly -- the entry map, a lane's slot at a level of the
// descent, and the descent itself one lane after the other.  After rounds
// 0 .. j-1 slot y holds ln of the summed weights of the stored sets whose
// index bits >= j equal y's and whose bits < j lie inside y's: the conditional
// sums a descent that fixes bits from the top needs.  Host and device, as
// order_sumtables_dev.h is: it compiles under hipcc and under a plain C++
// compiler (host/order_picktables_check.cpp).  Every path uses these
// definitions.
#pragma once

#include "order_sumtables_dev.h"

namespace ulg {

constexpr int kPickBits = 6;       // index bits fixed per level: lane l of a wave64 is the pattern l
constexpr int kPickLanes = 1 << kPickBits;
constexpr int kPickMaxChunks = (kTableMaxK + kPickBits - 1) / kPickBits;  // 5
constexpr uint32_t kPickDomain = 64;  // level c of position p draws in domain 1 + p + 64 c (level 0: the list pick's domain)

// nch_v: the levels of a pick in a table of K candidates
ULG_POST_HD int opt_chunks(int K) { return K <= kPickBits ? 1 : (K + kPickBits - 1) / kPickBits; }

// the bytes of variable v's tables: L_v alone, or with the nch - 1 stage tables and the int32 entry map
ULG_POST_HD double opt_bytes(int K, bool picks) { return (picks ? 8.0 * opt_chunks(K) + 4.0 : 8.0) * (double)ot_slots(K); }

// Lane l at level c of a pick at table index x: compatible iff its pattern lies
// inside x's bits of that chunk (and, in the top chunk, inside the table: implied
// by x < 2^K, kept as the contract states it)
ULG_POST_HD bool opt_lane_on(int K, uint32_t x, int c, int lane) {
    if ((uint32_t)lane & ~((x >> (kPickBits * c)) & (uint32_t)(kPickLanes - 1))) return false;
    return K - kPickBits * c >= kPickBits || lane < (1 << (K - kPickBits * c));
}

// ... and its slot: the bits fixed above, its own pattern, x's bits below
ULG_POST_HD uint32_t opt_slot(uint32_t fixed, uint32_t x, int c, int lane) {
    return fixed | ((uint32_t)lane << (kPickBits * c)) | (x & ((1u << (kPickBits * c)) - 1u));
}

// ost_build_serial with the snapshots: L as there, S[(c - 1) 2^K + x] = L[x]
// before round 6 c for c = 1 .. nch - 1 (copies, not recomputed), and
// E[idx(P_i)] = i - b, -1 elsewhere.  S may be null when nch = 1.
ULG_POST_HD void opt_build_serial(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t C, double *L, double *S,
                                  int32_t *E) {
    const int K = ot_popcount(C);
    const int64_t slots = ot_slots(K);
    for (int64_t x = 0; x < slots; ++x) L[x] = -INFINITY, E[x] = -1;
    for (int64_t i = b; i < e; ++i) {
        const uint32_t x = ot_index(C, sets[i]);
        L[x] = (double)scores[i], E[x] = (int32_t)(i - b);
    }
    for (int j = 0; j < K; ++j) {
        if (j && j % kPickBits == 0)
            for (int64_t x = 0; x < slots; ++x) S[(j / kPickBits - 1) * slots + x] = L[x];
        for (int64_t x = 0; x < slots; ++x)
            if ((x >> j) & 1) L[x] = ost_round(L[x], L[x ^ ((int64_t)1 << j)]);
    }
}

// The value lane l weighs at level c: the stage table's slot, or at level 0
// the score of the entry stored there (-inf without one)
ULG_POST_HD double opt_value(const double *S, const int32_t *E, const float *scores_v, int K, int c, uint32_t slot) {
    if (c >= 1) return S[(int64_t)(c - 1) * ot_slots(K) + slot];
    return E[slot] >= 0 ? (double)scores_v[E[slot]] : -INFINITY;
}

// The pick of position p of chain `chain` at step t: variable v's tables (S, E,
// K), scores_v = its list's scores, x = idx_v(pre_p), a = L_v[x].  -> the entry
// i - offsets[v], -1 when a level's weights are all 0 (the kernel takes a level
// with one lane per pattern and a scan across the wave: the integers are the same).
ULG_POST_HD int64_t opt_pick_serial(const double *S, const int32_t *E, const float *scores_v, int K, uint32_t x, double a, uint64_t seed,
                                    uint64_t t, uint32_t chain, int p) {
    uint32_t fixed = 0;
    double a_cur = a;
    for (int c = opt_chunks(K) - 1; c >= 0; --c) {
        uint64_t q[kPickLanes];
        double val[kPickLanes];
        for (int l = 0; l < kPickLanes; ++l) {
            const bool on = opt_lane_on(K, x, c, l);
            val[l] = on ? opt_value(S, E, scores_v, K, c, opt_slot(fixed, x, c, l)) : -INFINITY;
            q[l] = on ? post_weight_q(val[l] - a_cur) : 0;
        }
        uint32_t w[4];
        mcmc_draw(seed, t, chain, 1u + (uint32_t)p + kPickDomain * (uint32_t)c, w);
        const int64_t j = post_pick(q, kPickLanes, (uint64_t)w[0] | ((uint64_t)w[1] << 32));
        if (j == kPickLanes) return -1;
        fixed |= (uint32_t)j << (kPickBits * c);
        a_cur = val[j];
    }
    return E[fixed];
}

}  // namespace ulg
