// order_search_state.h -- what a context keeps of the order search
// (order_search.hip) and what the window re-optimisation (order_window.hip)
// shares with it: the searches' state beside the order MCMC's, which holds the
// lists; the permutation check of both entry points' orders; and the one scan
// -- wave_best -- from which every term and chosen set of either file comes.
#pragma once

#include <string>

#include "order_mcmc_state.h"
#include "order_search_dev.h"

namespace ulg {

// Per search the order, terms and entries, the best order and its entries, the
// pair stamps, S, S_best and the counts; the global step; the buffers a run's
// traces, ulg_order_best's orders and ulg_order_window's outputs pass through.
struct OrderSearchState {
    int n = 0;
    int64_t searches = 0;
    uint64_t seed = 0;
    int64_t tenure = 0, patience = 1;
    int64_t step = 0;
    bool ready = false;
    DevBuf<uint8_t> d_order, d_best_order;  // [searches][n]
    DevBuf<double> d_terms;                 // [searches][n] by position
    DevBuf<uint32_t> d_ent, d_best_ent;     // [searches][n] by position: the index in the variable's list
    DevBuf<uint32_t> d_stamp;               // [searches][n][n]
    DevBuf<double> d_score, d_best_score;   // [searches]
    DevBuf<long long> d_idle, d_moves, d_kicks;  // [searches]
    DevBuf<unsigned int> d_err;             // [1]: the least search with a -inf term
    DevBuf<double> r_gain, r_terms;
    DevBuf<uint8_t> r_pos, r_order;
    DevBuf<uint64_t> r_parents;
    DevBuf<double> r_wscore;      // ulg_order_window: [count] S
    DevBuf<long long> r_wcount;   // ... and [2][count]: the accepted windows, the sweeps
    // the dense candidate-set tables of option "search_tables" (order_tables.hip); `tables` says the searches use them
    bool tables = false;
    std::vector<uint64_t> cand;   // [n] C_v
    std::vector<int64_t> toff;    // [n + 1] the first slot of each variable's table
    DevBuf<uint64_t> d_cand, d_table;
    DevBuf<int64_t> d_toff;
    size_t table_bytes() const { return (d_cand.cap + d_table.cap + d_toff.cap) * 8; }
    size_t run_bytes() const {
        return (r_gain.cap + r_terms.cap + r_parents.cap + r_wscore.cap + r_wcount.cap) * 8 + r_pos.cap + r_order.cap;
    }
    size_t held_bytes() const {
        return d_order.cap + d_best_order.cap + d_terms.cap * 8 + (d_ent.cap + d_best_ent.cap + d_stamp.cap) * 4 +
               (d_score.cap + d_best_score.cap + d_idle.cap + d_moves.cap + d_kicks.cap) * 8 + run_bytes() + table_bytes();
    }
};

// the searches of the last ulg_order_search_begin*, or null
inline OrderSearchState *order_search_live(ulg_ctx *c) { return c->osearch && c->osearch->ready && c->mcmc ? c->osearch : nullptr; }

inline bool is_permutation(const uint8_t *row, int n) {
    uint64_t seen = 0;
    for (int p = 0; p < n; ++p) {
        if (row[p] >= n || ((seen >> row[p]) & 1ull)) return false;
        seen |= 1ull << row[p];
    }
    return true;
}

constexpr int kSearchWave = 64;

// What a launch of either run kernel (osearch_run_kernel, otab_run_kernel) reads
struct SearchArgs {
    const uint64_t *sets;
    const float *scores;
    const int64_t *offsets;
    uint8_t *order, *best_order;  // the searches' state ...
    double *terms;
    uint32_t *ent, *best_ent, *stamp;
    double *score, *best_score;
    long long *idle, *moves, *kicks;
    int n;
    int64_t searches;
    uint64_t seed;
    int64_t tenure, patience;
    int64_t t_begin, nsteps;  // the launch makes steps t_begin + 1 .. t_begin + nsteps
    int64_t t_call;           // the call began after step t_call: the traces are indexed from there
    double *t_gain;           // each may be null
    uint8_t *t_pos;
};

// ---- order_tables.hip: the tables of option "search_tables"
// C_v and the table offsets of the lists into s.cand, s.toff; refuses a K_v above kTableMaxK; *bytes = what the tables take
int order_tables_plan(ulg_ctx *c, const std::string &who, OrderSearchState &s, const OrderMcmcState &l, double *bytes);
int order_tables_build(ulg_ctx *c, OrderSearchState &s, const OrderMcmcState &l);  // allocates and fills them; s.tables
void order_tables_drop(OrderSearchState &s);
// osearch_best_kernel's outputs from the tables
int order_tables_best(ulg_ctx *c, const OrderSearchState &s, const OrderMcmcState &l, const uint8_t *d_orders, int64_t count,
                      double *d_terms, uint32_t *d_ent, uint64_t *d_parents);
void order_tables_run(ulg_ctx *c, const OrderSearchState &s, const SearchArgs &a);  // one launch of the run kernel over tables

#ifdef __HIPCC__
// ---- the scan: one wave, every lane returns the same key (0: no compatible entry)
__device__ __forceinline__ uint64_t wave_best(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t U, int lane) {
    const uint64_t outside = ~U;
    uint64_t key = 0;
    uint32_t low = 0xFFFFFFFFu - (uint32_t)lane;  // 2^32 - 1 - (i - b): a list holds at most 2^32 - 1 entries
#pragma unroll 2
    for (int64_t i = b + lane; i < e; i += kSearchWave, low -= kSearchWave) {
        const uint64_t S = sets[i];
        const uint64_t k = ((uint64_t)os_float_image(__float_as_uint(scores[i])) << 32) | low;
        if (!(S & outside) && k > key) key = k;
    }
    for (int d = kSearchWave / 2; d > 0; d >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)key, d, kSearchWave);
        key = o > key ? o : key;
    }
    return key;
}
#endif

}  // namespace ulg
