// order_mcmc_run.h -- what the two run kernels of the order MCMC share
// (mcmc_run_kernel of order_mcmc.hip over the lists, ostab_run_kernel of
// order_sumtables.hip over the log-sum tables of option "mcmc_tables"): the
// error word's bits, a launch's arguments, the record's parent-set pick, and
// the host entry points of the tables.
#pragma once

#include <string>

#include "order_mcmc_dev.h"
#include "order_mcmc_state.h"

namespace ulg {

// bits of the error word (d_err[0]); d_err[1] = the least chain with a -inf term
constexpr unsigned kErrSet = 1, kErrScore = 2, kErrDup = 4, kErrPick = 8;
constexpr int kMcmcWave = 64;

struct RunArgs {
    const uint64_t *sets;
    const float *scores;
    const int64_t *offsets;
    uint8_t *order;                 // [chains][n] the chains' state ...
    double *terms;                  // [chains][n]
    unsigned long long *accepted;   // [chains]
    int n;
    int64_t chains;
    uint64_t seed;
    int64_t t_begin, nsteps;  // the launch makes steps t_begin + 1 .. t_begin + nsteps
    int64_t t_call, thin;     // the call began after step t_call: records and traces are indexed from there
    uint8_t *r_order;         // each may be null
    double *r_score;
    uint64_t *r_parents;
    double *r_weight;
    double *t_delta;
    uint8_t *t_accept;
    unsigned int *err;
};

// ---- order_sumtables.hip: the tables of option "mcmc_tables"
// C_v and the table offsets of the lists into s.cand, s.toff; refuses a K_v above kTableMaxK and tables beyond the free memory
int order_sumtables_plan(ulg_ctx *c, const std::string &who, OrderMcmcState &s);
int order_sumtables_build(ulg_ctx *c, OrderMcmcState &s);  // allocates and fills them; s.tables
void order_sumtables_drop(OrderMcmcState &s);
int order_sumtables_terms(ulg_ctx *c, OrderMcmcState &s, int64_t chains);  // d_terms of the chains' d_order from the tables
void order_sumtables_run(ulg_ctx *c, const OrderMcmcState &s, const RunArgs &a);  // one launch of the run kernel over tables

// ---- order_picktables.hip: a record's DAG from the tables (option "mcmc_table_picks"; s.table_picks is set by the begin)
// s.soff and the memory of every table, stage table and entry map against what is free (big: the variable of the largest K);
// allocates d_soff, d_stage, d_entry.  Called by order_sumtables_plan in place of its own count.
int order_picktables_plan(ulg_ctx *c, const std::string &who, OrderMcmcState &s, int big);
void order_picktables_drop(OrderMcmcState &s);
void order_picktables_run(ulg_ctx *c, const OrderMcmcState &s, const RunArgs &a);  // one launch of the run kernel that picks from the tables

#ifdef __HIPCC__
// ---- a record's parent set: the sampler's set step (posterior_sample.hip)
__device__ __forceinline__ uint64_t wave_scan(uint64_t x, int lane) {
    for (int d = 1; d < kMcmcWave; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, d, kMcmcWave);
        if (lane >= d) x += y;
    }
    return x;
}
__device__ __forceinline__ int first_above(uint64_t C, uint64_t t) {
    const unsigned long long hit = __ballot(C > t);
    return hit ? __ffsll(hit) - 1 : -1;
}
// The entry of [b, e) chosen by u_set among those within U, weights
// floor(exp((double) s - a) 2^52); -1 when every weight is 0 (wave-uniform)
__device__ __forceinline__ int64_t wave_pick(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t U, double a,
                                             uint64_t u_set, int lane) {
    const uint64_t outside = ~U;
    auto weigh = [&](int64_t idx) -> uint64_t {
        if (idx >= e) return 0;
        if (sets[idx] & outside) return 0;
        return post_weight_q((double)scores[idx] - a);
    };
    if (e - b <= kMcmcWave) {
        const uint64_t C = wave_scan(weigh(b + lane), lane);
        const uint64_t t = post_pick_threshold(u_set, __shfl((unsigned long long)C, kMcmcWave - 1, kMcmcWave));
        const int j = first_above(C, t);
        return j >= 0 ? b + j : -1;
    }
    uint64_t T = 0;
    for (int64_t idx = b + lane; idx < e; idx += kMcmcWave) T += weigh(idx);
    for (int s = kMcmcWave / 2; s > 0; s >>= 1) T += __shfl_xor((unsigned long long)T, s, kMcmcWave);
    const uint64_t t = post_pick_threshold(u_set, T);
    uint64_t base = 0;
    for (int64_t c0 = b; c0 < e; c0 += kMcmcWave) {
        const uint64_t C = base + wave_scan(weigh(c0 + lane), lane);
        const int j = first_above(C, t);
        if (j >= 0) return c0 + j;
        base = __shfl((unsigned long long)C, kMcmcWave - 1, kMcmcWave);
    }
    return -1;
}
#endif

}  // namespace ulg
