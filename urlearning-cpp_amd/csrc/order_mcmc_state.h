// order_mcmc_state.h -- what a context keeps of the order MCMC
// (order_mcmc.hip): the device copy of the lists of the last
// ulg_order_mcmc_begin*, per chain the order, the terms and the accepted
// count, the global step, and the buffers a run's records and traces pass
// through.  With rungs >= 1 the chains are the replicas of `chains` tempered
// ladders (ulg_order_mc3_*): order, terms stay with a replica's slot
// ladder * rungs + r0, d_perm says which slot stands on each rung, and
// d_accepted counts by rung.  Beside PosteriorState and apart from it: no call of either kind
// reads the other's, and a ulg_posterior* call deletes this one
// (order_mcmc_delete) before it sizes its tables.
#pragma once

#include <vector>

#include "ulg_internal.h"

namespace ulg {

// What the ladders' kernel reads beyond its launch's steps: one copy in device
// memory per run, so that a launch passes a pointer and two numbers.
struct Mc3Args {
    const uint64_t *sets;
    const float *scores;
    const int64_t *offsets;
    uint8_t *order;                // [ladders][rungs][n] by replica slot ...
    double *terms;                 // [ladders][rungs][n]
    uint8_t *perm;                 // [ladders][rungs] the slot on each rung
    unsigned long long *accepted;  // [ladders][rungs] by rung
    unsigned long long *swaps;     // [ladders][rungs - 1]
    int n, rungs;
    int64_t ladders;
    uint64_t seed;
    int64_t swap_every;
    int64_t t_call, thin;  // the call began after step t_call: records and traces are indexed from there
    uint8_t *r_order;      // each may be null
    double *r_score;
    uint64_t *r_parents;
    double *r_weight;
    double *t_delta;
    uint8_t *t_accept;
    double *t_swap_d;
    uint8_t *t_swap_accept;
    unsigned int *err;
    double betas[16];
};

struct OrderMcmcState {
    int n = 0;
    int64_t total = 0;   // list entries
    int64_t chains = 0;  // chains, or ladders
    int rungs = 0;       // 0: independent chains (ulg_order_mcmc_*); >= 1: ladders of this many rungs (ulg_order_mc3_*)
    int64_t swap_every = 1;
    double betas[16] = {};
    uint64_t seed = 0;
    int64_t step = 0;    // steps every chain has made since begin
    bool ready = false;
    DevBuf<uint64_t> d_sets;
    DevBuf<float> d_scores;
    DevBuf<int64_t> d_offsets;
    std::vector<int64_t> offsets;  // their host copy (the source of the upload: it outlives the call)
    DevBuf<uint8_t> d_order;              // [chains][n]
    DevBuf<double> d_terms;               // [chains][n]
    DevBuf<unsigned long long> d_accepted;  // [chains]
    DevBuf<unsigned int> d_err;           // [2]: an error word, the least chain with a -inf term
    DevBuf<uint8_t> d_perm;                 // [ladders][rungs]
    DevBuf<unsigned long long> d_swaps;     // [ladders][rungs - 1]
    DevBuf<Mc3Args> d_args;                 // [1]
    Mc3Args args;                           // ... and the upload's source, which outlives the call
    // the records and traces of one run, and ulg_order_score's orders and terms
    DevBuf<uint8_t> r_order, r_taccept, r_tswapacc;
    DevBuf<double> r_score, r_weight, r_tdelta, r_tswapd;
    DevBuf<uint64_t> r_parents;
    // the dense log-sum tables of option "mcmc_tables" (order_sumtables.hip); `tables` says the chains read them
    bool tables = false;
    std::vector<uint64_t> cand;  // [n] C_v
    std::vector<int64_t> toff;   // [n + 1] the first slot of each variable's table
    DevBuf<uint64_t> d_cand;
    DevBuf<int64_t> d_toff;
    DevBuf<double> d_sumtable;
    // ... and what option "mcmc_table_picks" adds for a record's DAG (order_picktables.hip); `table_picks` says the records descend them
    bool table_picks = false;
    std::vector<int64_t> soff;  // [n + 1] the first slot of each variable's stage tables S_{v,1} .. S_{v,nch-1}
    DevBuf<int64_t> d_soff;
    DevBuf<double> d_stage;
    DevBuf<int32_t> d_entry;    // E_v at toff[v]
    size_t table_bytes() const { return (d_cand.cap + d_toff.cap + d_sumtable.cap + d_soff.cap + d_stage.cap) * 8 + d_entry.cap * 4; }
    size_t run_bytes() const {
        return r_order.cap + r_taccept.cap + r_tswapacc.cap + (r_score.cap + r_weight.cap + r_tdelta.cap + r_tswapd.cap) * 8 +
               r_parents.cap * 8;
    }
    size_t held_bytes() const {
        return d_sets.cap * 8 + d_scores.cap * 4 + d_offsets.cap * 8 + d_order.cap + d_terms.cap * 8 + d_accepted.cap * 8 +
               d_err.cap * 4 + d_perm.cap + d_swaps.cap * 8 + d_args.cap * sizeof(Mc3Args) + run_bytes();  // the tables apart: order_sumtables_plan counts them
    }
};

}  // namespace ulg
