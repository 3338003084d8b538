// order_mcmc_state.h -- what a context keeps of the order MCMC
// (order_mcmc.hip): the device copy of the lists of the last
// ulg_order_mcmc_begin*, per chain the order, the terms and the accepted
// count, the global step, and the buffers a run's records and traces pass
// through.  Beside PosteriorState and apart from it: no call of either kind
// reads the other's, and a ulg_posterior* call deletes this one
// (order_mcmc_delete) before it sizes its tables.
#pragma once

#include <vector>

#include "ulg_internal.h"

namespace ulg {

struct OrderMcmcState {
    int n = 0;
    int64_t total = 0;   // list entries
    int64_t chains = 0;
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
    // the records and traces of one run, and ulg_order_score's orders and terms
    DevBuf<uint8_t> r_order, r_taccept;
    DevBuf<double> r_score, r_weight, r_tdelta;
    DevBuf<uint64_t> r_parents;
    size_t run_bytes() const {
        return r_order.cap + r_taccept.cap + (r_score.cap + r_weight.cap + r_tdelta.cap) * 8 + r_parents.cap * 8;
    }
    size_t held_bytes() const {
        return d_sets.cap * 8 + d_scores.cap * 4 + d_offsets.cap * 8 + d_order.cap + d_terms.cap * 8 + d_accepted.cap * 8 +
               d_err.cap * 4 + run_bytes();
    }
};

}  // namespace ulg
