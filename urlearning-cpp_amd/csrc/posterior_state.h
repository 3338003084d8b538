// posterior_state.h -- what a context keeps of the exact model averaging:
// the lists and tables of the last ulg_posterior* call (posterior.hip), which
// the sampler reads (posterior_sample.hip), and the sampler's own buffers.
#pragma once

#include <vector>

#include "ulg_internal.h"

namespace ulg {

struct PosteriorState {
    int n = 0;
    int64_t total = 0;     // list entries
    bool ready = false;    // the tables are those of a successful call
    bool kept = false;     // ... and gamma holds all n tables
    DevBuf<uint64_t> d_sets;
    DevBuf<float> d_scores;
    DevBuf<int64_t> d_offsets;
    std::vector<int64_t> offsets;  // their host copy (the source of the upload: it outlives the call)
    DevBuf<double> alpha, f, b, gamma;
    DevBuf<double> d_logpost, d_edge;
    DevBuf<unsigned int> d_err;
    size_t held_bytes() const {
        return d_sets.cap * 8 + d_scores.cap * 4 + d_offsets.cap * 8 + (alpha.cap + f.cap + b.cap + gamma.cap) * 8 +
               (d_logpost.cap + d_edge.cap) * 8 + d_err.cap * 4;
    }
    // ulg_posterior_sample*: the samples of one call on the device, and the
    // draws of ulg_posterior_sample_u.  Kept from one sampling call to the
    // next; every posterior call frees them before it sizes its own buffers
    // (drop_samples), so they never stand in the way of the tables.
    DevBuf<uint64_t> s_parents, s_u;
    DevBuf<uint8_t> s_order;
    DevBuf<double> s_weight;
    DevBuf<unsigned int> s_err;
    size_t sample_bytes() const { return s_parents.cap * 8 + s_u.cap * 8 + s_order.cap + s_weight.cap * 8 + s_err.cap * 4; }
    void drop_samples() {
        s_parents.reset();
        s_u.reset();
        s_order.reset();
        s_weight.reset();
        s_err.reset();
    }
};

}  // namespace ulg
