// order_mcmc_dev.h -- the arithmetic of the order MCMC (order_mcmc.hip,
// ulg_order_mcmc_*, ulg_order_score; contract: include/ulg.h): the proposal
// from a draw, the shuffle's step, the accept rule, the 128-bit sum of an
// order term's weights and the term's final expression.  Host and device, as
// posterior_sample_dev.h is, whose Philox draw, fixed-point weight and pick it
// reuses, with linext_dev.h's two-word add: it compiles under hipcc and under
// a plain C++ compiler (host/order_mcmc_check.cpp).  Every path uses these
// definitions.
#pragma once

#include "linext_dev.h"
#include "posterior_sample_dev.h"

namespace ulg {

constexpr int kMcmcMaxVars = 63;             // a parent mask is one 64-bit word, the variable's own bit clear
constexpr int64_t kMcmcMaxChains = 1 << 20;  // one workgroup each, a launch's x dimension

// The draw of (step t, chain c, domain d): key (lo32(seed), hi32(seed)),
// counter (lo32(t), hi32(t), c, d).  d = 0: the move of step t; d = 1 + p: the
// parent set of position p of a record at step t; t = 0, d = p: the shuffle.
ULG_POST_HD void mcmc_draw(uint64_t seed, uint64_t t, uint32_t c, uint32_t d, uint32_t w[4]) {
    post_philox((uint32_t)t, (uint32_t)(t >> 32), c, d, (uint32_t)seed, (uint32_t)(seed >> 32), w);
}

// The proposal of a move's draw: positions i != j, both below n (n >= 2), and
// the 64-bit number the accept rule compares.
struct McmcMove {
    int i, j;
    uint64_t u_acc;
};
ULG_POST_HD McmcMove mcmc_move(const uint32_t w[4], int n) {
    McmcMove mv;
    mv.i = (int)post_mulhi32(w[0], (uint32_t)n);
    const int jp = (int)post_mulhi32(w[1], (uint32_t)(n - 1));
    mv.j = jp + (jp >= mv.i ? 1 : 0);
    mv.u_acc = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    return mv;
}

// The shuffle's step at position p >= 1: the position r <= p that p swaps with
ULG_POST_HD int mcmc_shuffle_pos(uint32_t w0, int p) { return (int)post_mulhi32(w0, (uint32_t)(p + 1)); }

// Chain c's initial order when none is given: from the identity, p = n-1 .. 1
ULG_POST_HD void mcmc_shuffle(uint64_t seed, uint32_t c, int n, uint8_t *order) {
    for (int p = 0; p < n; ++p) order[p] = (uint8_t)p;
    for (int p = n - 1; p >= 1; --p) {
        uint32_t w[4];
        mcmc_draw(seed, 0, c, (uint32_t)p, w);
        const int r = mcmc_shuffle_pos(w[0], p);
        const uint8_t x = order[p];
        order[p] = order[r];
        order[r] = x;
    }
}

// delta = -inf stands for a proposal with a term of -inf: never accepted.
ULG_POST_HD bool mcmc_accept(double delta, uint64_t u_acc) {
    if (!(delta > -INFINITY)) return false;
    if (delta >= 0.0) return true;
    return (u_acc >> 12) < post_weight_q(delta);
}

// sum of q[0 .. count) as lo + 2^64 hi
ULG_POST_HD LxCount mcmc_sum_q(const uint64_t *q, int64_t count) {
    LxCount T{0, 0};
    for (int64_t i = 0; i < count; ++i) T = lx_add(T, LxCount{q[i], 0});
    return T;
}

// a = m + log(T 2^-52) for the maximum m of the compatible scores and the sum T
// of their weights; T >= 2^52 (the maximum's own weight is exactly 2^52), and
// T = 2^52 gives y = 1, log(y) = 0 and a = m to the bit.
ULG_POST_HD double mcmc_term(double m, LxCount T) { return m + log(ldexp((double)T.hi, 12) + ldexp((double)T.lo, -52)); }

// The whole term of one variable over its list entries [b, e) with predecessor
// set U, one entry after the other (the check program and ulg_order_score's
// restatement on the host; the kernels stride the list by lanes and reduce the
// word pairs across the wave -- the integers are the same).
ULG_POST_HD double mcmc_term_serial(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t U) {
    double m = -INFINITY;
    for (int64_t i = b; i < e; ++i)
        if (!(sets[i] & ~U) && (double)scores[i] > m) m = (double)scores[i];
    if (!(m > -INFINITY)) return -INFINITY;
    LxCount T{0, 0};
    for (int64_t i = b; i < e; ++i)
        if (!(sets[i] & ~U)) T = lx_add(T, LxCount{post_weight_q((double)scores[i] - m), 0});
    return mcmc_term(m, T);
}

}  // namespace ulg
