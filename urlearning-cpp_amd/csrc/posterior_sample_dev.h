// posterior_sample_dev.h -- the integer arithmetic of the posterior sampler
// (posterior_sample.hip, ulg_posterior_sample*; contract: include/ulg.h): the
// Philox4x32-10 draw, a candidate's fixed-point weight and the pick of a
// candidate from a 64-bit draw.  Host and device, as posterior_dev.h is: it
// compiles under hipcc and under a plain C++ compiler
// (host/posterior_sample_check.cpp).  Every path uses these definitions.
#pragma once

#include "posterior_dev.h"

namespace ulg {

constexpr int kPostWeightBits = 52;  // a candidate of probability p weighs floor(p 2^52)

struct PostDraw {
    uint64_t sink, set;  // U_sink = w0 | w1 << 32, U_set = w2 | w3 << 32
};

ULG_POST_HD uint32_t post_mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): 10 rounds over the counter
// (c0 .. c3) with the key (k0, k1) bumped by the Weyl constants between rounds.
ULG_POST_HD void post_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = post_mulhi32(kM0, c0), lo0 = kM0 * c0;
        const uint32_t hi1 = post_mulhi32(kM1, c2), lo1 = kM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kW0;
        k1 += kW1;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// The two draws of step position i of sample k: key (lo32(seed), hi32(seed)),
// counter (lo32(k), hi32(k), i, 0).
ULG_POST_HD PostDraw post_draw(uint64_t seed, uint64_t k, uint32_t i) {
    uint32_t w[4];
    post_philox((uint32_t)k, (uint32_t)(k >> 32), i, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    PostDraw d;
    d.sink = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    d.set = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    return d;
}

// q = floor(exp(x) 2^52) of a candidate whose log-probability is x; 0 for
// x = -inf (a candidate of weight 0).  x is a log-probability: at most a few
// roundings above 0, so the product stays far below 2^64.  The product by 2^52
// is exact; what the integers inherit from FP64 is exp's rounding alone.
ULG_POST_HD uint64_t post_weight_q(double x) {
    if (!(x > -INFINITY)) return 0;
    return (uint64_t)floor(exp(x) * 4503599627370496.0);
}

// The high 64 bits of a * b
ULG_POST_HD uint64_t post_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The threshold of a pick among candidates whose weights sum to T: the choice
// is the first candidate j whose running sum C_j = q_0 + .. + q_j exceeds it.
// t < T whenever T > 0, so a candidate of weight 0 is never chosen: U = 0 gives
// the first candidate with q > 0, U = 2^64 - 1 gives t = T - 1 and the last.
ULG_POST_HD uint64_t post_pick_threshold(uint64_t U, uint64_t T) { return post_mulhi64(U, T); }

// The pick itself over an array (the check program and the host's restatement;
// the kernel forms the running sums by a scan across the wave): the index of
// the chosen candidate, `count` when every weight is 0.
ULG_POST_HD int64_t post_pick(const uint64_t *q, int64_t count, uint64_t U) {
    uint64_t T = 0;
    for (int64_t j = 0; j < count; ++j) T += q[j];
    const uint64_t t = post_pick_threshold(U, T);
    uint64_t C = 0;
    for (int64_t j = 0; j < count; ++j) {
        C += q[j];
        if (C > t) return j;
    }
    return count;
}

}  // namespace ulg
