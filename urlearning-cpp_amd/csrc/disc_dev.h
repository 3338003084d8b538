// disc_dev.h -- what the discrete kernels share (disc.hip: BIC scoring,
// disc_mmpc.hip: G^2 tests): the loaded records as the kernels see them and the
// fixed-point n ln n term that makes every sum independent of scheduling.
#pragma once

#include <algorithm>
#include <cmath>

#include "ulg_internal.h"

namespace ulg {

struct DiscData {
    const uint8_t *codes;  // [n][N]
    int64_t N;
    int n;
    int shift;             // fixed point: 2^-shift
    double half_ln_N;
    uint8_t arity[64];
};

// fix(n ln n): zero cells contribute nothing (ilogi[0] = 0), and 1 ln 1 = 0
__device__ __forceinline__ long long fix_nlogn(unsigned int n, int shift) {
    if (n <= 1u) return 0;
    return __double2ll_rn(ldexp((double)n * log((double)n), shift));
}

inline bool disc_ready(const ulg_ctx *c) { return c->disc_loaded && !c->loaded; }

inline DiscData disc_data(const ulg_ctx *c) {
    DiscData D{};
    D.codes = c->d_codes.p;
    D.N = c->N;
    D.n = c->n;
    // the largest power-of-two scale at which N ln N stays below 2^62, at most 2^32
    int ex = 0;
    (void)std::frexp((double)c->N * std::log((double)c->N), &ex);  // N ln N < 2^ex
    D.shift = std::min(32, 62 - ex);
    D.half_ln_N = std::log((double)c->N) / 2.0;
    for (int j = 0; j < c->n; ++j) D.arity[j] = (uint8_t)c->disc_arity[j];
    return D;
}

}  // namespace ulg
