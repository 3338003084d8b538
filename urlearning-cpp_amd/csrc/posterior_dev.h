// posterior_dev.h -- the arithmetic of the exact model averaging
// (posterior.hip, ulg_posterior*): the one logaddexp every kernel uses and the
// index helpers of the per-variable tables.  Host and device: it compiles under
// hipcc and under a plain C++ compiler (host/posterior_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ULG_POST_HD __host__ __device__ __forceinline__
#else
#define ULG_POST_HD inline
#endif

namespace ulg {

constexpr int kPostMaxVars = 28;  // n 2^(n-1) + 2^(n+1) + 2^(n-1) doubles: 35 GB at 28

// The gap above which logaddexp returns its maximum unchanged.  The term left
// out is log1p(exp(-d)) < exp(-38) = 3.2e-17 < 2^-54: below half an ulp of any
// maximum of magnitude >= 1/2 (the sum would round to the maximum anyway) and
// an absolute error below 5.6e-17 for a smaller one.
constexpr double kPostLogAddCut = 38.0;

// ln(exp(a) + exp(b)) = max + log1p(exp(-|a - b|)).  -inf stands for 0: with
// the smaller operand -inf the other is returned as it is (-inf when both
// are), and inf - inf is never formed (+inf gives +inf).  NaN does not occur:
// the lists' scores are checked finite before anything is computed.  The two
// early returns are what the transforms' short cuts are: a wave whose lanes
// all take one of them skips exp and log1p altogether.
ULG_POST_HD double post_logaddexp(double a, double b) {
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (!(lo > -INFINITY) || !(hi < INFINITY)) return hi;
    const double d = hi - lo;
    if (d > kPostLogAddCut) return hi;
    return hi + log1p(exp(-d));
}

// alpha_v and gamma_v are indexed by S, a subset of V \ {v}, with bit v
// squeezed out: 2^(n-1) entries.
ULG_POST_HD uint32_t post_squeeze(uint32_t S, int v) {  // bit v of S must be clear
    const uint32_t low = (1u << v) - 1u;
    return (S & low) | ((S >> 1) & ~low);
}
ULG_POST_HD uint32_t post_expand(uint32_t i, int v) {  // the inverse: a clear bit v put back
    const uint32_t low = (1u << v) - 1u;
    return (i & low) | ((i & ~low) << 1);
}
// V \ S \ {v} for the S of index i, as an index again: in squeezed form the
// complement within V \ {v} is the complement of the n - 1 index bits
ULG_POST_HD uint32_t post_complement(uint32_t i, int n) { return ~i & ((1u << (n - 1)) - 1u); }

}  // namespace ulg
