// bge_dev.h -- the one device function that computes a BGe value (bge.h), and
// what the two kernels of bge.hip share around it.
//
// One operation order.  q[0 .. L) are the parents in ascending variable order,
// q[L] is the variable.  Column by column, a Cholesky factorisation of
// R[Q,Q] = G[Q,Q] + t I with the variable last:
//     s_j  = (G[q_j,q_j] + t) - sum_{k<j} l_jk^2          one fma per k, k ascending
//     l_ij = (G[q_i,q_j] - sum_{k<j} l_ik l_jk) / sqrt(s_j)   as t * (1 / sqrt(s_j))
// det R[P,P] is the running product of s_0 .. s_{L-1} (1 for no parent; it
// cannot leave the FP64 range for N < 2^31, L <= 31 and t >= 5e-7: every pivot
// lies between about t and N), sigma is s_L, and the value is
//     fma(-A_L, ln sigma, fma(-1/2, ln prod, c_L))
// rounded to float once.  A pivot that is not > 0 (a NaN from a constant column
// included) gives NaN.  Every multiply-add is an explicit fma, so the unrolled
// instances (LC = 1 .. 8: L is a constant, the factor lives in registers) and
// the generic one (LC = 0: L at run time, the factor in scratch) perform the
// same operations on the same operands: a pair's value is the same bits from
// every kernel, for any grid and in every call.
#pragma once

#include "bge.h"
#include "ulg_internal.h"

namespace {

constexpr int kBgeBlock = 256;

template <int LC>
struct BgeDim {
    static constexpr int kMax = (LC > 0 ? LC : ulg::kWideMax) + 1;  // |Q| at most
    static constexpr int kUnroll = LC > 0 ? kMax : 1;               // full, or none
};

// row q of an n x n matrix (< 2^24: a full-rate 24-bit multiply on the device)
__host__ __device__ __forceinline__ int bge_row(int q, int n) {
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(q, n);
#else
    return q * n;
#endif
}

// g: G (n x n, row-major, in LDS); tab: [0, 32) c_l, [32, 64) A_l.  Compiles
// for the host too, where a test program can run the same text.
template <int LC>
__host__ __device__ __forceinline__ float bge_set_score(const double *g, int n, const int (&q)[BgeDim<LC>::kMax], int Lrt, double t,
                                               const double *tab) {
    constexpr int DM = BgeDim<LC>::kMax;
    constexpr int UN = BgeDim<LC>::kUnroll;
    const int L = LC > 0 ? LC : Lrt;
    const int D = L + 1;
    double Lm[DM * (DM + 1) / 2];
    double prod = 1.0, sigma = 0.0;
    bool ok = true;
#pragma unroll UN
    for (int j = 0; j < D; ++j) {
        const int rj = j * (j + 1) / 2;
        const int qj = q[j];
        const int roj = bge_row(qj, n);
        double s = g[roj + qj] + t;
#pragma unroll UN
        for (int k = 0; k < j; ++k) s = fma(-Lm[rj + k], Lm[rj + k], s);
        ok = ok && (s > 0.0);
        if (j < L) {
            prod *= s;
            const double inv = 1.0 / sqrt(s);
#pragma unroll UN
            for (int i = j + 1; i < D; ++i) {
                const int ri = i * (i + 1) / 2;
                double x = g[bge_row(q[i], n) + qj];
#pragma unroll UN
                for (int k = 0; k < j; ++k) x = fma(-Lm[ri + k], Lm[rj + k], x);
                Lm[ri + j] = x * inv;
            }
        } else {
            sigma = s;
        }
    }
    const double val = fma(-tab[ulg::kBgeLayers + L], log(sigma), fma(-0.5, log(prod), tab[L]));
    return ok ? (float)val : __builtin_nanf("");
}

// ulg_cbic_set_constraints' by-variable table in variable masks (cbic_layer_dev.h
// cons_violates): words [0, n] prefix the variables' alternatives, then one
// (required, forbidden) pair per alternative.
__device__ __forceinline__ bool bge_violates(const uint64_t *ct, int n, int v, uint64_t set) {
    const uint64_t b = ct[v], e = ct[v + 1];
    if (b == e) return false;
    const uint64_t *p = ct + n + 1 + 2 * b;
    for (uint64_t i = 0; i < e - b; ++i)
        if ((p[2 * i] & ~set) == 0 && (p[2 * i + 1] & set) == 0) return false;
    return true;
}

}  // namespace
