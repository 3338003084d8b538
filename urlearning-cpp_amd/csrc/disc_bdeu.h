// disc_bdeu.h -- the arithmetic of the BDeu score (ULG_SCORE_BDEU) that host
// and device share: the per-item parameters, the two kinds of term, the
// fixed-point rule and the choice of its scale.  Plain functions, usable
// without a GPU: host/bdeu_check.cpp checks the scale and the fix rule.
//
// Replaces BDeuScoringFunction::lg and the arithmetic of calculate /
// calculateScore (bdeu_scoring_function.cpp:21-35, 117-122, 133-140).
//
// For variable v of arity r, parent set P, q = prod r_p, cells = q r < 2^63:
//     a_j = ess / q      a_jk = ess / cells                           (FP64)
//     s(v, P) = sum over non-empty cells   [ lgamma(a_jk + n_jk) - lgamma(a_jk) ]
//             + sum over non-empty configs [ lgamma(a_j) - lgamma(a_j + n_j) ]
// Each bracket is one term: computed in FP64 from the exact count, rounded once
// to a multiple of 2^-shift (bdeu_fix) and added as an integer.  A term is a
// function of (a, lgamma(a), n) alone and integer adds commute, so the sum does
// not depend on which kernel path counted or on the scheduling.
//
// The scale.  With Gamma(x + 1) = x Gamma(x),
//     lgamma(a + n) - lgamma(a) = sum_{i < n} ln(a + i).
// Every a here lies in [ess 2^-63, ess] (a_j >= a_jk = ess / cells, cells <
// 2^63) and n <= N, so ess 2^-63 <= a + i < ess + N and
//     |ln(a + i)| <= Lm := max(-ln(ess 2^-63), ln(ess + N)),
// hence |term(a, n)| <= n Lm.  The cell counts add up to N and so do the
// configuration counts: sum |term| <= 2 N Lm over at most 2 N terms.  Fixing
// adds at most 1/2 per term, so the integers satisfy
//     sum |fix(term)| <= 2^shift 2 N Lm + N                  (shift >= 0).
// bdeu_shift takes U = 2 N (Lm + 1) < 2^ex and shift = min(32, 62 - ex):
// 2^shift U <= 2^62 exceeds the line above by (2^(shift+1) - 1) N >= N, which
// is far more than the rounding of U itself in FP64 (relative 2^-50 of
// U <= 118 x 2 N) and of the computed terms (a few ulps of lgamma each) can
// take back.  Every partial sum therefore stays below 2^62 in magnitude, and
// no smaller ex does that for the bound U.  N < 2^31 and ess <= 1e6 give
// U < 2^39: shift >= 23.
#pragma once

#include <cmath>
#include <cstdint>

#include "score_plan.h"  // ULG_HD

namespace ulg {

constexpr double kBdeuEssMin = 1e-6, kBdeuEssMax = 1e6;  // ulg_disc_set_ess

// What thread 0 computes once per item.
struct BdeuItem {
    double a_j, a_jk;    // ess / q, ess / (q r)
    double lg_j, lg_jk;  // lgamma of the two
};

ULG_HD inline BdeuItem bdeu_item(double ess, uint64_t q, uint64_t cells) {
    BdeuItem b;
    b.a_j = ess / (double)q;
    b.a_jk = ess / (double)cells;
    b.lg_j = lgamma(b.a_j);
    b.lg_jk = lgamma(b.a_jk);
    return b;
}

// the term of a non-empty cell, n = n_jk >= 1
ULG_HD inline double bdeu_cell_term(const BdeuItem &b, unsigned int n) { return lgamma(b.a_jk + (double)n) - b.lg_jk; }

// the term of a non-empty parent configuration, n = n_j >= 1
ULG_HD inline double bdeu_cfg_term(const BdeuItem &b, unsigned int n) { return b.lg_j - lgamma(b.a_j + (double)n); }

// one rounding (to nearest, ties to even) to a multiple of 2^-shift
ULG_HD inline long long bdeu_fix(double term, int shift) { return llrint(ldexp(term, shift)); }

ULG_HD inline double bdeu_unfix(long long sum, int shift) { return ldexp((double)sum, -shift); }

// Lm above
ULG_HD inline double bdeu_log_extreme(int64_t N, double ess) {
    return fmax(-log(ldexp(ess, -63)), log(ess + (double)N));
}

// U above: bounds sum |fix(term)| 2^-shift
ULG_HD inline double bdeu_sum_bound(int64_t N, double ess) {
    return 2.0 * (double)N * (bdeu_log_extreme(N, ess) + 1.0);
}

// the largest power-of-two scale at which the bound stays below 2^62, at most 2^32
ULG_HD inline int bdeu_shift(int64_t N, double ess) {
    int ex = 0;
    (void)frexp(bdeu_sum_bound(N, ess), &ex);  // U < 2^ex
    const int s = 62 - ex;
    return s < 32 ? s : 32;
}

}  // namespace ulg
