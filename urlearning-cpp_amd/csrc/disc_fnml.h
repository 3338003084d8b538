// disc_fnml.h -- the arithmetic of the fNML score (ULG_SCORE_FNML) that host
// and device share: the regret ln C(r, n) of the multinomial NML distribution,
// the fixed-point rule, the choice of its scale and the size rule of the
// device table.  Plain functions, usable without a GPU: host/fnml_check.cpp
// checks every one of them.
//
// Replaces fNMLScoringFunction::calculate / calculateScore and the regret
// lookup (fnml_scoring_function.cpp:17-74) and the literal table of
// fnml_scoring_function.h:300-340, which is computed here, not copied.
//
// For variable v of arity r and parent set P,
//     s(v, P) = sum_cells n_jk ln n_jk - sum_j n_j ln n_j - sum_{j : n_j > 0} ln C(r, n_j)
// BIC's log-likelihood with the regret of each non-empty parent configuration
// as the penalty.
//
// The regret of two values is the normaliser of the binomial NML distribution,
//     C(2, n) = sum_{h = 0..n} binom(n, h) (h / n)^h ((n - h) / n)^(n - h)     (0^0 = 1, C(2, 0) = 1)
// = 1, 2, 2.5, 26/9, ...  For n <= kFnmlExact = 1000 fnml_c2_table() is that
// sum, on the host, once per process, in long double.  With
// e(h) = (1 + 1/h)^h (e(0) = 1) and t_h the h-th term, t_0 = 1 and
//     t_{h+1} / t_h = e(h) / e(n - h - 1),
// so the terms follow from their neighbours by one multiplication and one
// division, and t_h = t_{n-h} halves the walk.  e(h) = exp(h log1p(1/h)), in long double, is
// good to about 2^-62 (the exponent is about 1 and carries log1pl's 2^-64 times
// h (1/h)); a term reached in h <= 500 steps is off by at most 3 h 2^-63
// relatively, the long double sum of <= 1001 positive terms adds 1001 2^-64:
// below 2^-53 of C(2, n) in all, so the FP64 value is the correctly rounded one
// or its neighbour.  (An FP64 lgamma form is 5e-14 off at n = 200.)
// For n > 1000 the regret is Szpankowski's three-term form, as in the reference:
//     C(2, n) ~ exp(ln(n pi / 2) / 2 + sqrt(8 / (9 n pi)) + (1/12 - 4 / (9 pi)) / n)
// in FP64.  It lies 5.46e-7 above the exact sum at n = 1001 (relatively, hence
// by the same amount in ln C), 5.0e-8 at n = 5000 and 6.3e-9 at n = 20000: the
// value of a parent configuration steps by 5.5e-7 between n_j = 1000 and 1001.
// That is the reference's own threshold.
//
// More values: C(k, n) = C(k-1, n) + n / (k - 2) C(k-2, n).  The reference runs
// it in float on the values, which turn infinite from 3.4e38 on (r = 60,
// n = 1000: ln C = 117.5).  Here it runs on the ratio rho_k = C(k, n) / C(k-1, n):
//     rho_2 = C(2, n)  (C(1, n) = 1),   rho_k = 1 + n / ((k - 2) rho_{k-1}),
//     ln C(k, n) = ln C(k-1, n) + ln rho_k,
// FP64 throughout.  1 < rho_k <= 1 + n, so nothing overflows:
// ln C(255, 100000) = 889.8.  ln C(1, n) = 0 and ln C(r, 0) = 0.
//
// Fixed point.  Every term -- n_jk ln n_jk, n_j ln n_j and each regret -- is
// rounded once to a multiple of 2^-shift and added as an integer, as for BIC
// and BDeu; the device table holds the regrets already fixed (int64), so a
// parent configuration costs one load and one integer add.  The scale: the
// cell counts add up to N and so do the configuration counts, so
//     sum |n ln n terms| <= 2 N ln N;
// C(r, n) counts weighted sequences, C(r, n) <= r^n, and the regret grows with
// r, so with rmax the largest arity loaded
//     sum_j ln C(r, n_j) <= sum_j n_j ln rmax = N ln rmax
// (Szpankowski's form exceeds the exact value by less than 1e-6 of it and stays
// far below 2^n).  There are at most N cells, N n_j ln n_j terms and N regrets;
// fixing adds at most 1/2 per term:
//     sum |fix(term)| <= 2^shift N (2 ln N + ln rmax) + 3 N / 2       (shift >= 0).
// fnml_shift takes U = N (2 ln N + ln rmax + 2) < 2^ex and shift =
// min(32, 62 - ex): 2^shift U <= 2^62 exceeds the line above by
// (2^(shift+1) - 3/2) N >= N / 2, far more than the rounding of U in FP64 and of
// the computed terms can take back.  Every partial sum stays below 2^62 in
// magnitude.  N < 2^31 and rmax <= 255 give U < 2^37: shift >= 25.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "score_plan.h"  // ULG_HD

namespace ulg {

constexpr int kFnmlExact = 1000;                   // C(2, n) is the exact sum up to here
constexpr int64_t kFnmlMaxEntries = 1ll << 28;     // the device table: 2 GiB of int64, ulg_disc_counts' stop

// C(2, n), n = 0 .. kFnmlExact, as above.  Host only; built at the first call.
inline const std::vector<double> &fnml_c2_table() {
    static const std::vector<double> table = [] {
        std::vector<long double> e(kFnmlExact + 1, 1.0L);  // e(h) = (1 + 1/h)^h
        for (int h = 1; h <= kFnmlExact; ++h) e[h] = std::exp((long double)h * std::log1p(1.0L / (long double)h));
        std::vector<double> t(kFnmlExact + 1);
        t[0] = 1.0;
        for (int n = 1; n <= kFnmlExact; ++n) {
            // terms 0 .. (n - 1) / 2 count twice; the middle one of an even n once
            long double term = 1.0L, sum = 0.0L;
            const int half = (n - 1) / 2;
            for (int h = 0; h <= half; ++h) {
                sum += term;
                term = term * e[h] / e[n - h - 1];
            }
            sum *= 2.0L;
            if (n % 2 == 0) sum += term;  // t_{n/2}
            t[n] = (double)sum;
        }
        return t;
    }();
    return table;
}

// C(2, n) for n > kFnmlExact
ULG_HD inline double fnml_c2_szpankowski(double n) {
    const double pi = 3.14159265358979323846;
    return exp(0.5 * log(n * pi / 2.0) + sqrt(8.0 / (9.0 * n * pi)) + (1.0 / 12.0 - 4.0 / (9.0 * pi)) / n);
}

// rho_k from rho_{k-1}, k >= 3
ULG_HD inline double fnml_next_ratio(double rho, double n, int k) { return 1.0 + n / ((double)(k - 2) * rho); }

// ln C(r, n) from c2 = C(2, n): r - 2 steps of the recurrence.  The table kernel
// runs the same loop and stores at the arities it needs.
ULG_HD inline double fnml_log_regret(int r, int64_t n, double c2) {
    if (r <= 1 || n <= 0) return 0.0;
    double rho = c2, lc = log(c2);
    for (int k = 3; k <= r; ++k) {
        rho = fnml_next_ratio(rho, (double)n, k);
        lc += log(rho);
    }
    return lc;
}

// one rounding (to nearest, ties to even) to a multiple of 2^-shift
ULG_HD inline long long fnml_fix(double term, int shift) { return llrint(ldexp(term, shift)); }

ULG_HD inline double fnml_unfix(long long sum, int shift) { return ldexp((double)sum, -shift); }

// U above: bounds sum |fix(term)| 2^-shift
ULG_HD inline double fnml_sum_bound(int64_t N, int rmax) {
    return (double)N * (2.0 * log((double)N) + log((double)(rmax < 2 ? 2 : rmax)) + 2.0);
}

// the largest power-of-two scale at which the bound stays below 2^62, at most 2^32
ULG_HD inline int fnml_shift(int64_t N, int rmax) {
    int ex = 0;
    (void)frexp(fnml_sum_bound(N, rmax), &ex);  // U < 2^ex
    const int s = 62 - ex;
    return s < 32 ? s : 32;
}

// The device table holds `rows` rows (one per distinct arity >= 2 of the loaded
// columns) of N + 1 entries: at most kFnmlMaxEntries in all.
inline bool fnml_table_fits(int rows, int64_t N) {
    return rows >= 0 && N >= 0 && (rows == 0 || N + 1 <= kFnmlMaxEntries / rows);
}

}  // namespace ulg
