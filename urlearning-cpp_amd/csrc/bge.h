// bge.h -- the prior of the BGe score (ulg_bge_*) and the constants that do
// not depend on the data: host only, usable without a GPU (host/bge_check.cpp).
//
// BGe, the Bayesian Gaussian equivalent score (Geiger & Heckerman 2002, in the
// corrected form of Kuipers, Moffa & Heckerman 2014), on the normalised data of
// ulg_cbic_load (zero mean, unit sample variance, G = Z'Z):
//     prior mean nu = 0, alpha_mu > 0 (default 1),
//     alpha_w > n + 1 (default n + alpha_mu + 1),
//     T = t I,  t = alpha_mu (alpha_w - n - 1) / (alpha_mu + 1),  R = G + t I.
// For |P| = l and A_l = (N + alpha_w - n + l + 1) / 2:
//     s(v, P) = c_l - 1/2 ln det R[P,P] - A_l ln sigma
//     sigma   = R[v,v] - R[v,P] R[P,P]^-1 R[P,v]
//     c_l     = lgamma(A_l) - lgamma((alpha_w - n + l + 1) / 2) - (N / 2) ln pi
//               + 1/2 ln(alpha_mu / (N + alpha_mu)) + ((alpha_w - n + 2 l + 1) / 2) ln t
// c_l and A_l are what this header computes, once per (N, n, alpha_mu,
// alpha_w); the kernels (bge_dev.h) read them from a device table.
#pragma once

#include <cmath>
#include <cstdint>

namespace ulg {

constexpr double kBgeAlphaMuMin = 1e-3, kBgeAlphaMuMax = 1e3;  // ulg_bge_set_prior
constexpr double kBgeAlphaWSpan = 1e6;                         // n + 1 < alpha_w <= n + 1e6
constexpr int kBgeLayers = 32;                                 // l = 0 .. ULG_MAX_PARENTS_GPU

// !(a <= x && x <= b) is also true for a NaN
inline bool bge_alpha_mu_ok(double am) { return am >= kBgeAlphaMuMin && am <= kBgeAlphaMuMax; }
// 0 stands for the default; anything else must leave t > 0
inline bool bge_alpha_w_ok(double aw, int n) {
    return aw == 0.0 || (aw > (double)(n + 1) && aw <= (double)n + kBgeAlphaWSpan);
}
inline double bge_alpha_w(double am, double aw, int n) { return aw == 0.0 ? (double)n + am + 1.0 : aw; }
inline double bge_t(double am, double aw_eff, int n) { return am * (aw_eff - (double)n - 1.0) / (am + 1.0); }

// The device table: [0, 32) c_l, [32, 64) A_l.
struct BgeConsts {
    double t;
    double tab[2 * kBgeLayers];
};

inline BgeConsts bge_consts(int64_t N, int n, double am, double aw) {
    BgeConsts k;
    const double w = bge_alpha_w(am, aw, n);
    const double dN = (double)N, dn = (double)n;
    k.t = bge_t(am, w, n);
    const double lnpi = std::log(3.14159265358979323846264338327950288);
    for (int l = 0; l < kBgeLayers; ++l) {
        const double dl = (double)l;
        const double A = (dN + w - dn + dl + 1.0) / 2.0;
        k.tab[kBgeLayers + l] = A;
        k.tab[l] = std::lgamma(A) - std::lgamma((w - dn + dl + 1.0) / 2.0) - (dN / 2.0) * lnpi +
                   0.5 * std::log(am / (dN + am)) + ((w - dn + 2.0 * dl + 1.0) / 2.0) * std::log(k.t);
    }
    return k;
}

}  // namespace ulg
