// bge_check -- the prior and the constants of the BGe score (csrc/bge.h) on the
// host.
//   bge_check                          the checks below
//   bge_check N n alpha_mu alpha_w     prints t, then "l c_l A_l" for l = 0 .. 31
//                                      ("%.17g"; alpha_w = 0: the default), for
//                                      tests/test_bge.py to hold against its reference
// The checks, over a grid of (N, n, alpha_mu, alpha_w) that holds the corners
// N = 2 and 2^31 - 1, n = 1 and 63, alpha_mu = 1e-3 and 1e3, alpha_w just above
// n + 1 and n + 1e6:
//   1. the range predicates of ulg_bge_set_prior, NaN and infinities included;
//   2. alpha_w = 0 is n + alpha_mu + 1 and gives t = alpha_mu^2 / (alpha_mu + 1);
//      t > 0 over the whole range (at least 5e-7 at the default alpha_w);
//   3. A_{l+1} = A_l + 1/2 exactly -- what makes the score equivalent: the two
//      orders of a pair differ by (A_1 - A_0 - 1/2) ln R[x,x] / R[y,y];
//   4. c_{l+1} - c_l = [lgamma(A_l + 1/2) - lgamma(A_l)] - [lgamma(B_l + 1/2) -
//      lgamma(B_l)] + ln t with B_l = (alpha_w - n + l + 1) / 2, against long
//      double, within 64 ulps of the largest term;
//   5. every c_l and A_l is finite.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "../csrc/bge.h"

using namespace ulg;

namespace {

long g_checks = 0;
long long g_N = 0;
int g_n = 0, g_l = 0;
double g_am = 0, g_aw = 0;

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) {                                                                                       \
            std::fprintf(stderr, "bge_check: %s:%d: %s fails (N=%lld n=%d alpha_mu=%g alpha_w=%g l=%d)\n",    \
                         __FILE__, __LINE__, #cond, g_N, g_n, g_am, g_aw, g_l);                              \
            std::exit(1);                                                                                    \
        }                                                                                                    \
    } while (0)

int print_table(char **argv) {
    const long long N = std::atoll(argv[1]);
    const int n = std::atoi(argv[2]);
    const double am = std::strtod(argv[3], nullptr), aw = std::strtod(argv[4], nullptr);
    if (N < 2 || n < 1 || n > 63 || !bge_alpha_mu_ok(am) || !bge_alpha_w_ok(aw, n)) {
        std::fprintf(stderr, "bge_check: arguments out of range\n");
        return 2;
    }
    const BgeConsts k = bge_consts(N, n, am, aw);
    std::printf("t %.17g\n", k.t);
    for (int l = 0; l < kBgeLayers; ++l) std::printf("%d %.17g %.17g\n", l, k.tab[l], k.tab[kBgeLayers + l]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 5) return print_table(argv);
    if (argc != 1) {
        std::fprintf(stderr, "usage: bge_check [N n alpha_mu alpha_w]\n");
        return 2;
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // 1. the ranges
    CHECK(kBgeAlphaMuMin == 1e-3 && kBgeAlphaMuMax == 1e3 && kBgeAlphaWSpan == 1e6 && kBgeLayers == 32);
    CHECK(bge_alpha_mu_ok(1e-3) && bge_alpha_mu_ok(1.0) && bge_alpha_mu_ok(1e3));
    CHECK(!bge_alpha_mu_ok(0.0) && !bge_alpha_mu_ok(-1.0) && !bge_alpha_mu_ok(9.99e-4) && !bge_alpha_mu_ok(1000.5));
    CHECK(!bge_alpha_mu_ok(nan) && !bge_alpha_mu_ok(inf) && !bge_alpha_mu_ok(-inf));
    CHECK(bge_alpha_w_ok(0.0, 0) && bge_alpha_w_ok(1.5, 0) && !bge_alpha_w_ok(1.0, 0) && !bge_alpha_w_ok(-2.0, 0));
    for (int n : {1, 10, 63}) {
        g_n = n;
        CHECK(bge_alpha_w_ok(0.0, n) && bge_alpha_w_ok(n + 1.5, n) && bge_alpha_w_ok(n + 1e6, n));
        CHECK(!bge_alpha_w_ok(n + 1.0, n) && !bge_alpha_w_ok((double)n, n) && !bge_alpha_w_ok(-1.0, n));
        CHECK(!bge_alpha_w_ok(n + 1e6 + 1.0, n) && !bge_alpha_w_ok(nan, n) && !bge_alpha_w_ok(inf, n) && !bge_alpha_w_ok(-inf, n));
    }
    const long long Ns[] = {2, 8, 50, 1000, 10000, 62000000, (1ll << 31) - 1};
    const int ns[] = {1, 2, 10, 25, 32, 63};
    const double ams[] = {1e-3, 0.1, 1.0, 7.5, 1e3};
    double worst = 0.0, tmin = inf;
    for (long long N : Ns)
        for (int n : ns)
            for (double am : ams) {
                const double aws[] = {0.0, n + 1.0 + 1e-3, n + 5.0, n + 1e6};
                for (double aw : aws) {
                    g_N = N, g_n = n, g_am = am, g_aw = aw, g_l = -1;
                    CHECK(bge_alpha_w_ok(aw, n));
                    const double w = bge_alpha_w(am, aw, n);
                    const BgeConsts k = bge_consts(N, n, am, aw);
                    // 2. the default and t
                    if (aw == 0.0) {
                        CHECK(w == (double)n + am + 1.0);
                        CHECK(std::fabs(k.t - am * am / (am + 1.0)) <= 4 * 0x1p-52 * (double)(n + 2));
                        CHECK(k.t >= 5e-7);
                        tmin = k.t < tmin ? k.t : tmin;
                    }
                    CHECK(k.t > 0.0 && std::isfinite(k.t));
                    const long double lt = std::log((long double)k.t);
                    for (int l = 0; l < kBgeLayers; ++l) {
                        g_l = l;
                        const double A = k.tab[kBgeLayers + l], c = k.tab[l];
                        // 5.
                        CHECK(std::isfinite(A) && std::isfinite(c) && A > 0.0);
                        if (l + 1 == kBgeLayers) break;
                        // 3.
                        CHECK(k.tab[kBgeLayers + l + 1] == A + 0.5);
                        // 4.
                        const long double B = ((long double)w - n + l + 1) / 2;
                        const long double dA = std::lgamma((long double)A + 0.5L) - std::lgamma((long double)A);
                        const long double dB = std::lgamma(B + 0.5L) - std::lgamma(B);
                        const long double want = dA - dB + lt;
                        // the largest term of either c: lgamma(A), (N / 2) ln pi and the ln t term
                        const double big = std::fmax(std::fmax(std::fabs(std::lgamma(A + 0.5)), 0.5724 * (double)N),
                                                     std::fabs((double)lt) * (w - n + 2.0 * l + 3.0) / 2.0);
                        const double err = (double)std::fabs((long double)k.tab[l + 1] - (long double)c - want);
                        const double tol = 64 * 0x1p-52 * std::fmax(big, 1.0);
                        CHECK(err <= tol);
                        worst = std::fmax(worst, err / tol);
                    }
                }
            }
    std::printf("bge_check ok (%ld checks, smallest default t %.3g, step error at most %.3f of its bound)\n", g_checks, tmin,
                worst);
    return 0;
}
