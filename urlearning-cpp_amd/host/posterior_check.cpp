// posterior_check -- the arithmetic of the exact model averaging
// (csrc/posterior_dev.h) on the host.
//   1. the index helpers, exhaustively for n <= 12: post_squeeze and
//      post_expand are inverse bijections between the subsets of V \ {v} and
//      0 .. 2^(n-1) - 1, they keep the subset order (S subset of S' iff the
//      indices are), and post_complement is the complement within V \ {v};
//   2. post_logaddexp at -inf and +inf (no NaN, inf - inf never formed), at
//      equal operands (ln 2 above them), on both sides of the cut-off gap and
//      for 0 against +-1e4; symmetric in its operands; against long double
//      within 4 ulps (exp, log1p and the sum) over a grid of gaps;
//   3. a 3-variable recursion worked by hand: the tables of the header's
//      contract written out term by term against the sum over the 6 orders.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "../csrc/posterior_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        ++g_checks;                                                                              \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "posterior_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

const double kInf = std::numeric_limits<double>::infinity();

double ulp_of(double x) { return std::nextafter(std::fabs(x), kInf) - std::fabs(x); }

void check_index() {
    for (int n = 1; n <= 12; ++n) {
        const uint32_t half = 1u << (n - 1), full = (1u << n) - 1u;
        for (int v = 0; v < n; ++v) {
            uint32_t prev = 0;
            for (uint32_t i = 0; i < half; ++i) {
                const uint32_t S = post_expand(i, v);
                CHECK(S <= full && !((S >> v) & 1u));
                CHECK(post_squeeze(S, v) == i);
                CHECK(__builtin_popcount(S) == __builtin_popcount(i));
                CHECK(i == 0 || S > prev);  // monotone: colex order is kept
                prev = S;
                const uint32_t c = post_complement(i, n);
                CHECK(c < half && post_expand(c, v) == (full & ~S & ~(1u << v)));
                CHECK(post_complement(c, n) == i);
                // subset order: one more element of V \ {v} in S is one more bit in i
                for (int u = 0; u < n; ++u)
                    if (u != v && !((S >> u) & 1u)) {
                        const uint32_t j = post_squeeze(S | (1u << u), v);
                        CHECK((j & i) == i && __builtin_popcount(j ^ i) == 1);
                    }
            }
        }
    }
}

void check_logaddexp() {
    const double ln2 = 0.69314718055994530942;
    CHECK(post_logaddexp(-kInf, -kInf) == -kInf);
    CHECK(post_logaddexp(-kInf, 3.5) == 3.5 && post_logaddexp(3.5, -kInf) == 3.5);
    CHECK(post_logaddexp(-kInf, -2e4) == -2e4 && post_logaddexp(-kInf, 0.0) == 0.0);
    CHECK(post_logaddexp(kInf, 1.0) == kInf && post_logaddexp(1.0, kInf) == kInf);
    CHECK(post_logaddexp(kInf, kInf) == kInf && post_logaddexp(kInf, -kInf) == kInf);
    for (double x : {0.0, 1.0, -1.0, 1e4, -1e4, 2e4, -2e4, 1e-300, 123.456})
        CHECK(std::fabs(post_logaddexp(x, x) - (x + ln2)) <= ulp_of(x + ln2));
    // the cut: beyond it the maximum itself, up to it the sum
    CHECK(kPostLogAddCut == 38.0 && std::exp(-kPostLogAddCut) < 0x1p-54);
    for (double hi : {0.0, 0.5, 1.0, -7.25, 2e4, -2e4}) {
        const double above = std::nextafter(hi - kPostLogAddCut, -kInf) - 1e-9 * (1.0 + std::fabs(hi));
        CHECK(hi - above > kPostLogAddCut);
        CHECK(post_logaddexp(hi, above) == hi && post_logaddexp(above, hi) == hi);
        CHECK(post_logaddexp(hi, hi - 39.0) == hi && post_logaddexp(hi, hi - 1e4) == hi);
        // what the cut leaves out is below half an ulp of a maximum >= 1/2, and below 2^-54 always
        CHECK(std::exp(-(hi - above)) < 0x1p-54);
        if (std::fabs(hi) >= 0.5) CHECK(std::exp(-(hi - above)) <= 0.5 * ulp_of(hi));
        const double below = hi - 37.0;  // exactly representable gaps within the cut
        if (hi - below <= kPostLogAddCut) {
            const double got = post_logaddexp(hi, below);
            CHECK(got >= hi && std::fabs(got - (hi + std::log1p(std::exp(-37.0)))) <= ulp_of(hi));
            if (hi == 0.0) CHECK(got > 0.0);  // a maximum of 0 keeps the small term
        }
    }
    CHECK(post_logaddexp(0.0, 1e4) == 1e4 && post_logaddexp(0.0, -1e4) == 0.0);
    CHECK(post_logaddexp(1e4, 0.0) == 1e4 && post_logaddexp(-1e4, 0.0) == 0.0);
    // against long double, symmetric
    for (double a : {-2e4, -311.5, -1.0, 0.0, 0.3, 17.0, 2e4})
        for (double d = 0.0; d <= 37.75; d += 0.37) {
            const double b = a - d, got = post_logaddexp(a, b);
            CHECK(got == post_logaddexp(b, a));
            const long double want = (long double)a + log1pl(expl(-(long double)(a - b)));
            CHECK(std::fabs((double)((long double)got - want)) <= 4 * ulp_of((double)want));
        }
}

// n = 3, lists: 0: {} w 2, {1} w 3;  1: {} w 5, {0,2} w 7;  2: {} w 11, {0} w 13, {0,1} w 17.
// By hand, over the six orders (each term the product of alpha_v(predecessors)):
//   012: 2 * (5) * (11+13+17) = 410      021: 2 * (11+13) * (5+7) = 576
//   102: 5 * (2+3) * (11+13+17) = 1025   120: 5 * (11) * (2+3) = 275
//   201: 11 * (2) * (5+7) = 264          210: 11 * (5) * (2+3) = 275
//   Z = 2825
// p(Pa_2 = {0,1}) = 17 (2*5 + 5*5) / 2825 = 595 / 2825  (orders 012 and 102)
// p(Pa_1 = {0,2}) = 7 (2*24 + 11*2) / 2825 = 490 / 2825  (orders 021 and 201)
void check_by_hand() {
    const int n = 3;
    const double w[3][4] = {// alpha lists by squeezed index (bit order of V \ {v})
                            {2, 3, 0, 0},     // 0: {} , {1}          (index bits: 1, 2)
                            {5, 0, 0, 7},     // 1: {} , {0,2}        (index bits: 0, 2)
                            {11, 13, 0, 17}};  // 2: {} , {0}, {0,1}   (index bits: 0, 1)
    double alpha[3][4], f[8], b[8];
    for (int v = 0; v < n; ++v) {
        for (int i = 0; i < 4; ++i) alpha[v][i] = w[v][i] > 0 ? std::log(w[v][i]) : -kInf;
        for (int bit = 0; bit < 2; ++bit)
            for (int i = 0; i < 4; ++i)
                if (i & (1 << bit)) alpha[v][i] = post_logaddexp(alpha[v][i], alpha[v][i ^ (1 << bit)]);
    }
    const double tol = 1e-14;
    CHECK(std::fabs(std::exp(alpha[2][3]) - 41.0) <= 41 * tol && std::fabs(std::exp(alpha[1][3]) - 12.0) <= 12 * tol);
    CHECK(std::fabs(std::exp(alpha[1][1]) - 5.0) <= 5 * tol && std::fabs(std::exp(alpha[0][2]) - 2.0) <= 2 * tol);
    f[0] = b[0] = 0.0;
    for (int layer = 1; layer <= n; ++layer)
        for (uint32_t S = 1; S < 8; ++S) {
            if (__builtin_popcount(S) != layer) continue;
            double fa = -kInf, ba = -kInf;
            for (int v = 0; v < n; ++v)
                if ((S >> v) & 1u) {
                    const uint32_t P = S ^ (1u << v);
                    fa = post_logaddexp(fa, f[P] + alpha[v][post_squeeze(P, v)]);
                    ba = post_logaddexp(ba, alpha[v][post_squeeze(7u & ~S, v)] + b[P]);
                }
            f[S] = fa, b[S] = ba;
        }
    CHECK(std::fabs(std::exp(f[7]) - 2825.0) <= 2825 * tol);
    CHECK(std::fabs(std::exp(b[7]) - 2825.0) <= 2825 * tol);
    // f({0,1}) = 2*5 + 5*5 = 35: the orders of {0,1} that fit the lists
    CHECK(std::fabs(std::exp(f[3]) - 35.0) <= 35 * tol);
    double gamma[3][4];
    for (int v = 0; v < n; ++v) {
        for (uint32_t i = 0; i < 4; ++i) gamma[v][i] = f[post_expand(i, v)] + b[post_expand(post_complement(i, n), v)];
        for (int bit = 0; bit < 2; ++bit)
            for (int i = 0; i < 4; ++i)
                if (!(i & (1 << bit))) gamma[v][i] = post_logaddexp(gamma[v][i], gamma[v][i | (1 << bit)]);
        // sum_S g_v(S) alpha_v(S) = Z: with gamma, sum over the stored sets of w gamma
        double tot = 0.0;
        for (int i = 0; i < 4; ++i)
            if (w[v][i] > 0) tot += w[v][i] * std::exp(gamma[v][i]);
        CHECK(std::fabs(tot - 2825.0) <= 2825 * tol);
    }
    CHECK(std::fabs(17.0 * std::exp(gamma[2][3]) - 595.0) <= 595 * tol);
    CHECK(std::fabs(7.0 * std::exp(gamma[1][3]) - 490.0) <= 490 * tol);
}

}  // namespace

int main() {
    check_index();
    check_logaddexp();
    check_by_hand();
    std::printf("posterior_check ok (%ld checks)\n", g_checks);
    return 0;
}
