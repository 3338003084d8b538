// order_sumtables_check -- the arithmetic of the order MCMC's log-sum tables
// (csrc/order_sumtables_dev.h) on the host: on random lists -- tied scores,
// gaps beyond the 38-nat cut, variables without the empty set, empty lists, a
// list of the empty set alone -- every slot of the serial scatter and
// butterfly against a direct long-double logsumexp over the entries inside
// the expanded subset:
//   -inf exactly where no entry is inside, and only there;
//   a subset with one entry inside holds that score's bits;
//   every other slot within K (6.25 2^-52 + ulp + e^-38): per round the
//   rounding of d, exp, log1p, the add and the cut (tests/order_sumtables_ref.py
//   derives it; the host's libm is inside the 4 ulp allowed there);
// and idx_v(U) finds the slot of any predecessor set U.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/order_sumtables_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;
double g_worst = 0.0;  // the largest error as a fraction of its cap

#define CHECK(cond)                                                                                    \
    do {                                                                                               \
        ++g_checks;                                                                                    \
        if (!(cond)) {                                                                                 \
            std::fprintf(stderr, "order_sumtables_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                              \
        }                                                                                              \
    } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

double ulp(double x) { return std::nextafter(std::fabs(x), INFINITY) - std::fabs(x); }

// ln sum exp(s_i) over the entries inside U, long double around the maximum; *inside = how many; *mag = the largest |s_i|
long double direct(const std::vector<uint64_t> &sets, const std::vector<float> &scores, uint64_t U, int *inside, double *mag) {
    long double m = -INFINITY;
    *inside = 0, *mag = 0.0;
    for (size_t i = 0; i < sets.size(); ++i)
        if (!(sets[i] & ~U)) {
            ++*inside;
            if ((long double)scores[i] > m) m = scores[i];
            if (std::fabs((double)scores[i]) > *mag) *mag = std::fabs((double)scores[i]);
        }
    if (!*inside) return -INFINITY;
    long double sum = 0;
    for (size_t i = 0; i < sets.size(); ++i)
        if (!(sets[i] & ~U)) sum += expl((long double)scores[i] - m);
    return m + logl(sum);
}

// One variable's list: `count` random sets inside a random pool of K candidates of n variables
void check_build(int n, int K, int count, bool empty_set, float spread) {
    uint64_t pool = 0;
    while (ot_popcount(pool) < K) pool |= 1ull << (rnd() % n);
    std::vector<uint64_t> sets;
    std::vector<float> scores;
    if (empty_set) sets.push_back(0);
    for (int k = 0; k < count; ++k) {
        const uint64_t P = ot_expand(pool, (uint32_t)(rnd() & rnd() & ((1ull << K) - 1)));
        bool dup = P == 0;
        for (uint64_t Q : sets) dup = dup || Q == P;
        if (!dup) sets.push_back(P);
    }
    for (size_t i = 0; i < sets.size(); ++i) scores.push_back(-(float)(rnd() % 64) * spread);  // a grid: ties; spread 2: gaps past the cut
    const int64_t e = (int64_t)sets.size();
    const uint64_t C = ot_candidates(sets.data(), 0, e);
    const int Kc = ot_popcount(C);
    std::vector<double> L((size_t)ot_slots(Kc) + 1, 12345.0);  // a guard slot behind the table
    ost_build_serial(sets.data(), scores.data(), 0, e, C, L.data());
    CHECK(L.back() == 12345.0);
    for (int64_t x = 0; x < ot_slots(Kc); ++x) {
        int inside;
        double mag;
        const long double want = direct(sets, scores, ot_expand(C, (uint32_t)x), &inside, &mag);
        if (!inside) {
            CHECK(L[x] == -INFINITY);
            continue;
        }
        CHECK(L[x] > -INFINITY);
        if (inside == 1) {
            CHECK(L[x] == (double)want);
            continue;
        }
        const double big = std::fabs(L[x]) > mag ? std::fabs(L[x]) : mag;
        const double cap = Kc * (6.25 * std::ldexp(1.0, -52) + ulp(big) + std::exp(-38.0));
        const double err = (double)fabsl((long double)L[x] - want);
        CHECK(err <= cap);
        if (err / cap > g_worst) g_worst = err / cap;
    }
    for (int k = 0; k < 50; ++k) {  // any predecessor set, candidates or not
        const uint64_t U = rnd() & ((1ull << n) - 1);
        CHECK(ot_index(C, U) < (uint32_t)ot_slots(Kc) && ot_expand(C, ot_index(C, U)) == (U & C));
    }
}

}  // namespace

int main() {
    // the round itself: symmetric, -inf is the neutral element, the cut at 38 nats
    CHECK(ost_round(-INFINITY, -INFINITY) == -INFINITY && ost_round(-3.5, -INFINITY) == -3.5 && ost_round(-INFINITY, -3.5) == -3.5);
    CHECK(ost_round(1.0, 40.0) == 40.0 && ost_round(40.0, 1.0) == 40.0 && ost_round(2.0, 1.0) == ost_round(1.0, 2.0));
    for (int n : {5, 33, 63})
        for (int K = 0; K <= 9 && K < n; ++K)
            for (int count : {0, 1, 7, 200})
                for (int empty_set = 0; empty_set < 2; ++empty_set)
                    for (float spread : {0.25f, 2.0f}) check_build(n, K, count, empty_set != 0, spread);
    std::printf("order_sumtables_check ok: %ld checks, the largest error %.3f of its cap\n", g_checks, g_worst);
    return 0;
}
