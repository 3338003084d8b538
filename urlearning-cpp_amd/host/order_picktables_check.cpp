// order_picktables_check -- the arithmetic of a record's DAG drawn from the
// order MCMC's tables (csrc/order_picktables_dev.h) on the host: on random
// lists -- tied scores, variables without the empty set, K on both sides of
// every chunk count up to 3 -- the serial build with snapshots and the serial
// descent:
//   L equals ost_build_serial's table bit for bit, E maps every stored set's
//   slot to its entry and nothing else;
//   S_c[y] is within the slot cap of the long-double sum over the stored sets
//   whose index bits >= 6 c equal y's and whose lower bits lie inside y's,
//   -inf exactly where there is none;
//   a pick returns a stored set inside the predecessors, is a function of its
//   arguments, and over every compatible set the product of the levels'
//   conditionals q / T is p = w(P) / A(U) within p 2 sum_c cap_c + sum_c 128 / T_c,
//   cap_c the cap of a slot made in 6 c rounds (tests/order_picktables_ref.py
//   derives it with 64 / T_c; the host's exp adds a unit per lane).
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/order_picktables_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;
double g_worst = 0.0;  // the largest law error as a fraction of its bound

#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        ++g_checks;                                                                                     \
        if (!(cond)) {                                                                                  \
            std::fprintf(stderr, "order_picktables_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                               \
        }                                                                                               \
    } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

double ulp(double x) { return std::nextafter(std::fabs(x), INFINITY) - std::fabs(x); }

struct Var {
    std::vector<uint64_t> sets;
    std::vector<float> scores;
    uint64_t C;
    int K;
    std::vector<double> L, S;
    std::vector<int32_t> E;
};

// cap_c of a slot of S_c: made in 6 c rounds (tests/order_picktables_ref.py); big = the largest magnitude
// among the variable's scores and the value, at least that of anything on the slot's way
double stage_cap(const Var &v, int c, double value) {
    double big = std::fabs(value);
    for (float s : v.scores) big = std::fmax(big, std::fabs((double)s));
    return std::min(kPickBits * c, v.K) * (6.25 * std::ldexp(1.0, -52) + ulp(big) / 2 + std::exp(-38.0));
}

// ln of the summed weights of the sets whose index agrees with y above bit `from` and lies inside y below it
long double direct(const Var &v, uint32_t y, int from, int *inside) {
    const uint32_t low = from >= 32 ? ~0u : (1u << from) - 1u;
    long double m = -INFINITY, sum = 0;
    *inside = 0;
    for (size_t i = 0; i < v.sets.size(); ++i) {
        const uint32_t x = ot_index(v.C, v.sets[i]);
        if ((x & ~low) != (y & ~low) || (x & low & ~y)) continue;
        ++*inside;
        if ((long double)v.scores[i] > m) m = v.scores[i];
    }
    if (!*inside) return -INFINITY;
    for (size_t i = 0; i < v.sets.size(); ++i) {
        const uint32_t x = ot_index(v.C, v.sets[i]);
        if ((x & ~low) != (y & ~low) || (x & low & ~y)) continue;
        sum += expl((long double)v.scores[i] - m);
    }
    return m + logl(sum);
}

Var make(int n, int K, int count, bool empty_set) {
    Var v;
    uint64_t pool = 0;
    while (ot_popcount(pool) < K) pool |= 1ull << (rnd() % n);
    if (empty_set) v.sets.push_back(0);
    for (int u = 0; u < 64; ++u)
        if ((pool >> u) & 1) v.sets.push_back(1ull << u);  // every candidate a single parent: K_v = K
    for (int k = 0; k < count; ++k) {
        const uint64_t P = ot_expand(pool, (uint32_t)(rnd() & rnd() & ((1ull << K) - 1)));
        bool dup = false;
        for (uint64_t Q : v.sets) dup = dup || Q == P;
        if (!dup) v.sets.push_back(P);
    }
    for (size_t i = 0; i < v.sets.size(); ++i) v.scores.push_back(-(float)(rnd() % 48) * 0.25f);
    v.C = ot_candidates(v.sets.data(), 0, (int64_t)v.sets.size());
    v.K = ot_popcount(v.C);
    const size_t slots = (size_t)ot_slots(v.K), nst = (size_t)opt_chunks(v.K) - 1;
    v.L.assign(slots + 1, 12345.0), v.S.assign(nst * slots + 1, 12345.0), v.E.assign(slots + 1, 777);  // a guard slot behind each
    opt_build_serial(v.sets.data(), v.scores.data(), 0, (int64_t)v.sets.size(), v.C, v.L.data(), v.S.data(), v.E.data());
    CHECK(v.L.back() == 12345.0 && v.S.back() == 12345.0 && v.E.back() == 777);
    return v;
}

void check_tables(const Var &v) {
    const int64_t slots = ot_slots(v.K);
    std::vector<double> plain((size_t)slots);
    ost_build_serial(v.sets.data(), v.scores.data(), 0, (int64_t)v.sets.size(), v.C, plain.data());
    std::vector<int> seen(v.sets.size(), 0);
    for (int64_t x = 0; x < slots; ++x) {
        CHECK(std::memcmp(&plain[x], &v.L[x], 8) == 0);
        if (v.E[x] >= 0) {
            CHECK((size_t)v.E[x] < v.sets.size() && ot_index(v.C, v.sets[v.E[x]]) == (uint32_t)x);
            ++seen[v.E[x]];
        } else {
            CHECK(v.E[x] == -1);
        }
    }
    for (int k : seen) CHECK(k == 1);
    for (int c = 1; c < opt_chunks(v.K); ++c)
        for (int64_t y = 0; y < slots; ++y) {
            int inside;
            const long double want = direct(v, (uint32_t)y, kPickBits * c, &inside);
            const double got = v.S[(size_t)((c - 1) * slots + y)];
            if (!inside) {
                CHECK(got == -INFINITY);
                continue;
            }
            CHECK((double)fabsl((long double)got - want) <= stage_cap(v, c, got));
        }
}

// every compatible set's probability as the product of the levels' conditionals, against w(P) / A(U)
void check_law(const Var &v, uint32_t x) {
    const double a = v.L[x];
    if (!(a > -INFINITY)) return;
    const int nch = opt_chunks(v.K);
    // level c's ratio is off by twice cap_c, relative (stage_cap's magnitude covers every lane's); the floors (and the
    // host's exp, a unit per lane more) by 2 x 64 / T_c, absolute
    double rel = 0.0;
    for (int c = 1; c < nch; ++c) rel += 2.0 * stage_cap(v, c, a);
    int inside;
    const long double A = direct(v, x, v.K, &inside);
    for (size_t i = 0; i < v.sets.size(); ++i) {
        const uint32_t px = ot_index(v.C, v.sets[i]);
        if (px & ~x) continue;
        long double prob = 1;
        double floors = 0.0;
        uint32_t fixed = 0;
        double a_cur = a;
        for (int c = nch - 1; c >= 0; --c) {
            uint64_t T = 0, mine = 0;
            double next = 0;
            for (int l = 0; l < kPickLanes; ++l) {
                if (!opt_lane_on(v.K, x, c, l)) continue;
                const double val = opt_value(v.S.data(), v.E.data(), v.scores.data(), v.K, c, opt_slot(fixed, x, c, l));
                const uint64_t q = post_weight_q(val - a_cur);
                T += q;
                if ((uint32_t)l == ((px >> (kPickBits * c)) & 63u)) mine = q, next = val;
            }
            CHECK(T > 0);
            prob *= (long double)mine / (long double)T;
            floors += 128.0 / (double)T;
            fixed |= px & (63u << (kPickBits * c));
            a_cur = next;
        }
        const long double want = expl((long double)v.scores[i] - A);
        const double err = (double)fabsl(prob - want), bound = (double)want * rel + floors;
        CHECK(err <= bound);
        if (err / bound > g_worst) g_worst = err / bound;
    }
}

void check_picks(const Var &v, uint32_t x) {
    const double a = v.L[x];
    if (!(a > -INFINITY)) return;
    for (int k = 0; k < 40; ++k) {
        const uint64_t seed = rnd(), t = 1 + rnd() % 1000;
        const uint32_t chain = (uint32_t)(rnd() % 64);
        const int p = (int)(rnd() % 63);
        const int64_t e = opt_pick_serial(v.S.data(), v.E.data(), v.scores.data(), v.K, x, a, seed, t, chain, p);
        CHECK(e >= 0 && (size_t)e < v.sets.size());
        CHECK(!(ot_index(v.C, v.sets[e]) & ~x));
        CHECK(e == opt_pick_serial(v.S.data(), v.E.data(), v.scores.data(), v.K, x, a, seed, t, chain, p));
    }
}

}  // namespace

int main() {
    CHECK(opt_chunks(0) == 1 && opt_chunks(6) == 1 && opt_chunks(7) == 2 && opt_chunks(12) == 2 && opt_chunks(13) == 3);
    CHECK(opt_chunks(19) == 4 && opt_chunks(25) == 5 && opt_chunks(kTableMaxK) == kPickMaxChunks);
    CHECK(opt_bytes(24, true) == 36.0 * 16777216.0 && opt_bytes(24, false) == 8.0 * 16777216.0);
    CHECK(opt_lane_on(7, 0x7f, 1, 1) && !opt_lane_on(7, 0x7f, 1, 2) && opt_lane_on(7, 0x7f, 0, 63) && !opt_lane_on(7, 0x3e, 0, 1));
    CHECK(opt_slot(0x1000, 0xabc, 1, 5) == (0x1000u | (5u << 6) | (0xabcu & 63u)));
    for (int n : {8, 33, 63})
        for (int K : {0, 1, 5, 6, 7, 11, 12, 13})
            for (int count : {0, 9, 150})
                for (int empty_set = 0; empty_set < 2; ++empty_set) {
                    if (K >= n) continue;
                    const Var v = make(n, K, count, empty_set != 0);
                    check_tables(v);
                    for (int k = 0; k < 6; ++k) {
                        const uint32_t x = k == 0 ? (uint32_t)(ot_slots(v.K) - 1) : (uint32_t)(rnd() % (uint64_t)ot_slots(v.K));
                        check_law(v, x);
                        check_picks(v, x);
                    }
                }
    std::printf("order_picktables_check ok: %ld checks, the largest law error %.3f of its bound\n", g_checks, g_worst);
    return 0;
}
