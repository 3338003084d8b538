// order_edges_check -- the arithmetic of the Rao-Blackwellised edge row
// (csrc/order_edges_dev.h) on the host, held to its definitions:
//   1. the conversion and the ratio: y is the term's own, g(T, T) = 2^40 for
//      sums below and beyond 2^64, g(0, T) = 0, halves and quarters to the bit,
//      g monotone in N and never above 2^40;
//   2. the row over small lists: N_u <= T for every u, g = 2^40 iff every
//      compatible entry (of positive weight) holds u, 0 outside U and for a
//      variable no compatible entry holds, an entry beyond 745 nats below the
//      maximum changes nothing, no compatible entry gives false and zeros;
//   3. against a direct restatement in unsigned __int128 over random lists of
//      up to 63 variables (bits above 31 and bit 62): the same N, T and g;
//   4. sums that cross 2^64 in both N and T: 8192 subsets at one score give
//      T = 2^65, N_u = 2^64 and g = 2^39 to the bit; 4200 entries at the
//      maximum of which all hold u and 4100 hold w give N_w past 2^64 too.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../csrc/order_edges_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                                 \
    do {                                                                                            \
        ++g_checks;                                                                                 \
        if (!(cond)) {                                                                              \
            std::fprintf(stderr, "order_edges_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                           \
        }                                                                                           \
    } while (0)

constexpr uint64_t kOne = 1ull << kPostWeightBits;  // the maximum's own weight
constexpr uint64_t kFull = 1ull << kEdgeBits;

typedef unsigned __int128 u128;
u128 wide(LxCount x) { return ((u128)x.hi << 64) | x.lo; }
LxCount narrow(u128 x) { return LxCount{(uint64_t)x, (uint64_t)(x >> 64)}; }

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

void check_ratio() {
    CHECK(edge_y(LxCount{kOne, 0}) == 1.0 && edge_y(LxCount{0, 1}) == 4096.0 && edge_y(LxCount{kOne, 1}) == 4097.0);
    CHECK(mcmc_term(0.0, LxCount{kOne * 3, 0}) == std::log(edge_y(LxCount{kOne * 3, 0})));  // the term's conversion
    const LxCount sums[] = {{kOne, 0}, {kOne + 1, 0}, {~0ull, 0}, {0, 1}, {1, 1}, {kOne * 5, 2}, {~0ull, 1023}};
    for (const LxCount &T : sums) {
        CHECK(edge_g(T, T) == kFull);
        CHECK(edge_g(LxCount{0, 0}, T) == 0);
        const u128 t = wide(T);
        uint64_t last = 0;
        for (int s = 0; s <= 16; ++s) {  // N = T s / 16, ascending
            const LxCount N = narrow(t / 16 * s + (s == 16 ? t % 16 : 0));
            const uint64_t g = edge_g(N, T);
            CHECK(g >= last && g <= kFull);
            last = g;
        }
    }
    // powers of two divide exactly
    CHECK(edge_g(LxCount{0, 1}, LxCount{0, 2}) == kFull / 2);
    CHECK(edge_g(LxCount{kOne, 0}, LxCount{kOne * 4, 0}) == kFull / 4);
    CHECK(edge_g(LxCount{0, 1}, LxCount{0, 4}) == kFull / 4);
    CHECK(edge_g(LxCount{kOne, 0}, LxCount{0, 1}) == kFull >> 12);  // 2^52 of 2^64
    CHECK(edge_g(LxCount{1, 0}, LxCount{0, 1}) == 0);               // 2^-64 floors to 0
    CHECK(edge_g(LxCount{kOne, 0}, LxCount{kOne * 3, 0}) == (uint64_t)std::floor(std::ldexp(1.0 / 3.0, kEdgeBits)));
}

void check_row() {
    uint64_t g[kMcmcMaxVars];
    LxCount N[kMcmcMaxVars], T;
    {
        // variable 3 of n = 5: {}, {0}, {0,1}, {2}, {4}
        const uint64_t sets[5] = {0, 1, 3, 4, 16};
        const float scores[5] = {-1.0f, -0.5f, 0.25f, 0.0f, 5.0f};
        CHECK(edge_row_serial(sets, scores, 0, 5, 0x7, 5, g, N, &T));  // U = {0,1,2}: {4} is incompatible
        for (int u = 0; u < 5; ++u) CHECK(wide(N[u]) <= wide(T));
        CHECK(T.hi == 0 && T.lo == kOne + post_weight_q(-1.25) + post_weight_q(-0.75) + post_weight_q(-0.25));
        CHECK(N[0].lo == kOne + post_weight_q(-0.75) && N[1].lo == kOne && N[2].lo == post_weight_q(-0.25));
        CHECK(g[3] == 0 && g[4] == 0 && N[4].lo == 0);  // the diagonal, and outside U
        CHECK(g[0] > g[1] && g[1] > g[2] && g[2] > 0 && g[0] < kFull);
        CHECK(g[1] == edge_g(N[1], T));
        // U = {0}: {} and {0}
        CHECK(edge_row_serial(sets, scores, 0, 5, 0x1, 5, g, N, &T));
        CHECK(T.lo == kOne + post_weight_q(-0.5) && N[0].lo == kOne && g[1] == 0 && g[2] == 0 && g[0] > kFull / 2 && g[0] < kFull);
        // U = {}: the empty set alone, every g 0
        CHECK(edge_row_serial(sets, scores, 0, 1, 0, 5, g, N, &T));
        for (int u = 0; u < 5; ++u) CHECK(g[u] == 0);
        CHECK(T.lo == kOne);
        // without the empty set and U = {}: no compatible entry
        g[0] = 77;
        CHECK(!edge_row_serial(sets, scores, 1, 5, 0, 5, g, nullptr, nullptr));
        for (int u = 0; u < 5; ++u) CHECK(g[u] == 0);
        CHECK(!edge_row_serial(sets, scores, 0, 0, ~0ull, 5, g, nullptr, nullptr));  // an empty list
    }
    {
        // every compatible entry holds 1: g = 2^40 exactly; 0 is held by some: below it
        const uint64_t sets[4] = {2, 3, 6, 8};
        const float scores[4] = {0.0f, 0.0f, -2.0f, 9.0f};
        CHECK(edge_row_serial(sets, scores, 0, 4, 0x7, 5, g, N, &T));
        CHECK(g[1] == kFull && wide(N[1]) == wide(T) && g[0] < kFull && g[0] > 0 && g[2] > 0 && g[2] < g[0]);
        // one compatible entry: 2^40 for its members, 0 for the rest
        CHECK(edge_row_serial(sets, scores, 0, 4, 0x6, 5, g, N, &T));  // {1} and {1,2}
        CHECK(g[1] == kFull && g[0] == 0);
        CHECK(edge_row_serial(sets, scores, 0, 4, 0x2, 5, g, N, &T));  // {1} alone
        CHECK(T.lo == kOne && g[1] == kFull && g[0] == 0 && g[2] == 0 && g[3] == 0);
    }
    {
        // an entry 796 nats below the maximum weighs 0: it moves neither T nor any N
        const uint64_t sets[3] = {1, 3, 0};
        const float scores[3] = {-3.25f, -800.0f, -3.25f};
        CHECK(edge_row_serial(sets, scores, 0, 3, 0x3, 3, g, N, &T));
        CHECK(T.lo == 2 * kOne && N[0].lo == kOne && N[1].lo == 0 && g[0] == kFull / 2 && g[1] == 0);
        CHECK(edge_row_serial(sets, scores, 0, 2, 0x3, 3, g, N, &T));  // every entry holds 0, one of them at weight 0
        CHECK(g[0] == kFull && g[1] == 0);
    }
    {
        // bit 62 and a variable above bit 31
        const uint64_t sets[3] = {0, 1ull << 62, (1ull << 62) | (1ull << 40)};
        const float scores[3] = {0.5f, 0.5f, 0.5f};
        CHECK(edge_row_serial(sets, scores, 0, 3, (1ull << 62) | (1ull << 40), 63, g, N, &T));
        CHECK(T.lo == 3 * kOne && N[62].lo == 2 * kOne && N[40].lo == kOne);
        CHECK(g[62] == edge_g(LxCount{2, 0}, LxCount{3, 0}) && g[40] == edge_g(LxCount{1, 0}, LxCount{3, 0}) && g[0] == 0);
        CHECK(edge_row_serial(sets, scores, 0, 3, 1ull << 62, 63, g, N, &T));
        CHECK(T.lo == 2 * kOne && g[62] == kFull / 2 && g[40] == 0);
    }
}

void check_random() {
    for (int round = 0; round < 300; ++round) {
        const int n = 2 + (int)(rnd() % 62);  // 2 .. 63
        const int v = (int)(rnd() % (uint64_t)n);
        const uint64_t all = ((1ull << n) - 1) & ~(1ull << v);
        const int len = 1 + (int)(rnd() % 300);
        std::vector<uint64_t> sets((size_t)len);
        std::vector<float> scores((size_t)len);
        for (int i = 0; i < len; ++i) {
            uint64_t S = 0;
            for (int r = (int)(rnd() % 5); r > 0; --r) S |= 1ull << (rnd() % (uint64_t)n);
            sets[(size_t)i] = S & all;
            scores[(size_t)i] = (float)((double)(rnd() % 2000) / 100.0 - 10.0) - (rnd() % 7 == 0 ? 800.0f : 0.0f);
        }
        const uint64_t U = ((rnd() | rnd()) & all) | (rnd() % 3 == 0 ? all : 0);
        uint64_t g[kMcmcMaxVars];
        LxCount N[kMcmcMaxVars], T;
        const bool ok = edge_row_serial(sets.data(), scores.data(), 0, len, U, n, g, N, &T);
        double m = -INFINITY;
        for (int i = 0; i < len; ++i)
            if (!(sets[(size_t)i] & ~U) && (double)scores[(size_t)i] > m) m = (double)scores[(size_t)i];
        CHECK(ok == (m > -INFINITY));
        if (!ok) continue;
        CHECK(mcmc_term(m, T) == mcmc_term_serial(sets.data(), scores.data(), 0, len, U));  // the term's own sum
        u128 t = 0;
        std::vector<u128> nu((size_t)n, 0);
        for (int i = 0; i < len; ++i) {
            if (sets[(size_t)i] & ~U) continue;
            const uint64_t q = post_weight_q((double)scores[(size_t)i] - m);
            t += q;
            for (int u = 0; u < n; ++u)
                if ((sets[(size_t)i] >> u) & 1ull) nu[(size_t)u] += q;
        }
        CHECK(wide(T) == t && t >= kOne);
        for (int u = 0; u < n; ++u) {
            CHECK(wide(N[u]) == nu[(size_t)u] && nu[(size_t)u] <= t);
            CHECK(g[u] == edge_g(N[u], T) && g[u] <= kFull);
            if (!((U >> u) & 1ull)) CHECK(g[u] == 0);
            CHECK((g[u] == kFull) == (nu[(size_t)u] == t));  // T < 2^61 here: the ratio of unequal sums is below 1 - 2^-52
        }
        CHECK(g[v] == 0);
    }
}

void check_carry() {
    {
        // variable 13 of n = 14 lists all 8192 subsets of the others at one score
        std::vector<uint64_t> sets(8192);
        std::vector<float> scores(8192, -2.5f);
        for (uint64_t S = 0; S < 8192; ++S) sets[S] = S;
        uint64_t g[kMcmcMaxVars];
        LxCount N[kMcmcMaxVars], T;
        CHECK(edge_row_serial(sets.data(), scores.data(), 0, 8192, 8191, 14, g, N, &T));
        CHECK(T.hi == 2 && T.lo == 0);  // 8192 x 2^52 = 2^65
        for (int u = 0; u < 13; ++u) CHECK(N[u].hi == 1 && N[u].lo == 0 && g[u] == kFull / 2);
        CHECK(g[13] == 0);
        // six predecessors: 64 compatible subsets, still a half each, below 2^64
        CHECK(edge_row_serial(sets.data(), scores.data(), 0, 8192, 0x3F, 14, g, N, &T));
        CHECK(T.hi == 0 && T.lo == 64 * kOne);
        for (int u = 0; u < 13; ++u) CHECK(g[u] == (u < 6 ? kFull / 2 : 0));
    }
    {
        // 4200 entries at the maximum: all hold 0, the first 4100 hold 1, every fifth holds 2
        const int len = 4200;
        std::vector<uint64_t> sets((size_t)len);
        std::vector<float> scores((size_t)len, 11.0f);
        for (int i = 0; i < len; ++i) sets[(size_t)i] = 1ull | (i < 4100 ? 2ull : 0ull) | (i % 5 == 0 ? 4ull : 0ull) | ((uint64_t)i << 8);
        uint64_t g[kMcmcMaxVars];
        LxCount N[kMcmcMaxVars], T;
        CHECK(edge_row_serial(sets.data(), scores.data(), 0, len, ~0ull >> 1, 63, g, N, &T));
        CHECK(T.hi == 1 && T.lo == (4200ull - 4096ull) << 52);
        CHECK(N[0].hi == 1 && N[0].lo == T.lo && g[0] == kFull);
        CHECK(N[1].hi == 1 && N[1].lo == 4ull << 52 && g[1] == (uint64_t)std::floor(std::ldexp(4100.0 / 4200.0, kEdgeBits)));
        CHECK(N[2].hi == 0 && N[2].lo == 840ull << 52 && g[2] == kFull / 5);  // 840 / 4200, the quotient rounded, then floored
        CHECK(wide(N[1]) <= wide(T) && g[1] < kFull);
    }
}

}  // namespace

int main() {
    check_ratio();
    check_row();
    check_random();
    check_carry();
    std::printf("order_edges_check ok: %ld checks\n", g_checks);
    return 0;
}
