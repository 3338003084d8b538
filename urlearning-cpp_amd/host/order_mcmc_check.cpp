// order_mcmc_check -- the arithmetic of the order MCMC (csrc/order_mcmc_dev.h)
// on the host.
//   1. the draw's counter layout, and the proposal: i != j, both in range, over
//      a grid of draws for every n = 2 .. 63, with both ends of each word;
//      every ordered pair (i, j) of a small n is reached;
//   2. the shuffle: a permutation for every n, the identity for n = 1, and the
//      swap position never beyond p;
//   3. the two-word sum: 4097 weights of 2^52 pass 2^64 and give hi = 1, a
//      carry at the word's edge, and the same words in any order;
//   4. the accept rule at delta = 0, a positive delta, -inf, NaN, and at
//      U = 0 and U = 2^64 - 1 on either side of the threshold;
//   5. the term: a single compatible entry gives exactly (double) s, none
//      gives -inf, two equal entries m + log 2, an entry beyond 745 nats below
//      the maximum changes nothing, and 4200 entries at the maximum (T past
//      2^64) give m + log 4200.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../csrc/order_mcmc_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        ++g_checks;                                                                                \
        if (!(cond)) {                                                                             \
            std::fprintf(stderr, "order_mcmc_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                          \
        }                                                                                          \
    } while (0)

const double kInf = std::numeric_limits<double>::infinity();

void check_move() {
    // the counter: (lo32(t), hi32(t), c, d) under the seed's halves
    const uint64_t seed = 0x299f31d0a4093822ull, t = 0x85a308d3243f6a88ull;
    uint32_t w[4], x[4];
    mcmc_draw(seed, t, 0x13198a2eu, 0x03707344u, w);
    CHECK(w[0] == 0xd16cfe09u && w[1] == 0x94fdccebu && w[2] == 0x5001e420u && w[3] == 0x24126ea1u);  // Random123's pi vector
    mcmc_draw(seed, t, 5, 0, w);
    mcmc_draw(seed, t, 5, 1, x);
    CHECK(w[0] != x[0]);
    mcmc_draw(seed, t + 1, 5, 0, x);
    CHECK(w[0] != x[0]);
    mcmc_draw(seed, t, 6, 0, x);
    CHECK(w[0] != x[0]);
    const uint32_t ends[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    for (int n = 2; n <= kMcmcMaxVars; ++n) {
        for (uint32_t a : ends)
            for (uint32_t b : ends) {
                const uint32_t d[4] = {a, b, 0x89abcdefu, 0x01234567u};
                const McmcMove mv = mcmc_move(d, n);
                CHECK(mv.i >= 0 && mv.i < n && mv.j >= 0 && mv.j < n && mv.i != mv.j);
                CHECK(mv.u_acc == 0x0123456789abcdefull);
            }
        for (uint32_t g = 0; g < 4096; ++g) {
            mcmc_draw(seed, g, (uint32_t)n, 0, w);
            const McmcMove mv = mcmc_move(w, n);
            CHECK(mv.i >= 0 && mv.i < n && mv.j >= 0 && mv.j < n && mv.i != mv.j);
        }
    }
    // w0 = 0 gives i = 0 and w1 = 0 then j = 1; the last words give i = n - 1, j = n - 2
    const uint32_t first[4] = {0, 0, 0, 0}, last[4] = {~0u, ~0u, 0, 0};
    CHECK(mcmc_move(first, 7).i == 0 && mcmc_move(first, 7).j == 1);
    CHECK(mcmc_move(last, 7).i == 6 && mcmc_move(last, 7).j == 5);
    // every ordered pair of n = 4 from a grid of words
    bool hit[4][4] = {};
    for (uint32_t a = 0; a < 4; ++a)
        for (uint32_t b = 0; b < 3; ++b) {
            const uint32_t d[4] = {a << 30, (uint32_t)(((uint64_t)b << 32) / 3 + 1), 0, 0};
            const McmcMove mv = mcmc_move(d, 4);
            hit[mv.i][mv.j] = true;
        }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) CHECK(hit[i][j] == (i != j));
}

void check_shuffle() {
    for (int n = 1; n <= kMcmcMaxVars; ++n)
        for (uint32_t c = 0; c < 50; ++c) {
            uint8_t order[kMcmcMaxVars + 1];
            order[n] = 0xAB;  // the guard behind the row
            mcmc_shuffle(77 + c, c, n, order);
            uint64_t seen = 0;
            for (int p = 0; p < n; ++p) {
                CHECK(order[p] < n && !((seen >> order[p]) & 1ull));
                seen |= 1ull << order[p];
            }
            CHECK(order[n] == 0xAB);
        }
    uint8_t one[1];
    mcmc_shuffle(5, 0, 1, one);
    CHECK(one[0] == 0);
    for (int p = 1; p < kMcmcMaxVars; ++p) {
        CHECK(mcmc_shuffle_pos(0u, p) == 0 && mcmc_shuffle_pos(~0u, p) == p);
    }
    // two chains of one seed differ, a chain is the same in every call
    uint8_t a[20], b[20], a2[20];
    mcmc_shuffle(9, 0, 20, a);
    mcmc_shuffle(9, 1, 20, b);
    mcmc_shuffle(9, 0, 20, a2);
    CHECK(!std::equal(a, a + 20, b) && std::equal(a, a + 20, a2));
}

void check_sum() {
    const uint64_t one = 1ull << kPostWeightBits;
    std::vector<uint64_t> q(4097, one);
    LxCount T = mcmc_sum_q(q.data(), 4096);
    CHECK(T.hi == 1 && T.lo == 0);  // 4096 x 2^52 = 2^64
    T = mcmc_sum_q(q.data(), 4095);
    CHECK(T.hi == 0 && T.lo == 0ull - one);
    T = mcmc_sum_q(q.data(), 4097);
    CHECK(T.hi == 1 && T.lo == one);
    std::vector<uint64_t> r = {~0ull, 1ull, ~0ull, 2ull, 12345ull};
    T = mcmc_sum_q(r.data(), (int64_t)r.size());
    CHECK(T.hi == 2 && T.lo == 12345ull + 1ull);  // 2 (2^64 - 1) + 3 + 12345
    std::reverse(r.begin(), r.end());
    const LxCount R = mcmc_sum_q(r.data(), (int64_t)r.size());
    CHECK(R.hi == T.hi && R.lo == T.lo);
    CHECK(mcmc_sum_q(r.data(), 0).lo == 0 && mcmc_sum_q(r.data(), 0).hi == 0);
}

void check_accept() {
    const uint64_t all = ~0ull;
    CHECK(mcmc_accept(0.0, 0) && mcmc_accept(0.0, all) && mcmc_accept(-0.0, all));
    CHECK(mcmc_accept(3.5, all) && mcmc_accept(1e300, all) && mcmc_accept(kInf, all));
    CHECK(!mcmc_accept(-kInf, 0) && !mcmc_accept(-kInf, all));
    CHECK(!mcmc_accept(std::nan(""), 0));
    // delta = ln(1/2): the threshold is about 2^51 of the 52 bits U >> 12
    const double half = std::log(0.5);
    const uint64_t q = post_weight_q(half);
    CHECK(mcmc_accept(half, 0) && !mcmc_accept(half, all));
    CHECK(mcmc_accept(half, (q - 1) << 12) && mcmc_accept(half, ((q - 1) << 12) | 0xfff));
    CHECK(!mcmc_accept(half, q << 12) && !mcmc_accept(half, (q << 12) | 0xfff));
    // a delta whose weight floors to 0 is never accepted, not even at U = 0
    CHECK(post_weight_q(-40.0) == 0 && !mcmc_accept(-40.0, 0) && !mcmc_accept(-1e4, 0));
    // just below 0: all but the last few of the 2^52 values accept
    CHECK(mcmc_accept(-1e-15, 0) && mcmc_accept(-1e-15, (all >> 12) << 11) && !mcmc_accept(-1e-3, all));
}

void check_term() {
    const double ln2 = std::log(2.0);
    // one compatible entry: its score to the bit, whatever its size
    for (float s : {0.0f, -1.5f, 2e4f, -2e4f, 1e-30f, -3.3e38f}) {
        const uint64_t sets[3] = {0x5ull, 0x2ull, 1ull << 62};
        const float scores[3] = {7.0f, s, 9.0f};
        CHECK(mcmc_term_serial(sets, scores, 0, 3, 0x2ull) == (double)s);
        CHECK(mcmc_term_serial(sets, scores, 1, 2, ~0ull) == (double)s);
    }
    {
        const uint64_t sets[2] = {0x1ull, 0x4ull};
        const float scores[2] = {1.0f, 2.0f};
        CHECK(mcmc_term_serial(sets, scores, 0, 2, 0x2ull) == -kInf);  // none compatible
        CHECK(mcmc_term_serial(sets, scores, 0, 0, ~0ull) == -kInf);   // an empty list
        CHECK(mcmc_term_serial(sets, scores, 0, 2, 1ull << 62) == -kInf);
    }
    {
        const uint64_t sets[3] = {0, 1, 2};
        const float scores[3] = {-3.25f, -3.25f, -800.0f};
        CHECK(mcmc_term_serial(sets, scores, 0, 2, 1) == -3.25 + ln2);
        CHECK(mcmc_term_serial(sets, scores, 0, 3, 3) == -3.25 + ln2);  // 796 nats below: weight 0
        CHECK(mcmc_term_serial(sets, scores, 2, 3, 3) == -800.0);       // alone it is the maximum
    }
    {
        // the empty set and the set of bit 62, a variable above bit 31
        const uint64_t sets[2] = {0, 1ull << 62};
        const float scores[2] = {0.5f, 0.5f};
        CHECK(mcmc_term_serial(sets, scores, 0, 2, 0) == 0.5);
        CHECK(mcmc_term_serial(sets, scores, 0, 2, 1ull << 62) == 0.5 + ln2);
        CHECK(mcmc_term_serial(sets, scores, 0, 2, (1ull << 62) - 1) == 0.5);
    }
    {
        // 5000 entries, 4200 at the maximum: T = 4200 x 2^52 + the rest passes 2^64
        std::vector<uint64_t> sets(5000);
        std::vector<float> scores(5000);
        for (int i = 0; i < 5000; ++i) {
            sets[i] = (uint64_t)i;
            scores[i] = i % 25 < 21 ? 11.0f : -900.0f;  // 4200 of them
        }
        std::vector<uint64_t> q;
        for (int i = 0; i < 5000; ++i) q.push_back(post_weight_q((double)scores[i] - 11.0));
        const LxCount T = mcmc_sum_q(q.data(), 5000);
        CHECK(T.hi == 1 && T.lo == (4200ull - 4096ull) << 52);
        const double a = mcmc_term_serial(sets.data(), scores.data(), 0, 5000, ~0ull);
        CHECK(a == 11.0 + std::log(4200.0));
        CHECK(mcmc_term(11.0, T) == a);
    }
    CHECK(mcmc_term(-7.0, LxCount{1ull << 52, 0}) == -7.0);
}

}  // namespace

int main() {
    check_move();
    check_shuffle();
    check_sum();
    check_accept();
    check_term();
    std::printf("order_mcmc_check ok: %ld checks\n", g_checks);
    return 0;
}
