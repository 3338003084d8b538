// posterior_sample_check -- the integer arithmetic of the posterior sampler
// (csrc/posterior_sample_dev.h) on the host.
//   1. Philox4x32-10 at three known answers (the zero and all-ones vectors of
//      the Random123 distribution's kat_vectors, and its pi-digits vector),
//      and post_draw's packing of key, counter and the two 64-bit draws;
//   2. post_weight_q at -inf (0), at 0 (2^52 exactly), at ln(1/2), at a
//      negative x so small that q is exactly 0, around the first x whose q is
//      1, and monotone over a grid;
//   3. the pick: U = 0 takes the first candidate of positive weight and
//      U = 2^64 - 1 the last, with leading, inner and trailing zero weights;
//      every U lands where the exact rational U T / 2^64 does; all-zero
//      weights give `count`; the threshold stays below T.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../csrc/posterior_sample_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        ++g_checks;                                                                                     \
        if (!(cond)) {                                                                                  \
            std::fprintf(stderr, "posterior_sample_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                               \
        }                                                                                               \
    } while (0)

const double kInf = std::numeric_limits<double>::infinity();

void check_philox() {
    uint32_t w[4];
    post_philox(0, 0, 0, 0, 0, 0, w);
    CHECK(w[0] == 0x6627e8d5u && w[1] == 0xe169c58du && w[2] == 0xbc57ac4cu && w[3] == 0x9b00dbd8u);
    post_philox(~0u, ~0u, ~0u, ~0u, ~0u, ~0u, w);
    CHECK(w[0] == 0x408f276du && w[1] == 0x41c83b0eu && w[2] == 0xa20bc7c6u && w[3] == 0x6d5451fdu);
    post_philox(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, w);
    CHECK(w[0] == 0xd16cfe09u && w[1] == 0x94fdccebu && w[2] == 0x5001e420u && w[3] == 0x24126ea1u);
    // post_draw: key = the seed's halves, counter = (k's halves, i, 0)
    const PostDraw z = post_draw(0, 0, 0);
    CHECK(z.sink == 0xe169c58d6627e8d5ull && z.set == 0x9b00dbd8bc57ac4cull);
    const uint64_t seed = 0x299f31d0a4093822ull, k = 0x85a308d3243f6a88ull;
    post_philox(0x243f6a88u, 0x85a308d3u, 7u, 0u, 0xa4093822u, 0x299f31d0u, w);
    const PostDraw d = post_draw(seed, k, 7);
    CHECK(d.sink == ((uint64_t)w[0] | ((uint64_t)w[1] << 32)) && d.set == ((uint64_t)w[2] | ((uint64_t)w[3] << 32)));
    // neighbouring counters and seeds give other words
    CHECK(post_draw(seed, k, 8).sink != d.sink && post_draw(seed, k + 1, 7).sink != d.sink && post_draw(seed + 1, k, 7).sink != d.sink);
}

void check_weight() {
    const uint64_t one = 1ull << kPostWeightBits;
    CHECK(post_weight_q(-kInf) == 0);
    CHECK(post_weight_q(0.0) == one);
    CHECK(post_weight_q(-0.0) == one);
    const uint64_t half = post_weight_q(std::log(0.5));
    CHECK(half >= one / 2 - 2 && half <= one / 2 + 2);
    CHECK(post_weight_q(-37.0) == 0);     // exp(-37) 2^52 = 0.38
    CHECK(post_weight_q(-745.0) == 0);    // a subnormal exp
    CHECK(post_weight_q(-1e4) == 0 && post_weight_q(-4e4) == 0);  // exp underflows to 0
    CHECK(post_weight_q(-36.0) == 1);     // exp(-36) 2^52 = 1.04
    CHECK(post_weight_q(-35.0) == 2);     // ... 2.84
    uint64_t prev = 0;
    for (double x = -40.0; x <= 0.0; x += 1.0 / 64) {
        const uint64_t q = post_weight_q(x);
        CHECK(q >= prev && q <= one);
        const long double want = expl((long double)x) * 4503599627370496.0L;
        CHECK((long double)q <= want + 4.0L && (long double)q + 5.0L >= want);
        prev = q;
    }
}

// the candidate the exact rational U T / 2^64 selects
int64_t pick_exact(const std::vector<uint64_t> &q, uint64_t U) {
    unsigned __int128 T = 0, C = 0;
    for (uint64_t x : q) T += x;
    const unsigned __int128 ut = (unsigned __int128)U * T;  // T < 2^64 in every case below
    for (size_t j = 0; j < q.size(); ++j) {
        C += q[j];
        if ((C << 64) > ut) return (int64_t)j;  // C > U T / 2^64  <=>  C > floor(U T / 2^64)
    }
    return (int64_t)q.size();
}

void check_pick() {
    const uint64_t kMax = ~0ull, one = 1ull << kPostWeightBits;
    CHECK(post_mulhi64(kMax, kMax) == kMax - 1 && post_mulhi64(1ull << 63, 6) == 3 && post_mulhi64(0, kMax) == 0);
    for (uint64_t T : std::initializer_list<uint64_t>{1, 2, 1000, one, one + 12345, kMax}) {
        CHECK(post_pick_threshold(0, T) == 0);
        CHECK(post_pick_threshold(kMax, T) == T - 1);
        CHECK(post_pick_threshold(1ull << 63, T) == T / 2);
    }
    const std::vector<std::vector<uint64_t>> cases = {
        {one},
        {5, 7},
        {0, 0, 5, 7},                        // leading zeros
        {5, 7, 0, 0},                        // trailing zeros
        {0, 5, 0, 0, 7, 0},                  // both, and inner ones
        {0, 1, 0},                           // one unit of weight in all
        {one / 3, 0, one / 3, one / 3, 0},
        {1, one, 1},
    };
    for (const auto &q : cases) {
        int64_t firstpos = -1, lastpos = -1;
        for (size_t j = 0; j < q.size(); ++j)
            if (q[j]) {
                if (firstpos < 0) firstpos = (int64_t)j;
                lastpos = (int64_t)j;
            }
        const int64_t cnt = (int64_t)q.size();
        CHECK(post_pick(q.data(), cnt, 0) == firstpos);
        CHECK(post_pick(q.data(), cnt, kMax) == lastpos);
        uint64_t U = 0x9e3779b97f4a7c15ull;
        for (int r = 0; r < 2000; ++r) {
            const int64_t j = post_pick(q.data(), cnt, U);
            CHECK(j >= 0 && j < cnt && q[(size_t)j] > 0);
            CHECK(j == pick_exact(q, U));
            U = U * 6364136223846793005ull + 1442695040888963407ull;
        }
    }
    // the share of draws a candidate takes: {5, 7} splits the 64-bit range at 5/12
    {
        const uint64_t q[2] = {5, 7};
        const uint64_t edge = (uint64_t)(((unsigned __int128)5 << 64) / 12);  // floor(2^64 5/12): U T / 2^64 < 5 up to here
        CHECK(post_pick(q, 2, edge) == 0 && post_pick(q, 2, edge + 1) == 1);
    }
    const uint64_t zeros[3] = {0, 0, 0};
    CHECK(post_pick(zeros, 3, 0) == 3 && post_pick(zeros, 3, kMax) == 3 && post_pick(zeros, 0, 1) == 0);
}

}  // namespace

int main() {
    check_philox();
    check_weight();
    check_pick();
    std::printf("posterior_sample_check ok (%ld checks)\n", g_checks);
    return 0;
}
