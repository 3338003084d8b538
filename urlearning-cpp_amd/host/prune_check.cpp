// prune_check -- the subset-rank arithmetic of the discrete scorer's prune pass
// (csrc/disc_prune.h for_each_subset_rank) against brute force.
//   m <= 12, every L <= m: the L-subsets of 0 .. m - 1 are listed as masks in
//   ascending order (= colex order); for every rank the visited members must be
//   the mask's bits, highest first, and each sub-rank the position of the mask
//   without that bit in the list of layer L - 1.
//   m = 62, L in {1, 2, 7, 31}: the first rank, the last and 1000 seeded ones.
//   The members must form the set whose rank -- counted with a Pascal triangle
//   built here by additions -- is the one asked for, the set of the next rank
//   must be its successor among the masks of L bits (Gosper's step), and each
//   sub-rank the counted rank of the set without that member.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../csrc/disc_prune.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "prune_check: %s:%d: %s fails (m=%d L=%d rank=%llu)\n", __FILE__, __LINE__, #cond, \
                         g_m, g_L, (unsigned long long)g_r);                               \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

int g_m = 0, g_L = 0;
uint64_t g_r = 0;

uint64_t pascal[64][64];

// masks of L bits below `mask`, counted bit by bit from the top
uint64_t counted_rank(uint64_t mask, int L) {
    uint64_t r = 0;
    int left = L;
    for (int b = 63; b >= 0 && left > 0; --b)
        if ((mask >> b) & 1ull) {
            r += pascal[b][left];  // this bit clear, `left` bits among the b below it
            --left;
        }
    return r;
}

struct Visit {
    int t, c;
    uint64_t sub;
};

std::vector<Visit> visits(const uint64_t *binom, int m, int L, uint64_t r) {
    std::vector<Visit> v;
    for_each_subset_rank(binom, m, L, r, [&](int t, int c, uint64_t sub) { v.push_back({t, c, sub}); });
    return v;
}

uint64_t mask_of(const std::vector<Visit> &v, int m) {
    uint64_t mask = 0;
    int prev = m;
    for (size_t k = 0; k < v.size(); ++k) {
        CHECK(v[k].t == (int)v.size() - 1 - (int)k);
        CHECK(v[k].c >= 0 && v[k].c < prev);  // strictly descending, inside 0 .. m - 1
        prev = v[k].c;
        mask |= 1ull << v[k].c;
    }
    return mask;
}

}  // namespace

int main() {
    std::vector<uint64_t> binom(64 * 64);
    for (int a = 0; a < 64; ++a)
        for (int b = 0; b < 64; ++b) binom[a * 64 + b] = binom64(a, b);
    for (int a = 0; a < 64; ++a)
        for (int b = 0; b < 64; ++b)
            pascal[a][b] = b == 0 ? 1 : (a == 0 ? 0 : pascal[a - 1][b - 1] + pascal[a - 1][b]);

    for (int m = 0; m <= 12; ++m) {
        std::vector<std::vector<uint64_t>> layer(m + 1);
        for (uint64_t s = 0; s < (1ull << m); ++s) layer[__builtin_popcountll(s)].push_back(s);  // ascending
        for (int L = 0; L <= m; ++L)
            for (uint64_t r = 0; r < layer[L].size(); ++r) {
                g_m = m, g_L = L, g_r = r;
                const std::vector<Visit> v = visits(binom.data(), m, L, r);
                CHECK((int)v.size() == L);
                CHECK(mask_of(v, m) == layer[L][r]);
                for (const Visit &x : v) {
                    const uint64_t sub = layer[L][r] & ~(1ull << x.c);
                    CHECK(x.sub < layer[L - 1].size() && layer[L - 1][x.sub] == sub);
                }
            }
    }

    const int m = 62;
    std::mt19937_64 rng(20261019);
    for (int L : {1, 2, 7, 31}) {
        const uint64_t count = pascal[m][L];
        CHECK(count == binom[m * 64 + L]);
        std::vector<uint64_t> ranks = {0, count - 1};
        for (int k = 0; k < 1000; ++k) ranks.push_back(rng() % count);
        for (uint64_t r : ranks) {
            g_m = m, g_L = L, g_r = r;
            const std::vector<Visit> v = visits(binom.data(), m, L, r);
            CHECK((int)v.size() == L);
            const uint64_t mask = mask_of(v, m);
            CHECK(__builtin_popcountll(mask) == L && counted_rank(mask, L) == r);
            if (r == 0) CHECK(mask == (1ull << L) - 1);
            if (r == count - 1) CHECK(mask == ((1ull << L) - 1) << (m - L));
            if (r + 1 < count) {
                const uint64_t low = mask & (~mask + 1), ripple = mask + low;
                const uint64_t next = ripple | (((mask ^ ripple) >> 2) / low);  // the next mask of L bits
                CHECK(mask_of(visits(binom.data(), m, L, r + 1), m) == next);
            }
            for (const Visit &x : v) {
                CHECK(x.sub < pascal[m][L - 1]);
                CHECK(x.sub == counted_rank(mask & ~(1ull << x.c), L - 1));
            }
        }
    }
    std::printf("prune_check ok (%ld checks)\n", g_checks);
    return 0;
}
