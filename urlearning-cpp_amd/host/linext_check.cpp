// linext_check -- the host side of csrc/linext_dev.h, the arithmetic of
// ulg_dag_linear_extensions: the two-word add across the carry, the term test,
// the (layer, colex rank) table index with the rank of S \ v, the unranking, and the recursion itself
// (lx_count_host) on DAGs worked by hand.  The same definitions run in the
// kernels of csrc/linext.hip.
// Built with AddressSanitizer + UBSan by `make sanitize` (tests/test_linext_ref.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/linext_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                           \
    do {                                                                                      \
        ++g_checks;                                                                           \
        if (!(cond)) {                                                                        \
            std::fprintf(stderr, "linext_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                     \
        }                                                                                     \
    } while (0)

constexpr uint64_t kMax = ~0ull;

bool eq(LxCount a, uint64_t lo, uint64_t hi) { return a.lo == lo && a.hi == hi; }

}  // namespace

int main() {
    static_assert(sizeof(LxCount) == 16 && alignof(LxCount) == 16, "one 16-byte vector access");
    // ---- the add
    CHECK(eq(lx_add({0, 0}, {0, 0}), 0, 0));
    CHECK(eq(lx_add({kMax, 0}, {1, 0}), 0, 1));  // 2^64 - 1 + 1
    CHECK(eq(lx_add({1, 0}, {kMax, 0}), 0, 1));
    CHECK(eq(lx_add({kMax, 0}, {kMax, 0}), kMax - 1, 1));
    CHECK(eq(lx_add({kMax, kMax}, {1, 0}), 0, 0));  // both words at maximum: wraps mod 2^128
    CHECK(eq(lx_add({kMax, kMax}, {kMax, kMax}), kMax - 1, kMax));
    CHECK(eq(lx_add({5, 7}, {6, 8}), 11, 15));  // no carry
    CHECK(eq(lx_add({1ull << 63, 3}, {1ull << 63, 4}), 0, 8));
    CHECK(eq(lx_add({kMax, 2}, {0, 3}), kMax, 5));
    // ---- 21! = 2 * 2^64 + 14197454024290336768, as 21 additions of 20!
    {
        const LxCount f20{2432902008176640000ull, 0};
        LxCount a{0, 0};
        for (int i = 0; i < 21; ++i) a = lx_add(a, f20);
        CHECK(eq(a, 14197454024290336768ull, 2));
    }
    // ---- the term test
    CHECK(lx_term(0b0111u, 2, 0b0011u));   // both parents inside
    CHECK(!lx_term(0b0101u, 2, 0b0011u));  // parent 1 outside
    CHECK(!lx_term(0b0011u, 2, 0u));       // v itself outside
    CHECK(lx_term(0b0100u, 2, 0u));        // a root
    CHECK(lx_term(1u << 27, 27, 0u) && !lx_term(1u << 27, 27, 1u));
    CHECK(lx_term(0xFFFFFFFu, 0, 0xFFFFFFEu));
    // ---- the index: past 2^32 entries, and 2^32 bytes at one DAG of n = 28
    CHECK(lx_index(0, 28, 0xFFFFFFFu, 0) == 0xFFFFFFFull);
    CHECK(lx_index(1, 28, 0, 0) * sizeof(LxCount) == 1ull << 32);
    CHECK(lx_index(17, 28, 3, 2) == (17ull << 28) + 5);
    CHECK(lx_index(70000, 16, 65000, 535) == 70000ull * 65536 + 65535);
    // ---- the binomials, the layers' offsets
    std::vector<uint32_t> bn(kLxBinomSize);
    lx_binom_fill(bn.data());
    CHECK(bn[27 * kLxBinomStride + 13] == 20058300u && bn[6 * kLxBinomStride + 3] == 20u && bn[0] == 1u);
    CHECK(bn[5 * kLxBinomStride + 6] == 0u && bn[27 * kLxBinomStride + 28] == 0u && bn[27 * kLxBinomStride + 27] == 1u);
    for (int n = 1; n <= kLinextMaxVars; ++n) {
        uint32_t off[kLinextMaxVars + 2];
        lx_layer_offsets(n, off);
        CHECK(off[0] == 0 && off[1] == 1 && off[n] == (1u << n) - 1u && off[n + 1] == 1u << n);
        for (int l = 0; l < n; ++l)  // C(n, l) = C(n-1, l-1) + C(n-1, l) out of the table
            CHECK(off[l + 1] - off[l] == (l ? bn[(n - 1) * kLxBinomStride + l - 1] : 0u) + bn[(n - 1) * kLxBinomStride + l]);
    }
    // ---- the unranking: within a layer the colex ranks ascend with the subset's number; and the
    // rank of S \ v out of the walk from the largest member down
    for (int n = 1; n <= 10; ++n) {
        std::vector<uint32_t> rank_of(1u << n, 0);
        for (int l = 0; l <= n; ++l) {
            uint32_t r = 0;
            for (uint32_t S = 0; S < (1u << n); ++S)
                if (__builtin_popcount(S) == l) {
                    CHECK(lx_unrank(bn.data(), n, l, r) == S);
                    rank_of[S] = r++;
                }
            CHECK(r == (l ? bn[(n - 1) * kLxBinomStride + l - 1] : 0u) + (l < n ? bn[(n - 1) * kLxBinomStride + l] : 0u));
        }
        for (uint32_t S = 1; S < (1u << n); ++S) {
            LxWalk w;
            for (int v = n - 1; v >= 0; --v) {
                const uint32_t got = lx_walk_step(w, bn.data(), S, rank_of[S], v);
                if ((S >> v) & 1u) CHECK(got == rank_of[S ^ (1u << v)]);
            }
        }
    }
    CHECK(lx_unrank(bn.data(), 28, 28, 0) == 0xFFFFFFFu);
    CHECK(lx_unrank(bn.data(), 28, 1, 27) == 1u << 27);
    CHECK(lx_unrank(bn.data(), 28, 14, 40116600u - 1u) == 0xFFFC000u);
    {
        LxWalk w;  // V of n = 28: every V \ v has rank 27 - v in layer 27
        for (int v = 27; v >= 0; --v) CHECK(lx_walk_step(w, bn.data(), 0xFFFFFFFu, 0, v) == (uint32_t)(27 - v));
    }
    // ---- the recursion
    {
        // 0 -> 2 <- 1: the orders 0 1 2 and 1 0 2
        const uint32_t par[3] = {0, 0, 0b011};
        std::vector<LxCount> t;
        CHECK(eq(lx_count_host(3, par, &t), 2, 0));
        // layers: {} | {0} {1} {2} | {0,1} {0,2} {1,2} | V;  {2}, {0,2}, {1,2} are not closed under parents
        const uint64_t want[8] = {1, 1, 1, 0, 2, 0, 0, 2};
        CHECK(t.size() == 8);
        for (uint32_t i = 0; i < 8; ++i) CHECK(eq(t[i], want[i], 0));
    }
    {
        // 0 -> 2 <- 1, 2 -> 3, 2 -> 4: (0, 1 in either order) 2 (3, 4 in either order)
        const uint32_t par[5] = {0, 0, 0b00011, 0b00100, 0b00100};
        CHECK(eq(lx_count_host(5, par), 4, 0));
        // the chains 0 -> 1 -> 2 and 3 -> 4 interleave in C(5, 3) ways
        const uint32_t chains[5] = {0, 0b00001, 0b00010, 0, 0b01000};
        CHECK(eq(lx_count_host(5, chains), 10, 0));
        // the diamond 0 -> 1, 0 -> 2, 1 -> 3, 2 -> 3 with the tail 3 -> 4
        const uint32_t diamond[5] = {0, 0b00001, 0b00001, 0b00110, 0b01000};
        CHECK(eq(lx_count_host(5, diamond), 2, 0));
        // a cycle 1 -> 2 -> 3 -> 1 counts 0
        const uint32_t cyc[5] = {0, 0b01000, 0b00010, 0b00100, 0};
        CHECK(eq(lx_count_host(5, cyc), 0, 0));
    }
    {
        const uint32_t two[2] = {0b10, 0b01};  // the 2-cycle
        CHECK(eq(lx_count_host(2, two), 0, 0));
        const uint32_t one[1] = {0};
        CHECK(eq(lx_count_host(1, one), 1, 0));
    }
    {
        // the empty graph: n!, whose carry reaches the high word at n = 21
        const std::vector<uint32_t> none(21, 0);
        CHECK(eq(lx_count_host(20, none.data()), 2432902008176640000ull, 0));
        CHECK(eq(lx_count_host(21, none.data()), 14197454024290336768ull, 2));
    }
    std::printf("linext_check ok: %ld checks\n", g_checks);
    return 0;
}
