// order_tables_check -- the arithmetic of the order search's candidate-set
// tables (csrc/order_tables_dev.h) on the host.
//   1. ranks and indices: ot_rank counts the candidates below, ot_index and
//      ot_expand invert each other on the subsets of C, a non-candidate adds
//      nothing, ot_bit is the index's change when a variable joins, with
//      candidates above bit 31;
//   2. the build: on random lists -- tied scores, variables without the empty
//      set, empty lists, a list of the empty set alone -- every slot of the
//      serial scatter and butterfly is os_best_serial on the expanded subset,
//      and idx_v(U) finds b_v(U) and its least index for any U.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/order_tables_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                                 \
    do {                                                                                            \
        ++g_checks;                                                                                 \
        if (!(cond)) {                                                                              \
            std::fprintf(stderr, "order_tables_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                           \
        }                                                                                           \
    } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void check_indices() {
    const uint64_t C = (1ull << 3) | (1ull << 31) | (1ull << 32) | (1ull << 40) | (1ull << 62);
    CHECK(ot_popcount(C) == 5 && ot_rank(C, 3) == 0 && ot_rank(C, 31) == 1 && ot_rank(C, 32) == 2 && ot_rank(C, 62) == 4);
    CHECK(ot_rank(C, 0) == 0 && ot_rank(C, 33) == 3);
    CHECK(ot_bit(C, 40) == 8u && ot_bit(C, 62) == 16u && ot_bit(C, 5) == 0u && ot_bit(0, 7) == 0u);
    CHECK(ot_index(C, 0) == 0u && ot_index(C, ~0ull) == 31u && ot_index(0, ~0ull) == 0u && ot_expand(0, 0) == 0ull);
    for (uint32_t x = 0; x < 32; ++x) {
        const uint64_t U = ot_expand(C, x);
        CHECK(!(U & ~C) && ot_popcount(U) == ot_popcount(x) && ot_index(C, U) == x);
        CHECK(ot_index(C, U | (rnd() & ~C)) == x);  // what is no candidate adds nothing
        for (int u = 0; u < 63; ++u)
            if (!((U >> u) & 1ull)) CHECK(ot_index(C, U | (1ull << u)) == x + ot_bit(C, u));
    }
}

// One variable's list: `count` random sets inside a random pool of K candidates of n variables
void check_build(int n, int K, int count, bool empty_set) {
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
    for (size_t i = 0; i < sets.size(); ++i) scores.push_back(-(float)(rnd() % 16) * 0.5f);  // a coarse grid: ties
    const int64_t e = (int64_t)sets.size();
    const uint64_t C = ot_candidates(sets.data(), 0, e);
    CHECK(!(C & ~pool));
    const int Kc = ot_popcount(C);
    std::vector<uint64_t> T((size_t)ot_slots(Kc) + 1, 0xABABABABABABABABull);  // a guard slot behind the table
    ot_build_serial(sets.data(), scores.data(), 0, e, C, T.data());
    CHECK(T.back() == 0xABABABABABABABABull);
    CHECK((T[0] != 0) == (e > 0 && empty_set));
    for (int64_t x = 0; x < ot_slots(Kc); ++x)
        CHECK(T[x] == os_best_serial(sets.data(), scores.data(), 0, e, ot_expand(C, (uint32_t)x)));
    for (int k = 0; k < 50; ++k) {  // any predecessor set, candidates or not
        const uint64_t U = rnd() & ((1ull << n) - 1);
        const OsBest got = os_decode(T[ot_index(C, U)]), want = os_decode(os_best_serial(sets.data(), scores.data(), 0, e, U));
        CHECK(got.b == want.b && got.ent == want.ent);
    }
}

}  // namespace

int main() {
    check_indices();
    for (int n : {5, 33, 63})
        for (int K = 0; K <= 9 && K < n; ++K)
            for (int count : {0, 1, 7, 200})
                for (int empty_set = 0; empty_set < 2; ++empty_set) check_build(n, K, count, empty_set != 0);
    CHECK(ot_slots(kTableMaxK) == 67108864 && ot_slots(kTableLdsK) * 8 == 65536);
    std::printf("order_tables_check ok: %ld checks\n", g_checks);
    return 0;
}
