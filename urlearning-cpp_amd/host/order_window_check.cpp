// order_window_check -- the arithmetic of the window re-optimisation
// (csrc/order_window_dev.h) on the host.
//   1. the helpers: the width and stride a call uses, a sweep's starts, the
//      squeezed index (a bijection of the masks without bit j onto
//      0 .. 2^(w-1) - 1 that keeps the other bits' order), the LDS bytes;
//   2. the serial form of a window -- scatter, subset-max, DP, walk back -- on
//      random small lists, some variables without the empty set (-inf terms):
//      after the butterflies every table word is the image of b from the
//      lists; F(full) and whether the window is taken equal a direct
//      evaluation of all w! arrangements, w <= 6, each summed as the contract
//      sums it; the order taken is the arrangement the contract's tie rule
//      picks, its terms are b of its positions, nothing outside the window moves.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../csrc/order_window_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                                 \
    do {                                                                                            \
        ++g_checks;                                                                                 \
        if (!(cond)) {                                                                              \
            std::fprintf(stderr, "order_window_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                           \
        }                                                                                           \
    } while (0)

const double kInf = std::numeric_limits<double>::infinity();

uint64_t g_rng = 0x2545F4914F6CDD1Dull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void check_helpers() {
    CHECK(ow_width(12, 5) == 5 && ow_width(3, 5) == 3 && ow_width(5, 5) == 5);
    CHECK(ow_stride(0, 2, 2) == 1 && ow_stride(0, 3, 3) == 1 && ow_stride(0, 12, 12) == 6 && ow_stride(0, 12, 5) == 5);
    CHECK(ow_stride(7, 7, 7) == 7 && ow_stride(4, 8, 5) == 4 && ow_stride(8, 8, 5) == 5);
    std::vector<int> starts;  // n = 8, w = 3, stride 2: 0 2 4 5
    for (int a = 0;; a = ow_next_start(a, 2, 8, 3)) {
        starts.push_back(a);
        if (a == 5) break;
    }
    CHECK((starts == std::vector<int>{0, 2, 4, 5}));
    CHECK(ow_next_start(0, 5, 5, 5) == 0);
    for (int w = 1; w <= kWindowMaxWidth; ++w)
        for (int j = 0; j < w; ++j) {
            uint32_t next = 0;  // ascending masks without bit j take ascending indices, all of them
            for (uint32_t m = 0; m < (1u << w); ++m)
                if (!((m >> j) & 1u)) CHECK(ow_squeeze(m, j) == next++);
            CHECK(next == (w > 1 ? 1u << (w - 1) : 1u));
        }
    CHECK(ow_table_words(12) == 24576u && ow_lds_bytes(12) == 98304u + 32768u + 4096u && ow_lds_bytes(1) == 16u + 4u + 2u);
    CHECK(ow_beta(0) == -kInf && ow_beta(os_float_image(0x80000000u)) == 0.0 && !std::signbit(ow_beta(os_float_image(0x80000000u))));
}

struct Lists {
    int n;
    std::vector<int64_t> offsets;
    std::vector<uint64_t> sets;
    std::vector<float> scores;
    OsHostLists view() const { return OsHostLists{n, offsets.data(), sets.data(), scores.data()}; }
};

// the variables below `rooted` have no empty set
Lists random_lists(int n, int per_var, int rooted) {
    Lists L;
    L.n = n;
    L.offsets.push_back(0);
    for (int v = 0; v < n; ++v) {
        std::vector<uint64_t> mine;
        if (v >= rooted) mine.push_back(0);
        for (int k = 0; k < per_var; ++k) {
            uint64_t P = (1ull << (rnd() % n)) | (1ull << (rnd() % n)) | (rnd() % 3 ? 0 : 1ull << (rnd() % n));
            P &= ~(1ull << v);
            if (P && std::find(mine.begin(), mine.end(), P) == mine.end()) mine.push_back(P);
        }
        for (uint64_t P : mine) {
            L.sets.push_back(P);
            L.scores.push_back(-(float)(rnd() % 32) * 0.5f);  // a coarse grid: ties
        }
        L.offsets.push_back((int64_t)L.sets.size());
    }
    return L;
}

int g_taken = 0, g_left = 0, g_repaired = 0, g_ties = 0;

void check_window(const Lists &L, std::vector<uint8_t> order, int a, int w) {
    const int n = L.n;
    std::vector<double> terms(n);
    uint64_t U = 0, pre = 0;
    for (int p = 0; p < n; ++p) {
        if (p == a) pre = U;
        terms[p] = os_term_serial(L.view(), order[p], U).b;
        U |= 1ull << order[p];
    }
    const std::vector<uint8_t> was = order;
    const std::vector<double> twas = terms;
    const double present = ow_sum(twas.data() + a, w);
    std::vector<uint32_t> T(ow_table_words(w));
    std::vector<double> F((size_t)1 << w);
    std::vector<uint8_t> c((size_t)1 << w);
    const bool took = ow_window_serial(L.view(), order.data(), terms.data(), a, w, T.data(), F.data(), c.data());
    // every table word is b from the lists
    for (int j = 0; j < w; ++j)
        for (uint32_t M = 0; M < (1u << w); ++M) {
            if ((M >> j) & 1u) continue;
            uint64_t UM = pre;
            for (int i = 0; i < w; ++i)
                if ((M >> i) & 1u) UM |= 1ull << was[a + i];
            CHECK(ow_beta(T[((uint32_t)j << (w - 1)) + ow_squeeze(M, j)]) == os_term_serial(L.view(), was[a + j], UM).b);
        }
    // all arrangements, each summed ascending from +0.0
    std::vector<int> perm(w);
    for (int j = 0; j < w; ++j) perm[j] = j;
    double best = -kInf;
    int attain = 0;
    do {
        double s = 0.0;
        uint64_t UM = pre;
        for (int k = 0; k < w; ++k) {
            s = s + os_term_serial(L.view(), was[a + perm[k]], UM).b;
            UM |= 1ull << was[a + perm[k]];
        }
        if (s > best) best = s, attain = 0;
        attain += s == best;
    } while (std::next_permutation(perm.begin(), perm.end()));
    // F's adds run along the arrangement in the same order: the same bits
    CHECK(F[(1u << w) - 1u] == best || (best == -kInf && F[(1u << w) - 1u] == -kInf));
    CHECK(took == (best > present));
    g_ties += attain > 1;
    for (int p = 0; p < n; ++p)
        if (p < a || p >= a + w || !took) CHECK(order[p] == was[p] && terms[p] == twas[p]);
    if (!took) {
        ++g_left;
        return;
    }
    ++g_taken;
    g_repaired += present == -kInf;
    uint64_t seen = 0, UM = pre;
    double s = 0.0;
    for (int k = 0; k < w; ++k) {
        seen |= 1ull << order[a + k];
        CHECK(terms[a + k] == os_term_serial(L.view(), order[a + k], UM).b);
        s = s + terms[a + k];
        UM |= 1ull << order[a + k];
    }
    uint64_t want = 0;
    for (int k = 0; k < w; ++k) want |= 1ull << was[a + k];
    CHECK(seen == want && s == best);
    // a second pass over the same window finds nothing better
    CHECK(!ow_window_serial(L.view(), order.data(), terms.data(), a, w, T.data(), F.data(), c.data()));
}

}  // namespace

int main() {
    check_helpers();
    for (int n = 1; n <= 9; ++n)
        for (int rooted = 0; rooted <= 2 && rooted < n; ++rooted) {
            const Lists L = random_lists(n, 6, rooted);
            for (int trial = 0; trial < 6; ++trial) {
                std::vector<uint8_t> order(n);
                for (int p = 0; p < n; ++p) order[p] = (uint8_t)p;
                for (int p = n - 1; p > 0; --p) std::swap(order[p], order[rnd() % (p + 1)]);
                for (int w = 1; w <= 6 && w <= n; ++w)
                    for (int a = 0; a + w <= n; ++a) check_window(L, order, a, w);
            }
        }
    CHECK(g_taken > 0 && g_left > 0 && g_repaired > 0 && g_ties > 0);
    std::printf("order_window_check ok: %ld checks, %d windows taken (%d from -inf), %d left, %d with tied optima\n", g_checks, g_taken,
                g_repaired, g_left, g_ties);
    return 0;
}
