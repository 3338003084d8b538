// order_mc3_check -- the arithmetic of the tempered ladders
// (csrc/order_mcmc_dev.h, "tempered ladders") on the host.
//   1. the tempered accept: beta = 1 is mcmc_accept to the bit over a grid of
//      deltas and draws (R = 1 reduces to the chains' rule); -inf and NaN are
//      refused and delta >= 0 accepted at every beta; a smaller beta never
//      turns an acceptance into a refusal; either side of the threshold;
//   2. a round's pairs: r = x (mod 2), r + 1 < R, disjoint, none for R = 1, and
//      two rounds in a row cover every pair;
//   3. the exchange: d's sign, its antisymmetry in the sums, d >= 0 always
//      accepted, d < 0 by the weight's floor at both ends of U, and the
//      product rounded once (not fused with anything).
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../csrc/order_mcmc_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        ++g_checks;                                                                               \
        if (!(cond)) {                                                                            \
            std::fprintf(stderr, "order_mc3_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                         \
        }                                                                                         \
    } while (0)

const double kInf = std::numeric_limits<double>::infinity();

void check_accept() {
    const double deltas[] = {-kInf, -800.0, -36.5, -3.25, -1.0, -0x1p-30, -0x1p-60, 0.0, 0x1p-60, 2.5, kInf};
    const double betas[] = {1.0, 0.75, 0.3, 0.1, 0x1p-40};
    const uint64_t us[] = {0ull, 1ull << 12, 0x0123456789abcdefull, 0x8000000000000000ull, ~0ull};
    for (double delta : deltas)
        for (uint64_t u : us) {
            CHECK(mc3_accept(1.0, delta, u) == mcmc_accept(delta, u));  // R = 1: the chains' rule
            bool before = false;
            for (double beta : betas) {  // descending: the hotter rung accepts whatever the colder one does
                const bool now = mc3_accept(beta, delta, u);
                CHECK(!before || now);
                CHECK(delta >= 0.0 ? now : true);
                CHECK(delta > -kInf || !now);
                before = now;
            }
        }
    CHECK(!mc3_accept(0.5, std::nan(""), 0));
    // either side of the threshold: beta delta = -ln 2 exactly representable as a product?  use the weight itself
    const double beta = 0.25, delta = -6.0;
    const uint64_t q = post_weight_q(beta * delta);
    CHECK(q > 0 && q < (1ull << 52));
    CHECK(mc3_accept(beta, delta, (q - 1) << 12));
    CHECK(mc3_accept(beta, delta, ((q - 1) << 12) | 0xfffull));  // the low 12 bits do not count
    CHECK(!mc3_accept(beta, delta, q << 12));
    CHECK(q == post_weight_q(-1.5));  // one product, then the chains' weight
}

void check_pairs() {
    for (int R = 1; R <= kMc3MaxRungs; ++R)
        for (int64_t x : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)7, (int64_t)1 << 40, ((int64_t)1 << 40) + 1}) {
            int count = 0;
            for (int r = 0; r < R; ++r) {
                const bool on = mc3_pair_considered(x, r, R);
                CHECK(on == (r + 1 < R && (r % 2) == (int)(x % 2)));
                if (on) {
                    ++count;
                    CHECK(!mc3_pair_considered(x, r + 1, R));  // disjoint
                    CHECK(!mc3_pair_considered(x + 1, r, R));
                } else if (r + 1 < R) {
                    CHECK(mc3_pair_considered(x + 1, r, R));  // the next round takes it
                }
            }
            CHECK(count == (x % 2 == 0 ? R / 2 : (R - 1) / 2));
        }
    CHECK(!mc3_pair_considered(0, 0, 1));
}

void check_swap() {
    // the hotter rung holds the better order: d > 0, always exchanged
    CHECK(mc3_swap_d(1.0, 0.3, -10.0, -4.0) > 0.0);
    CHECK(mc3_swap_accept(mc3_swap_d(1.0, 0.3, -10.0, -4.0), ~0ull));
    CHECK(mc3_swap_d(1.0, 0.3, -4.0, -10.0) == -mc3_swap_d(1.0, 0.3, -10.0, -4.0));
    CHECK(mc3_swap_d(1.0, 0.3, -7.0, -7.0) == 0.0 && mc3_swap_accept(0.0, ~0ull));
    const double d = mc3_swap_d(1.0, 0.5, -4.0, -10.0);  // 0.5 x -6
    CHECK(d == -3.0);
    const uint64_t q = post_weight_q(-3.0);
    CHECK(mc3_swap_accept(d, (q - 1) << 12) && !mc3_swap_accept(d, q << 12));
    CHECK(mc3_swap_accept(d, 0) && !mc3_swap_accept(d, ~0ull));
    // each operation rounds on its own: the differences first
    const double br = 1.0, bn = 0.1, sr = -1234.56789, sn = -1230.000001;
    const volatile double db = br - bn, ds = sn - sr;
    CHECK(mc3_swap_d(br, bn, sr, sn) == db * ds);
    CHECK(kMc3SwapDomain > (uint32_t)kMcmcMaxVars);  // 1 + p <= 63
}

}  // namespace

int main() {
    check_accept();
    check_pairs();
    check_swap();
    std::printf("order_mc3_check: %ld checks passed\n", g_checks);
    return 0;
}
