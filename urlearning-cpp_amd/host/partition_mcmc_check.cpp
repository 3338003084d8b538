// partition_mcmc_check -- the arithmetic of the partition MCMC
// (csrc/partition_mcmc_dev.h) on the host.
//   1. eligibility and the term: part 0 takes the empty set alone, a later
//      part needs a parent in the part just before and none outside the parts
//      before; one eligible entry gives exactly (double) s, none gives -inf,
//      4200 eligible entries at the maximum pass 2^64 and give m + log 4200;
//   2. part_masks: m of a valid row, 0 for a skipped index or one >= n;
//   3. plans: from a grid of draws on random partitions of every n = 1 .. 63,
//      a plan that is not a no-op yields (part_new_index) a valid partition of
//      m_new parts whose masks are part_new_mask's, differs from the state,
//      and follows the move's description; every operation and every no-op
//      case occurs;
//   4. ln rho: a split's plus the inverse join's is 0 to rounding, a
//      relocation's plus its inverse's is 0, a swap's is 0.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../csrc/partition_mcmc_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                                    \
    do {                                                                                               \
        ++g_checks;                                                                                    \
        if (!(cond)) {                                                                                 \
            std::fprintf(stderr, "partition_mcmc_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                              \
        }                                                                                              \
    } while (0)

const double kInf = std::numeric_limits<double>::infinity();

void check_term() {
    CHECK(part_eligible(0, 0, 0) && !part_eligible(1, 0, 0));                 // part 0
    CHECK(part_eligible(0x6, 0x7, 0x4) && !part_eligible(0x3, 0x7, 0x4));      // a parent in R
    CHECK(!part_eligible(0xC, 0x7, 0x4) && !part_eligible(0, 0x7, 0x4));       // inside A; the empty set past part 0
    CHECK(part_eligible(1ull << 62, 1ull << 62, 1ull << 62));
    const uint64_t sets[4] = {0, 0x2, 0x6, 1ull << 62};
    const float scores[4] = {-1.5f, 2e4f, -3.25f, -3.25f};
    CHECK(part_term_serial(sets, scores, 0, 4, 0, 0) == -1.5);
    CHECK(part_term_serial(sets, scores, 1, 4, 0, 0) == -kInf);  // a list without the empty set, in part 0
    CHECK(part_term_serial(sets, scores, 0, 4, 0x6, 0x4) == -3.25);
    CHECK(part_term_serial(sets, scores, 0, 4, 0x6, 0x2) == 2e4);  // -3.25 is 20003 nats below: weight 0
    CHECK(part_term_serial(sets, scores, 2, 4, (1ull << 62) | 0x6, (1ull << 62) | 0x4) == -3.25 + std::log(2.0));
    CHECK(part_term_serial(sets, scores, 0, 0, ~0ull, 1) == -kInf);
    std::vector<uint64_t> many(5000);
    std::vector<float> val(5000);
    for (int i = 0; i < 5000; ++i) {
        many[i] = 1ull | ((uint64_t)(i + 1) << 1);
        val[i] = i % 25 < 21 ? 11.0f : -900.0f;  // 4200 of them
    }
    CHECK(part_term_serial(many.data(), val.data(), 0, 5000, ~0ull >> 1, 1) == 11.0 + std::log(4200.0));
    CHECK(part_term_serial(many.data(), val.data(), 0, 5000, ~0ull >> 1, 1ull << 40) == -kInf);
}

void check_masks() {
    uint64_t mask[kMcmcMaxVars];
    const uint8_t ok[5] = {1, 0, 2, 1, 0}, skipped[5] = {0, 2, 2, 0, 0}, high[5] = {0, 1, 5, 0, 0}, flat[5] = {0, 0, 0, 0, 0};
    CHECK(part_masks(5, ok, mask) == 3 && mask[0] == 0x12 && mask[1] == 0x9 && mask[2] == 0x4);
    CHECK(part_masks(5, skipped, mask) == 0 && part_masks(5, high, mask) == 0);
    CHECK(part_masks(5, flat, mask) == 1 && mask[0] == 0x1f);
}

void check_plans() {
    bool seen_op[5] = {}, seen_noop[5] = {};
    for (int n = 1; n <= kMcmcMaxVars; ++n)
        for (uint32_t g = 0; g < 600; ++g) {
            uint32_t w[4], x[4];
            mcmc_draw(1234 + (uint64_t)n, g, 7, 3, x);
            // a random partition: every variable a part below a random bound, the used indices made dense
            uint8_t part_of[kMcmcMaxVars];
            int remap[kMcmcMaxVars];
            const int bound = 1 + (int)post_mulhi32(x[0], (uint32_t)n);
            uint64_t used = 0;
            for (int v = 0; v < n; ++v) {
                mcmc_draw(99, g, (uint32_t)v, (uint32_t)n, w);
                part_of[v] = (uint8_t)post_mulhi32(w[0], (uint32_t)bound);
                used |= 1ull << part_of[v];
            }
            for (int j = 0, next = 0; j < n; ++j) remap[j] = (used >> j) & 1ull ? next++ : -1;
            for (int v = 0; v < n; ++v) part_of[v] = (uint8_t)remap[part_of[v]];
            uint64_t mask[kMcmcMaxVars], after[kMcmcMaxVars];
            const int m = part_masks(n, part_of, mask);
            CHECK(m >= 1 && m <= n);
            mcmc_draw(5678, g, (uint32_t)n, 0, w);
            const uint64_t r = (uint64_t)x[2] | ((uint64_t)x[3] << 32);
            const PartPlan pl = part_plan(w, r, n, m, part_of, mask);
            CHECK(pl.m == m && pl.op >= 0 && pl.op <= 4);
            if (pl.noop) {
                seen_noop[pl.op] = true;
                CHECK(pl.m_new == m);
                continue;
            }
            CHECK(n >= 2);
            seen_op[pl.op] = true;
            uint8_t next[kMcmcMaxVars];
            bool moved = false;
            for (int v = 0; v < n; ++v) {
                const int q = part_new_index(pl, v, part_of[v]);
                CHECK(q >= 0 && q < pl.m_new);
                next[v] = (uint8_t)q;
                moved = moved || q != part_of[v];
            }
            CHECK(part_masks(n, next, after) == pl.m_new && pl.m_new <= n);
            for (int i = 0; i < pl.m_new; ++i) CHECK(part_new_mask(pl, i, mask) == after[i]);
            // the order of the other variables' parts is kept, whatever the move
            for (int u = 0; u < n; ++u)
                for (int z = 0; z < n; ++z) {
                    if (pl.op == kPartSwap || pl.op == kPartToPart || pl.op == kPartToGap)
                        if (u == pl.v || z == pl.v || (pl.op == kPartSwap && (u == pl.w || z == pl.w))) continue;
                    if (part_of[u] < part_of[z]) CHECK(next[u] < next[z] || (pl.op == kPartJoin && next[u] == next[z]));
                    if (part_of[u] == part_of[z]) CHECK(next[u] == next[z] || (pl.op == kPartSplit && part_of[u] == pl.a));
                }
            switch (pl.op) {
                case kPartSwap: CHECK(next[pl.v] == part_of[pl.w] && next[pl.w] == part_of[pl.v] && pl.m_new == m && moved); break;
                case kPartToPart: CHECK(after[next[pl.v]] != 1ull << pl.v && pl.m_new == m - (pl.emptied ? 1 : 0)); break;
                case kPartToGap: CHECK(after[next[pl.v]] == 1ull << pl.v && pl.m_new == m + 1 - (pl.emptied ? 1 : 0)); break;
                case kPartSplit:
                    CHECK(after[pl.a] == (mask[pl.a] & r) && after[pl.a + 1] == (mask[pl.a] & ~r) && pl.m_new == m + 1);
                    CHECK(pl.k == __builtin_popcountll(mask[pl.a]));
                    break;
                default:
                    CHECK(after[pl.a] == (mask[pl.a] | mask[pl.a + 1]) && pl.m_new == m - 1 && pl.k == __builtin_popcountll(after[pl.a]));
            }
            // a move that is not a no-op changes the state
            bool same = pl.m_new == m;
            for (int i = 0; same && i < m; ++i) same = after[i] == mask[i];
            CHECK(!same);
        }
    for (int op = 0; op < 5; ++op) CHECK(seen_op[op] && seen_noop[op]);
}

void check_rho() {
    PartPlan pl{};
    pl.op = kPartSwap;
    CHECK(part_log_rho(pl) == 0.0);
    for (int m = 1; m < 63; ++m)
        for (int k = 2; k <= 63; k += 7) {
            PartPlan sp{}, jn{};
            sp.op = kPartSplit, sp.m = m, sp.m_new = m + 1, sp.k = k;
            jn.op = kPartJoin, jn.m = m + 1, jn.m_new = m, jn.k = k;
            CHECK(std::fabs(part_log_rho(sp) + part_log_rho(jn)) < 1e-13);
            CHECK(std::fabs(part_log_rho(sp) - (k * std::log(2.0) + std::log((double)m / (m + 1)))) < 1e-13);
            PartPlan up{}, down{}, flat{};
            up.op = kPartToGap, up.m = m, up.m_new = m + 1;
            down.op = kPartToPart, down.m = m + 1, down.m_new = m;
            flat.op = kPartToPart, flat.m = flat.m_new = m;
            CHECK(std::fabs(part_log_rho(up) + part_log_rho(down)) < 1e-15 && part_log_rho(flat) == 0.0);
            CHECK(part_log_rho(up) < 0.0);
        }
}

}  // namespace

int main() {
    check_term();
    check_masks();
    check_plans();
    check_rho();
    std::printf("partition_mcmc_check ok: %ld checks\n", g_checks);
    return 0;
}
