// bdeu_check -- the fixed-point arithmetic of the BDeu score (csrc/disc_bdeu.h)
// on the host, over a grid of (N, ess, q r) that holds the corners: N = 2 and
// 2^31 - 1, ess = 1e-6 and 1e6, q r = 1 and 2^63 - 1.
//   1. bdeu_shift(N, ess) is the largest shift <= 32 at which the bound
//      U = bdeu_sum_bound(N, ess) stays below 2^62 (ldexp is exact).
//   2. The worst case of the integer sum, counted here in __int128 from a long
//      double Lm: at most 2 N terms whose counts add up to N twice, each
//      |fix(term)| <= n ceil(Lm 2^shift) + 1/2, i.e. 2 N ceil(Lm 2^shift) + N in
//      all, fits 62 bits.
//   3. Per term (cell and configuration, n from 1 to N): |fix(term)| is within
//      n ceil(Lm 2^shift) + 1 -- the lemma |term(a, n)| <= n Lm that 2. rests on
//      -- and the term fixed and un-fixed is within 2^-(shift+1) of the FP64 term.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../csrc/disc_bdeu.h"

using namespace ulg;

namespace {

long g_checks = 0;
long long g_N = 0;
double g_ess = 0;
unsigned long long g_cells = 0;
unsigned int g_n = 0;

#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        ++g_checks;                                                                                      \
        if (!(cond)) {                                                                                   \
            std::fprintf(stderr, "bdeu_check: %s:%d: %s fails (N=%lld ess=%g cells=%llu n=%u)\n", __FILE__, \
                         __LINE__, #cond, g_N, g_ess, g_cells, g_n);                                      \
            std::exit(1);                                                                                \
        }                                                                                                \
    } while (0)

typedef __int128 i128;

i128 iabs(i128 x) { return x < 0 ? -x : x; }

}  // namespace

int main() {
    const long long Ns[] = {2, 3, 64, 1000, 10000, 62000000, (1ll << 31) - 1};
    const double esses[] = {1e-6, 1e-3, 0.1, 1.0, 10.0, 1e3, 1e6};
    const unsigned long long cells_[] = {1ull, 2ull, 12ull, 16384ull, 1ull << 31, (1ull << 53) + 1ull,
                                         55000000000000000ull, (1ull << 63) - 1ull};
    const i128 two62 = (i128)1 << 62;
    CHECK(kBdeuEssMin == 1e-6 && kBdeuEssMax == 1e6);
    int lowest = 32;
    for (long long N : Ns)
        for (double ess : esses) {
            g_N = N, g_ess = ess, g_cells = 0, g_n = 0;
            const int s = bdeu_shift(N, ess);
            const double U = bdeu_sum_bound(N, ess);
            lowest = s < lowest ? s : lowest;
            // 1. the largest shift, at most 32
            CHECK(s >= 0 && s <= 32);
            CHECK(std::ldexp(U, s) < 0x1p62);
            CHECK(s == 32 || std::ldexp(U, s + 1) >= 0x1p62);
            // 2. the worst-case integer sum, from an Lm of this program's own
            const long double lm = std::fmax(-std::log(std::ldexp((long double)ess, -63)), std::log((long double)ess + (long double)N)) *
                                   (1.0L + 0x1p-60L);
            CHECK(lm > 0 && (double)lm <= bdeu_log_extreme(N, ess) * (1.0 + 0x1p-40));
            const i128 lfix = (i128)std::ceil(std::ldexp(lm, s));
            const i128 worst = (i128)2 * N * lfix + N;
            CHECK(worst < two62);
            // 3. the terms
            for (unsigned long long cells : cells_) {
                g_cells = cells;
                // a_jk = ess / cells with a_j = ess (no parents) and with a_j = a_jk (arity 1)
                for (int same = 0; same < 2; ++same) {
                    const BdeuItem b = bdeu_item(ess, same ? cells : 1ull, cells);
                    CHECK(b.a_jk >= std::ldexp(ess, -63) && b.a_jk <= ess && b.a_j >= b.a_jk && b.a_j <= ess);
                    CHECK(std::isfinite(b.lg_j) && std::isfinite(b.lg_jk));
                    const unsigned int ns[] = {1u, 2u, 3u, 7u, (unsigned)(N / 2), (unsigned)(N - 1), (unsigned)N};
                    for (unsigned int n : ns) {
                        if (n < 1) continue;
                        g_n = n;
                        const double t[2] = {bdeu_cell_term(b, n), bdeu_cfg_term(b, n)};
                        for (double x : t) {
                            CHECK(std::isfinite(x));
                            const long long f = bdeu_fix(x, s);
                            CHECK(iabs((i128)f) <= (i128)n * lfix + 1);
                            CHECK(std::fabs(bdeu_unfix(f, s) - x) <= std::ldexp(1.0, -(s + 1)));
                        }
                    }
                }
            }
        }
    // the scale does leave 2^32 on this grid, and never goes below the header's floor
    CHECK(lowest < 32 && lowest >= 23);
    CHECK(bdeu_shift(2, 1.0) == 32 && bdeu_shift(62000000, 1.0) < 32);
    std::printf("bdeu_check ok (%ld checks, lowest shift %d)\n", g_checks, lowest);
    return 0;
}
