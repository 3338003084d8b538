// fnml_check -- the arithmetic of the fNML score (csrc/disc_fnml.h) on the host.
//   1. C(2, n) of fnml_c2_table(): 1, 2, 2.5, 26/9 at n <= 3; for n <= 24 against
//      the exact rational sum_h binom(n, h) h^h (n-h)^(n-h) / n^n, whose
//      numerator and denominator fit unsigned __int128, within one FP64 ulp;
//      for every n <= 1000 against a second long double method (log-terms from
//      lgammal, compensated sum), whose own error of a few 1e-15 sets that
//      tolerance; rising with n.  `fnml_check c2` prints the 1001 values as hex
//      floats, for tests/test_fnml.py to hold to Python rationals at any n.
//   2. The ratio recurrence (fnml_log_regret, FP64) against the direct one,
//      C(k, n) = C(k-1, n) + n / (k-2) C(k-2, n), in long double, for r up to
//      255 and n up to 2^31 - 1, within the error bound derived at `tol` below;
//      both against the brute-force multinomial sum at (r, n) = (3, 4), (4, 6);
//      finite where float overflows; ln C(1, n) = ln C(r, 0) = 0.
//   3. fnml_shift(N, rmax) at N = 2 .. 2^31 - 1, rmax = 2 .. 255: the largest
//      shift <= 32 with U 2^shift < 2^62; the worst-case integer sum, counted
//      in __int128, fits 62 bits; each fixed term is within its share of it, and
//      the lemma ln C(r, n) <= n ln r holds, Szpankowski's range included.
//   4. fnml_table_fits against the product in __int128.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/disc_fnml.h"

using namespace ulg;

namespace {

long g_checks = 0;
long long g_N = 0, g_n = 0;
int g_r = 0;

#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        ++g_checks;                                                                                             \
        if (!(cond)) {                                                                                          \
            std::fprintf(stderr, "fnml_check: %s:%d: %s fails (N=%lld r=%d n=%lld)\n", __FILE__, __LINE__, #cond, \
                         g_N, g_r, g_n);                                                                        \
            std::exit(1);                                                                                       \
        }                                                                                                       \
    } while (0)

typedef __int128 i128;
typedef unsigned __int128 u128;

u128 ipow(unsigned b, unsigned e) {
    u128 x = 1;
    while (e--) x *= b;
    return x;  // 0^0 = 1
}

// C(2, n) for n > kFnmlExact as the table kernel takes it, else the table's
double c2_of(long long n) { return n <= kFnmlExact ? fnml_c2_table()[(size_t)n] : fnml_c2_szpankowski((double)n); }

// the direct recurrence on the values
long double direct_regret(int r, long long n, long double c2) {
    if (r <= 1 || n <= 0) return 1.0L;
    long double a = 1.0L, b = c2;  // C(1, n), C(2, n)
    for (int k = 3; k <= r; ++k) {
        const long double c = b + (long double)n / (long double)(k - 2) * a;
        a = b, b = c;
    }
    return b;
}

// sum over all count vectors of r parts of n: multinomial x prod (h_i / n)^h_i
long double brute(int r, int n, int left, long double weight) {
    if (r == 1) return weight * std::pow((long double)left / n, (long double)left);  // pow(0, 0) = 1
    long double s = 0, binom = 1;  // binom(left, h)
    for (int h = 0; h <= left; ++h) {
        s += brute(r - 1, n, left - h, weight * binom * std::pow((long double)h / n, (long double)h));
        binom = binom * (long double)(left - h) / (long double)(h + 1);
    }
    return s;
}

}  // namespace

int main(int argc, char **argv) {
    const std::vector<double> &c2 = fnml_c2_table();
    if (argc > 1 && std::strcmp(argv[1], "c2") == 0) {
        for (double x : c2) std::printf("%a\n", x);
        return 0;
    }
    const double ulp = 0x1p-52;
    // ---- 1. C(2, n) --------------------------------------------------------------
    CHECK(c2.size() == (size_t)kFnmlExact + 1);
    CHECK(c2[0] == 1.0 && c2[1] == 2.0 && c2[2] == 2.5 && c2[3] == (double)(26.0L / 9.0L));
    for (int n = 1; n <= 24; ++n) {
        g_n = n;
        u128 num = 0, binom = 1;
        for (int h = 0; h <= n; ++h) {
            num += binom * ipow((unsigned)h, (unsigned)h) * ipow((unsigned)(n - h), (unsigned)(n - h));
            binom = binom * (u128)(n - h) / (u128)(h + 1);  // exact: binom(n, h + 1)
        }
        const long double exact = (long double)num / (long double)ipow((unsigned)n, (unsigned)n);
        CHECK(std::fabs((long double)c2[(size_t)n] - exact) <= (long double)ulp * exact);
    }
    for (int n = 1; n <= kFnmlExact; ++n) {
        g_n = n;
        // log-terms; lgammal's absolute error at n ln n = 7000 is about 7000 x 2^-63 = 8e-16 per value
        long double sum = 0, comp = 0;
        for (int h = 0; h <= n; ++h) {
            long double lt = lgammal(n + 1.0L) - lgammal(h + 1.0L) - lgammal(n - h + 1.0L);
            if (h) lt += h * std::log((long double)h / n);
            if (n - h) lt += (n - h) * std::log((long double)(n - h) / n);
            const long double y = std::exp(lt) - comp, t = sum + y;
            comp = (t - sum) - y;
            sum = t;
        }
        CHECK(std::fabs((long double)c2[(size_t)n] - sum) <= 64 * (long double)ulp * sum);
        CHECK(c2[(size_t)n] > c2[(size_t)n - 1]);
    }
    // ---- 2. the ratio recurrence ----------------------------------------------------
    {
        g_r = 3, g_n = 4;
        const long double b34 = brute(3, 4, 4, 1.0L), b46 = brute(4, 6, 6, 1.0L), b25 = brute(2, 5, 5, 1.0L);
        CHECK(std::fabs((long double)c2[5] - b25) <= 4 * ulp * b25);
        CHECK(std::fabs(direct_regret(3, 4, c2[4]) - b34) <= 4 * ulp * b34);
        CHECK(std::fabs(direct_regret(4, 6, c2[6]) - b46) <= 4 * ulp * b46);
        CHECK(std::fabs(fnml_log_regret(3, 4, c2[4]) - (double)std::log(b34)) <= 8 * ulp);
        CHECK(std::fabs(fnml_log_regret(4, 6, c2[6]) - (double)std::log(b46)) <= 8 * ulp);
    }
    const int rs[] = {1, 2, 3, 4, 5, 17, 60, 128, 254, 255};
    const long long ns[] = {0, 1, 2, 3, 7, 100, 999, 1000, 1001, 1002, 2500, 100000, 62000000, (1ll << 31) - 1};
    double deepest = 0;
    for (int r : rs)
        for (long long n : ns) {
            g_r = r, g_n = n;
            const double x = c2_of(n);
            const double got = fnml_log_regret(r, n, x);
            CHECK(std::isfinite(got) && got >= 0.0);
            if (r == 1 || n == 0) {
                CHECK(got == 0.0);
                continue;
            }
            const long double want = std::log(direct_regret(r, n, (long double)x));
            CHECK(std::isfinite(want));
            // With u = 2^-53: the ratio rho_k = 1 + x', x' = n / ((k - 2) rho_{k-1}), carries the relative
            // error d_k <= d_{k-1} + 3 u (x' / rho_k < 1 passes d_{k-1} and two roundings on, the
            // addition rounds once); d_2 = 0 here, both sides start from the same C(2, n).  ln rho_k
            // is then off by d_k plus the log's own 2 u ln rho_k, and each of the r - 2 additions
            // rounds the partial sum, at most u ln C:
            //     sum_k 3 u (k - 2) + (2 + r - 2) u ln C  <=  u (1.5 (r - 2)(r - 1) + r ln C);
            // doubled for the long double side and the conversion of `want`.
            const double tol = 2 * 0x1p-53 * (1.5 * (r - 2) * (r - 1) + r * (double)want + 1.0);
            CHECK(std::fabs((long double)got - want) <= tol);
            deepest = got > deepest ? got : deepest;
        }
    // where the reference's float values are infinite: ln FLT_MAX = 88.72
    g_r = 60, g_n = 1000;
    CHECK(std::fabs(fnml_log_regret(60, 1000, c2[1000]) - 117.5) < 0.05);
    CHECK(fnml_log_regret(255, 2500, c2_of(2500)) > 88.73);
    CHECK(std::fabs(fnml_log_regret(255, 100000, c2_of(100000)) - 889.8) < 0.05);
    // Szpankowski's form against the exact sum where both exist, and the step at the threshold
    g_r = 2, g_n = 1000;
    CHECK(std::fabs(fnml_c2_szpankowski(1000.0) / c2[1000] - 1.0) < 6e-7);
    CHECK(fnml_c2_szpankowski(1001.0) > c2[1000] && fnml_c2_szpankowski(1001.0) < c2[1000] * 1.001);
    // ---- 3. the scale ---------------------------------------------------------------
    const long long Ns[] = {2, 3, 64, 1000, 10000, 62000000, (1ll << 31) - 1};
    const int rmaxes[] = {2, 3, 16, 255};
    const i128 two62 = (i128)1 << 62;
    int lowest = 32;
    for (long long N : Ns)
        for (int rmax : rmaxes) {
            g_N = N, g_r = rmax, g_n = 0;
            const int s = fnml_shift(N, rmax);
            const double U = fnml_sum_bound(N, rmax);
            lowest = s < lowest ? s : lowest;
            CHECK(s >= 0 && s <= 32);
            CHECK(std::ldexp(U, s) < 0x1p62);
            CHECK(s == 32 || std::ldexp(U, s + 1) >= 0x1p62);
            // the worst case: counts that add up to N twice, at most 3 N terms of 1/2 each
            const i128 lnN = (i128)std::ceil(std::ldexp(std::log((long double)N) * (1.0L + 0x1p-60L), s));
            const i128 lnr = (i128)std::ceil(std::ldexp(std::log((long double)rmax) * (1.0L + 0x1p-60L), s));
            CHECK((i128)N * (2 * lnN + lnr) + 2 * (i128)N < two62);
            const long long terms[] = {1, 2, 3, 1000, 1001, N / 2, N - 1, N};
            for (long long n : terms) {
                if (n < 1 || n > N) continue;
                g_n = n;
                const double nln = (double)n * std::log((double)n);
                CHECK((i128)fnml_fix(nln, s) <= (i128)n * lnN + 1);
                CHECK(std::fabs(fnml_unfix(fnml_fix(nln, s), s) - nln) <= std::ldexp(1.0, -(s + 1)));
                double below = 0;
                for (int r : {2, 3, rmax}) {
                    if (r > rmax) continue;
                    const double reg = fnml_log_regret(r, n, c2_of(n));
                    CHECK(reg >= below);  // rises with the arity
                    below = reg;
                    CHECK(reg <= (double)n * std::log((double)r) * (1.0 + 0x1p-40));  // C(r, n) <= r^n
                    const long long f = fnml_fix(reg, s);
                    CHECK(f >= 0 && (i128)f <= (i128)n * lnr + 1);
                    CHECK(std::fabs(fnml_unfix(f, s) - reg) <= std::ldexp(1.0, -(s + 1)));
                }
            }
        }
    CHECK(lowest < 32 && lowest >= 25);
    CHECK(fnml_shift(2, 2) == 32 && fnml_shift(2500, 255) == 32 && fnml_shift((1ll << 31) - 1, 255) == 25);
    // ---- 4. the size of the device table ----------------------------------------------
    g_N = g_n = 0, g_r = 0;
    const int rows_[] = {0, 1, 2, 3, 7, 254};
    const long long tN[] = {2, 2500, (1ll << 20) - 1, 1ll << 20, (1ll << 27) - 1, 1ll << 27, (1ll << 28) - 1, 1ll << 28,
                            1056831, 1056832, (1ll << 31) - 1};
    for (int rows : rows_)
        for (long long N : tN) {
            g_r = rows, g_N = N;
            CHECK(fnml_table_fits(rows, N) == ((i128)rows * ((i128)N + 1) <= (i128)kFnmlMaxEntries));
        }
    CHECK(fnml_table_fits(1, (1ll << 28) - 1) && !fnml_table_fits(1, 1ll << 28) && !fnml_table_fits(254, (1ll << 31) - 1));
    CHECK(!fnml_table_fits(-1, 10) && !fnml_table_fits(1, -1));
    std::printf("fnml_check ok (%ld checks, lowest shift %d, largest ln C %.1f)\n", g_checks, lowest, deepest);
    return 0;
}
