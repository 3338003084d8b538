// unrank_lut_check -- the host side of the scorer's unrank tables and of the
// set rank the two-pass kernels take from child_ranks (csrc/score_plan.h).
//
//   unrank_lut_check ranks
//       For every candidate count m <= 12 and layer L <= 6, every L-subset of
//       m compact indices in Gosper's order (the order the kernels' ranks
//       index): child_ranks_t's return value must be the set's enumeration
//       index, and its children's ranks those of the set minus one member
//       (and, with variable 0 toggled in, plus compact index 0), each found
//       here by counting the smaller sets, not from a binomial sum.
//   unrank_lut_check plan CAP MAXP N V:MASK... [ / CAP MAXP N V:MASK... ]...
//       One scoring call per group, all on one cache, as ulg_cbic_score makes
//       them: prints the tables the cache holds after each call and the
//       call's per-launch offsets, for tests/test_unrank_lut_host.py to
//       compare with its own statement of the rule.  MASK is hexadecimal.
//
// Plain C++17; built with AddressSanitizer + UBSan by `make sanitize`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/score_plan.h"

using namespace ulg;

namespace {

constexpr int kStride = kMaxL + 2;  // the device table's columns (ulg_internal.h kBinomK)

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::fprintf(stderr, "unrank_lut_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

std::vector<uint32_t> table() {
    std::vector<uint32_t> b(64 * kStride);
    for (int a = 0; a < 64; ++a)
        for (int k = 0; k < kStride; ++k) {
            const uint64_t v = binom64(a, k);
            b[a * kStride + k] = v > 0xffffffffull ? 0xffffffffu : (uint32_t)v;
        }
    return b;
}

// every l-subset of m indices in Gosper's order
std::vector<uint64_t> subsets(int m, int l) {
    std::vector<uint64_t> out;
    if (l == 0) return {0ull};
    if (l > m) return out;
    uint64_t s = (1ull << l) - 1ull;
    const uint64_t lim = 1ull << m;
    while (s < lim) {
        out.push_back(s);
        const uint64_t c = s & -s, r = s + c;
        s = (((r ^ s) >> 2) / c) | r;
    }
    return out;
}

long index_of(const std::vector<uint64_t> &v, uint64_t s) {
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] == s) return (long)i;
    return -1;
}

template <int L>
long check_ranks(const std::vector<uint32_t> &b, int m) {
    const std::vector<uint64_t> sets = subsets(m, L), below = subsets(m, L - 1);
    long checks = 0;
    for (size_t i = 0; i < sets.size(); ++i) {
        const uint64_t cm = sets[i];
        uint64_t rc[L], rz[L];
        CHECK((child_ranks_t<L, false, kStride>(cm, b.data(), rc, rz)) == (uint32_t)i);
        uint64_t rc1[L], rz1[L];
        CHECK((child_ranks_t<L, true, kStride>(cm, b.data(), rc1, rz1)) == (uint32_t)i);
        uint64_t rem = cm;
        for (int j = 0; j < L; ++j) {
            const uint64_t bit = rem & -rem;
            rem &= rem - 1;
            CHECK((long)rc[j] == index_of(below, cm ^ bit) && rc1[j] == rc[j]);
            if (!(cm & 1ull)) CHECK((long)rz1[j] == index_of(sets, (cm ^ bit) | 1ull));
            checks += 3;
        }
    }
    return checks;
}

int run_ranks() {
    const std::vector<uint32_t> b = table();
    long checks = 0;
    for (int m = 1; m <= 12; ++m) {
        if (m >= 1) checks += check_ranks<1>(b, m);
        if (m >= 2) checks += check_ranks<2>(b, m);
        if (m >= 3) checks += check_ranks<3>(b, m);
        if (m >= 4) checks += check_ranks<4>(b, m);
        if (m >= 5) checks += check_ranks<5>(b, m);
        if (m >= 6) checks += check_ranks<6>(b, m);
    }
    std::printf("unrank_lut_check ok: %ld rank checks\n", checks);
    return 0;
}

int run_plan(int argc, char **argv) {
    LutCache cache;
    ScoreLists ls;
    CbicPlan p;
    int a = 2, call = 0;
    while (a < argc) {
        if (argc - a < 4) return 2;
        const long long cap = std::atoll(argv[a]);
        const int maxp = std::atoi(argv[a + 1]), n = std::atoi(argv[a + 2]);
        a += 3;
        std::vector<int> vars;
        std::vector<uint64_t> masks;
        for (; a < argc && std::strcmp(argv[a], "/") != 0; ++a) {
            char *colon = nullptr;
            vars.push_back((int)std::strtol(argv[a], &colon, 10));
            if (!colon || *colon != ':') return 2;
            masks.push_back(std::strtoull(colon + 1, nullptr, 16));
        }
        if (a < argc) ++a;  // the separator
        if (ls.build(n, vars.data(), (int)vars.size(), masks.data(), maxp) != ScoreLists::kOk) return 3;
        Options o;
        o.score_unrank_lut = cap;
        p.build(ls, {}, {}, {}, o, false);
        p.build_luts(ls, cap, cache);
        std::printf("CALL %d kmax %d any %d new %zu total %llu\n", call++, p.kmax, p.lut_any ? 1 : 0, p.lut_new.size(),
                    (unsigned long long)cache.total);
        for (const LutTable &t : cache.tables)
            std::printf("T %d %d %llu %llu\n", t.U, t.l, (unsigned long long)t.off, (unsigned long long)t.count);
        for (const LutTable &t : p.lut_new) CHECK(cache.find(t.U, t.l) && cache.find(t.U, t.l)->off == t.off);
        CHECK(p.lutoff.empty() == !p.lut_any);
        for (int L = 1; L <= p.kmax && p.lut_any; ++L)
            for (int ph = 0; ph < 2; ++ph)
                for (int i = 0; i < p.nv; ++i) {
                    const int32_t off = p.lutoff[p.lut_offset(L, ph) + i];
                    if (off < 0) continue;
                    // a launch's lanes index the table with the variable's set
                    // ranks: the table must hold exactly that many entries
                    const uint64_t *w = &p.work[((size_t)L * 2 + ph) * (p.nv + 1)];
                    bool sized = false;
                    for (const LutTable &t : cache.tables)
                        if ((int64_t)t.off == off) sized = t.count == w[i + 1] - w[i];
                    CHECK(sized);
                    std::printf("O %d %d %d %d\n", L, ph, i, (int)off);
                }
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "ranks") == 0) return run_ranks();
    if (argc >= 2 && std::strcmp(argv[1], "plan") == 0) return run_plan(argc, argv);
    std::fprintf(stderr, "usage: unrank_lut_check ranks | plan CAP MAXP N V:MASK... [ / CAP MAXP N V:MASK... ]...\n");
    return 2;
}
