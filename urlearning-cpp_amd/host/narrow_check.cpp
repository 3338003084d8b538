// narrow_check -- the host side of the layer kernels' narrow form (option
// score_narrow; csrc/score_plan.h).
//
//   narrow_check ranks
//       child_ranks_t and mask_elements over 32-bit masks against the same
//       functions over 64-bit masks: the set's rank, every child's rank with
//       and without variable 0 toggled in, and the elements.  Every set of
//       m <= 12 candidates and L <= 6 members, every set of L <= 3 at m = 32,
//       and a seeded sample of L = 5 and 6 at m = 31 and 32 that always holds
//       the top set {m - L, ..., m - 1} (bit 31 at m = 32) and {0, ..., L - 1}.
//   narrow_check rule
//       CbicPlan::narrow_fits just inside and just outside each condition,
//       and narrow_built's (layer, variant) pairs.
//   narrow_check plan NARROW VARIANT STREAMS MAXP N V:MASK...
//       One scoring call as ulg_cbic_score plans it: prints which launches
//       take the narrow form, for tests/test_narrow_host.py to compare with
//       its own statement of the rule.  MASK is hexadecimal.
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

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            std::fprintf(stderr, "narrow_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                         \
        }                                                                                         \
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

// one set: both widths of both functions, field by field
template <int L>
long check_set(const std::vector<uint32_t> &b, uint64_t cm) {
    CHECK(__builtin_popcountll(cm) == L && (cm >> 32) == 0);
    const uint32_t cn = (uint32_t)cm;
    uint64_t rc[L], rz[L], rc1[L], rz1[L];
    uint32_t nc[L], nz[L], nc1[L], nz1[L];
    const uint32_t r64 = child_ranks_t<L, false, kStride>(cm, b.data(), rc, rz);
    const uint32_t r32 = child_ranks_t<L, false, kStride>(cn, b.data(), nc, nz);
    const uint32_t q64 = child_ranks_t<L, true, kStride>(cm, b.data(), rc1, rz1);
    const uint32_t q32 = child_ranks_t<L, true, kStride>(cn, b.data(), nc1, nz1);
    CHECK(r64 == r32 && q64 == q32 && r64 == q64);
    int e64[L], e32[L];
    mask_elements<L>(cm, e64);
    mask_elements<L>(cn, e32);
    uint64_t rebuilt = 0;
    for (int j = 0; j < L; ++j) {
        // the 64-bit children's ranks of the unrolled layers fit 32 bits
        CHECK((rc[j] >> 32) == 0 && (rz[j] >> 32) == 0 && (rc1[j] >> 32) == 0 && (rz1[j] >> 32) == 0);
        CHECK(nc[j] == (uint32_t)rc[j] && nz[j] == (uint32_t)rz[j]);
        CHECK(nc1[j] == (uint32_t)rc1[j] && nz1[j] == (uint32_t)rz1[j]);
        CHECK(e64[j] == e32[j] && e32[j] >= 0 && e32[j] < 32 && (j == 0 || e32[j] > e32[j - 1]));
        rebuilt |= 1ull << e32[j];
    }
    CHECK(rebuilt == cm);
    return 4 * L + 4;
}

template <int L>
long check_all(const std::vector<uint32_t> &b, int m) {
    if (L > m) return 0;
    long checks = 0;
    uint64_t s = (1ull << L) - 1ull;
    const uint64_t lim = 1ull << m;
    while (s < lim) {  // Gosper's order
        checks += check_set<L>(b, s);
        const uint64_t c = s & -s, r = s + c;
        s = (((r ^ s) >> 2) / c) | r;
    }
    return checks;
}

// a seeded sample of L-subsets of m indices, the two extreme sets first
template <int L>
long check_sample(const std::vector<uint32_t> &b, int m, uint64_t &seed, int count) {
    long checks = 0;
    checks += check_set<L>(b, ((1ull << L) - 1ull) << (m - L));  // m = 32, L = 6: {26, ..., 31}
    checks += check_set<L>(b, (1ull << L) - 1ull);               // {0, ..., L - 1}
    for (int i = 0; i < count; ++i) {
        uint64_t s = 0;
        while (__builtin_popcountll(s) < L) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            s |= 1ull << ((seed >> 33) % (uint64_t)m);
        }
        checks += check_set<L>(b, s);
    }
    return checks;
}

int run_ranks() {
    const std::vector<uint32_t> b = table();
    long checks = 0;
    for (int m = 1; m <= 12; ++m) {
        checks += check_all<1>(b, m);
        checks += check_all<2>(b, m);
        checks += check_all<3>(b, m);
        checks += check_all<4>(b, m);
        checks += check_all<5>(b, m);
        checks += check_all<6>(b, m);
    }
    checks += check_all<1>(b, 32);
    checks += check_all<2>(b, 32);
    checks += check_all<3>(b, 32);
    uint64_t seed = 0x9e3779b97f4a7c15ull;
    for (int m = 31; m <= 32; ++m) {
        checks += check_sample<5>(b, m, seed, 20000);
        checks += check_sample<6>(b, m, seed, 20000);
    }
    std::printf("narrow_check ok: %ld rank checks\n", checks);
    return 0;
}

int run_rule() {
    // candidates: 32 against 33
    CHECK(CbicPlan::narrow_fits(32, 1, 1) && !CbicPlan::narrow_fits(33, 1, 1));
    CHECK(CbicPlan::narrow_fits(1, 1, 1) && !CbicPlan::narrow_fits(63, 1, 1));
    // sets: the last block's lanes past the launch's sets still index below 2^32
    const uint64_t two32 = 1ull << 32;
    CHECK(CbicPlan::narrow_fits(32, two32 - kBlock, 1) && !CbicPlan::narrow_fits(32, two32 - kBlock + 1, 1));
    CHECK(!CbicPlan::narrow_fits(32, two32, 1) && !CbicPlan::narrow_fits(32, ~0ull, 1));  // no wrap-around
    // slots: 32-bit byte offsets
    CHECK(CbicPlan::narrow_fits(32, 1, (1ull << 30) - 1) && !CbicPlan::narrow_fits(32, 1, 1ull << 30));
    CHECK(!CbicPlan::narrow_fits(32, 1, ~0ull));
    // the kernels built: the default variant's layers 5 and 6
    for (int L = 0; L <= kMaxL + 1; ++L)
        for (int v : {1, 49, 65, 113, 241}) CHECK(CbicPlan::narrow_built(L, v) == (v == 241 && (L == 5 || L == 6)));
    std::printf("narrow_check ok: rule\n");
    return 0;
}

int run_plan(int argc, char **argv) {
    if (argc < 8) return 2;
    Options o;
    o.score_narrow = std::atoll(argv[2]);
    o.score_variant = std::atoll(argv[3]);
    o.score_streams = std::atoll(argv[4]);
    const int maxp = std::atoi(argv[5]), n = std::atoi(argv[6]);
    std::vector<int> vars;
    std::vector<uint64_t> masks;
    for (int a = 7; a < argc; ++a) {
        char *colon = nullptr;
        vars.push_back((int)std::strtol(argv[a], &colon, 10));
        if (!colon || *colon != ':') return 2;
        masks.push_back(std::strtoull(colon + 1, nullptr, 16));
    }
    ScoreLists ls;
    CbicPlan p;
    if (ls.build(n, vars.data(), (int)vars.size(), masks.data(), maxp) != ScoreLists::kOk) return 3;
    p.build(ls, {}, {}, {}, o, false);
    std::printf("PLAN variant %d G %d Ls %d kmax %d narrow_launches %d\n", p.variant, p.G, p.Ls, p.kmax, p.narrow_launches);
    int seen = 0;
    for (int g = 0; g < p.G; ++g)
        for (int L = 1; L <= std::min(p.kmax, kMaxL); ++L)
            for (int ph = 0; ph < 2; ++ph) {
                const bool nw = p.launch_narrow(g, L, ph);
                // a narrow launch is an unrolled group launch with sets
                if (nw) CHECK(L > p.Ls && p.launch_count(g, L, ph) > 0 && CbicPlan::narrow_built(L, p.variant));
                seen += nw;
                if (L > p.Ls && p.launch_count(g, L, ph))
                    std::printf("LAUNCH %d %d %d %llu %d\n", g, L, ph, (unsigned long long)p.launch_count(g, L, ph), nw ? 1 : 0);
            }
    CHECK(seen == p.narrow_launches);
    // a second build with the option off clears every flag (the plan is reused)
    o.score_narrow = 0;
    p.build(ls, {}, {}, {}, o, false);
    CHECK(p.narrow_launches == 0);
    for (int g = 0; g < p.G; ++g)
        for (int L = 0; L <= p.kmax; ++L)
            for (int ph = 0; ph < 2; ++ph) CHECK(!p.launch_narrow(g, L, ph));
    std::printf("narrow_check ok: plan\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "ranks") == 0) return run_ranks();
    if (argc >= 2 && std::strcmp(argv[1], "rule") == 0) return run_rule();
    if (argc >= 2 && std::strcmp(argv[1], "plan") == 0) return run_plan(argc, argv);
    std::fprintf(stderr, "usage: narrow_check ranks | rule | plan NARROW VARIANT STREAMS MAXP N V:MASK...\n");
    return 2;
}
