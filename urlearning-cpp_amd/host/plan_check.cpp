// plan_check -- the scoring call's host arithmetic (csrc/score_plan.h:
// ScoreLists, CbicPlan) against brute-force enumeration of parent sets: slot
// offsets, the launches' phase counts, the stream groups' stripes, queue
// words, segment-counter offsets, hi-cover offsets, the compact constraint
// table and the wide pool's per-variable prefixes.  No formula of the plan is
// reused here: every count comes from walking the subsets of a candidate mask.
// Built with AddressSanitizer + UBSan by `make sanitize` (tests/test_sanitize.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/score_plan.h"

using namespace ulg;

namespace {

long g_checks = 0;
char g_case[256];

#define CHECK(cond)                                                                         \
    do {                                                                                    \
        ++g_checks;                                                                         \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "plan_check: %s:%d: %s fails in %s\n", __FILE__, __LINE__, #cond, g_case); \
            std::exit(1);                                                                   \
        }                                                                                   \
    } while (0)

// Brute[i][L][ph]: subsets of variable i's candidates of L <= max_parents
// members, ph 0 = holding variable 0 (layers >= 1), ph 1 = the rest
struct Brute {
    int kmax = 0;
    std::vector<std::vector<uint64_t>> cnt[2];
    std::vector<uint64_t> C;
    std::vector<int> m;
};

Brute enumerate(int n, const std::vector<int> &vars, const std::vector<uint64_t> &masks, int maxp) {
    Brute b;
    const int nv = (int)vars.size();
    for (int ph = 0; ph < 2; ++ph) b.cnt[ph].assign(nv, std::vector<uint64_t>(n + 1, 0));
    for (int i = 0; i < nv; ++i) {
        uint64_t C = 0;
        for (int v = 0; v < n; ++v)
            if (v != vars[i] && ((masks[i] >> v) & 1ull)) C |= 1ull << v;
        b.C.push_back(C);
        b.m.push_back(__builtin_popcountll(C));
        uint64_t s = 0;
        do {  // every subset of C
            const int L = __builtin_popcountll(s);
            if (L <= maxp) {
                ++b.cnt[L >= 1 && (s & 1ull) ? 0 : 1][i][L];
                b.kmax = std::max(b.kmax, L);
            }
            s = (s - C) & C;
        } while (s);
    }
    return b;
}

void check_case(int n, const std::vector<int> &vars, const std::vector<uint64_t> &masks, int max_parents,
                const Options &o, bool with_cons, ScoreLists &ls, CbicPlan &p) {
    const int nv = (int)vars.size();
    const int maxp = (max_parents < 1 || max_parents > n - 1) ? n - 1 : max_parents;
    const Brute b = enumerate(n, vars, masks, maxp);

    CHECK(ls.build(n, vars.data(), nv, masks.data(), max_parents) == ScoreLists::kOk);
    CHECK(ls.max_parents == maxp && ls.kmax == b.kmax && ls.S == b.kmax + 1);
    const int kmax = b.kmax, S = kmax + 1;
    // slots
    uint64_t acc = 0;
    CHECK(ls.toff.size() == (size_t)nv * S + 1);
    for (int i = 0; i < nv; ++i) {
        CHECK(ls.mv[i] == b.m[i] && ls.cmask[i] == b.C[i]);
        uint64_t back = 0;
        for (int k = 0; k < ls.mv[i]; ++k) {
            CHECK(k == 0 || ls.cand[(size_t)i * 64 + k] > ls.cand[(size_t)i * 64 + k - 1]);
            back |= 1ull << ls.cand[(size_t)i * 64 + k];
        }
        CHECK(back == b.C[i]);
        for (int L = 0; L < S; ++L) {
            CHECK(ls.toff[(size_t)i * S + L] == acc);
            CHECK(ls.slab_count(i, L) == b.cnt[0][i][L] + b.cnt[1][i][L]);
            acc += b.cnt[0][i][L] + b.cnt[1][i][L];
        }
    }
    CHECK(ls.toff[(size_t)nv * S] == acc && ls.total_slots == acc);
    for (int L = 0; L <= kmax; ++L) {
        int64_t upto = 0;
        for (int i = 0; i < nv; ++i)
            for (int l = 0; l <= L; ++l) upto += (int64_t)(b.cnt[0][i][l] + b.cnt[1][i][l]);
        CHECK(ls.scored_up_to(L) == upto);
    }

    std::vector<int> cv;
    std::vector<uint64_t> cr, cf;
    if (with_cons) {
        // three alternatives: two of variable 3 (the second may name
        // non-candidates), one of variable 5 requiring itself (unsatisfiable)
        cv = {3, 3, 5};
        cr = {1ull << 1, (1ull << 0) | (1ull << 4), 1ull << 5};
        cf = {1ull << 2, 1ull << 7, 0};
    }
    const bool wck = false;  // the ULG_WALK_CLOCK diagnostics are off
    p.build(ls, cv, cr, cf, o, wck);
    CHECK(p.nv == nv && p.kmax == kmax);
    for (int i = 0; i < nv; ++i)
        CHECK(p.meta[i * 4] == vars[i] && p.meta[i * 4 + 1] == b.m[i] && p.meta[i * 4 + 2] == (int)(b.C[i] & 1ull));

    // phase counts
    CHECK(p.work.size() == (size_t)(kmax + 1) * 2 * (nv + 1));
    for (int L = 0; L <= kmax; ++L)
        for (int ph = 0; ph < 2; ++ph) {
            const uint64_t *w = &p.work[((size_t)L * 2 + ph) * (nv + 1)];
            CHECK(w[0] == 0);
            for (int i = 0; i < nv; ++i) CHECK(w[i + 1] - w[i] == (L >= 1 ? b.cnt[ph][i][L] : 0));
        }
    // variant, groups and their stripes
    const bool two_pass = (o.score_variant & 16) != 0;
    CHECK(p.variant == o.score_variant);  // far below 2^30 slots
    CHECK(p.G == (two_pass && !wck ? std::max(1, std::min((int)o.score_streams, nv)) : 1));
    const int G = p.G;
    std::vector<uint64_t> gcnt((size_t)G * (kmax + 1) * 2, 0);  // brute-force launch sizes
    for (int g = 0; g < G; ++g)
        for (int L = 1; L <= kmax; ++L)
            for (int ph = 0; ph < 2; ++ph) {
                uint64_t s = 0;
                for (int i = 0; i < nv; ++i)
                    if (i % G == g) s += b.cnt[ph][i][L];
                gcnt[((size_t)g * (kmax + 1) + L) * 2 + ph] = s;
                CHECK(p.launch_count(g, L, ph) == s);
                if (G > 1) {
                    const uint64_t *wg = &p.workg[p.work_offset(g, L, ph)];
                    CHECK(wg[0] == 0);
                    for (int i = 0; i < nv; ++i) CHECK(wg[i + 1] - wg[i] == (i % G == g ? b.cnt[ph][i][L] : 0));
                }
            }
    CHECK(G > 1 ? p.workg.size() == (size_t)G * p.work.size() : p.workg.empty());
    // queue words, segment counters
    CHECK(p.segoff.size() == (size_t)G * 2 * (kmax + 1) + 1 && p.segoff[0] == 0);
    CHECK(p.nqc == (size_t)G * 2 * (kmax + 1) + 1);
    uint64_t nseg56 = 1;
    for (int g = 0; g < G; ++g)
        for (int L = 0; L <= kmax; ++L)
            for (int ph = 0; ph < 2; ++ph) {
                const uint64_t cnt = gcnt[((size_t)g * (kmax + 1) + L) * 2 + ph];
                const uint64_t blocks = (cnt + kBlock - 1) / kBlock;
                const uint64_t nseg = (blocks + kSegBlocks - 1) / kSegBlocks;
                const bool queued = two_pass && L >= 1 && L <= kMaxL;
                if (queued) CHECK(p.qwords >= nseg * kSegEntries * (uint64_t)(1 + 2 * bits_words(L)));
                if (L > kMaxL) CHECK(p.wqwords >= 6 * cnt);
                if (L == 5 || L == 6) nseg56 = std::max(nseg56, nseg);
                const size_t s = p.seg_slot(g, L, ph);
                CHECK(s == ((size_t)g * (kmax + 1) + L) * 2 + ph);
                CHECK(p.segoff[s + 1] >= p.segoff[s]);
                const uint64_t room = p.segoff[s + 1] - p.segoff[s];
                const uint64_t hdr = queued && (L == 5 || L == 6) && cnt ? (uint64_t)kBucketHdrWords : 0;
                CHECK(room == (queued ? nseg * kSegStride : 0) + hdr);
            }
    if (!two_pass) CHECK(p.qwords == 0 && p.segoff.back() == 0);
    if (kmax <= kMaxL) CHECK(p.wqwords == 0);
    CHECK(p.nseg_max == nseg56);
    CHECK(p.qcap % 256 == 0 && 3 * p.qcap >= p.qwords && p.wave_cap == p.qcap / 64 + kBucketMax);
    CHECK(p.zero_q == (two_pass || kmax > kMaxL));
    CHECK(p.nqseg == (p.zero_q ? std::max<uint64_t>(p.segoff.back(), 1) : 0));
    CHECK(p.bucket == ((o.score_variant & 112) == 112 && o.walk_bucket && !wck && kmax >= 5));
    // small and fused layers
    CHECK(p.Ls == (two_pass && !wck ? std::min(kmax, std::min(kMaxL, (int)o.score_small_layers)) : 0));
    CHECK(p.vsmall == (o.score_variant & 65));
    CHECK(p.Lf == (p.vsmall == 65 && o.time_limit_ms == 0 ? std::min(p.Ls, (int)o.score_fused) : 0));
    CHECK(p.nb == (int64_t)((acc + kSlotsPerBlock - 1) / kSlotsPerBlock));
    // hi-cover offsets, the checked-bitset slice
    {
        uint64_t run = 0;
        bool any = false;
        for (int i = 0; i < nv; ++i) {
            int top = 0;
            for (int L = 0; L <= kmax; ++L)
                if (b.cnt[0][i][L] + b.cnt[1][i][L]) top = L;
            const bool has = kmax > kMaxL && o.wide_prune && top > kMaxL && b.m[i] <= kHiMaxBits;
            if (!p.hoff.empty()) CHECK(p.hoff[i] == (has ? run : ~0ull));
            if (has) run += 1ull << b.m[i];
            any = any || has;
        }
        CHECK(p.hoff.empty() == !any && p.htot == run);
        if (kmax > kMaxL) CHECK(p.wslice * G <= std::max<uint64_t>(kWideBitsWords, (uint64_t)G << (kmax + 1 - 6)) &&
                                p.wslice >= (1ull << (kmax + 1 - 6)));
        else CHECK(p.wslice == 0);
    }
    // the constraint table
    {
        size_t pairs = 0;
        std::vector<std::vector<uint64_t>> want(nv);
        for (int i = 0; i < nv; ++i) {
            bool any = false;
            for (size_t j = 0; j < cv.size(); ++j) {
                if (cv[j] != vars[i]) continue;
                any = true;
                if (cr[j] & ~b.C[i]) continue;
                want[i].push_back(cr[j]);
                want[i].push_back(cf[j] & b.C[i]);
            }
            if (any && want[i].empty()) want[i] = {1ull << 63, 0};
            pairs += want[i].size() / 2;
        }
        if (pairs == 0) {
            CHECK(p.cons_words == 0 && p.cons_lds == 0);
        } else {
            CHECK(p.cons_words == (int)(nv + 1 + 2 * pairs) && p.ct.size() == (size_t)p.cons_words);
            CHECK(p.cons_lds == (p.cons_words <= kConsLdsWords ? p.cons_words * 8 : 0));
            CHECK(p.ct[nv] == pairs);
            for (int i = 0; i < nv; ++i) {
                CHECK(p.ct[i + 1] - p.ct[i] == want[i].size() / 2);
                for (size_t k = 0; k < want[i].size(); ++k) {
                    const uint64_t cm = p.ct[(size_t)nv + 1 + 2 * p.ct[i] + k];
                    uint64_t vm = cm & (1ull << 63);  // the sentinel names no candidate
                    for (int q = 0; q < b.m[i]; ++q)
                        if ((cm >> q) & 1ull) vm |= 1ull << ls.cand[(size_t)i * 64 + q];
                    CHECK((cm & ~(1ull << 63)) >> b.m[i] == 0);
                    CHECK(vm == want[i][k]);
                }
            }
        }
    }
    // the pool's per-variable prefixes
    {
        int lo = 64, hi = -1;
        std::vector<int> widev;
        for (int i = 0; i < nv; ++i)
            if (std::min(b.m[i], maxp) > kMaxL) {
                widev.push_back(i);
                lo = std::min(lo, b.m[i]);
                hi = std::max(hi, b.m[i]);
            }
        const bool pool = (o.wide_pool == 1 || (o.wide_pool == 2 && hi >= 0 && hi - lo >= 2)) && kmax > kMaxL &&
                          G > 1 && o.time_limit_ms == 0;
        CHECK(p.use_pool == pool);
        if (!pool) {
            CHECK(p.vw.empty() && p.pool_order.empty());
        } else {
            CHECK(p.pool_order.size() == widev.size() && p.vw.size() == widev.size() * p.work.size());
            uint64_t seen = 0;
            for (size_t k = 0; k < p.pool_order.size(); ++k) {
                const int i = p.pool_order[k];
                CHECK(std::min(b.m[i], maxp) > kMaxL && !((seen >> i) & 1ull));
                seen |= 1ull << i;
                if (k) {
                    const int prev = p.pool_order[k - 1];
                    CHECK(b.m[prev] > b.m[i] || (b.m[prev] == b.m[i] && prev < i));
                }
                for (int L = 0; L <= kmax; ++L)
                    for (int ph = 0; ph < 2; ++ph) {
                        const uint64_t *v = &p.vw[k * p.work.size() + ((size_t)L * 2 + ph) * (nv + 1)];
                        const uint64_t share = L > kMaxL ? b.cnt[ph][i][L] : 0;
                        CHECK(v[0] == 0 && v[nv] == share);
                        for (int j = 0; j < nv; ++j) CHECK(v[j + 1] - v[j] == (j == i ? share : 0));
                    }
            }
        }
    }
}

}  // namespace

int main() {
    const int n = 12;
    std::vector<int> all12(n);
    for (int i = 0; i < n; ++i) all12[i] = i;
    const std::vector<int> sub7 = {1, 2, 3, 5, 7, 8, 11};  // variable 0 is a candidate only
    // variable 8 has exactly kMaxL candidates: it reaches no wide layer while its neighbours do
    const uint64_t sparse[12] = {0x0b6, 0xfff, 0x3d5, 0x801, 0x7fe, 0x000, 0xaaa, 0x555, 0xe1f, 0x3ff, 0xffe, 0x123};
    ScoreLists ls;  // reused across the cases, as the context reuses its own
    CbicPlan plan;
    long cases = 0;
    for (const std::vector<int> &vars : {all12, sub7})
        for (int mk = 0; mk < 3; ++mk) {
            std::vector<uint64_t> masks;
            for (int v : vars) masks.push_back(mk == 0 ? 0xfffull : mk == 1 ? 0xffeull : sparse[v]);
            for (int max_parents : {0, 1, 4, 6, 8, 10})
                for (int streams : {1, 3})
                    for (int variant : {1, 113, 241})
                        for (int cons = 0; cons < 2; ++cons)
                            for (int alt = 0; alt < 3; ++alt) {
                                Options o;  // alt 1: the pool forced, no pruning; alt 2: -r and the queue-order walk
                                o.score_variant = variant;
                                o.score_streams = streams;
                                if (alt == 1) o.wide_pool = 1, o.wide_prune = 0;
                                if (alt == 2) o.time_limit_ms = 1000, o.walk_bucket = 0;
                                std::snprintf(g_case, sizeof g_case,
                                              "nv=%d masks=%d max_parents=%d streams=%d variant=%d cons=%d alt=%d",
                                              (int)vars.size(), mk, max_parents, streams, variant, cons, alt);
                                check_case(n, vars, masks, max_parents, o, cons != 0, ls, plan);
                                ++cases;
                            }
        }
    // the lists' refusals
    const int dup[3] = {1, 2, 1}, far[2] = {0, 12};
    const uint64_t m3[3] = {0xfff, 0xfff, 0xfff};
    if (ls.build(n, dup, 3, m3, 2) != ScoreLists::kNotDistinct || ls.build(n, far, 2, m3, 2) != ScoreLists::kNotDistinct ||
        ls.build(n, nullptr, 3, m3, 2) != ScoreLists::kBadList || ls.build(2, dup, 3, m3, 2) != ScoreLists::kBadList) {
        std::fprintf(stderr, "plan_check: a bad variable list was accepted\n");
        return 1;
    }
    std::printf("plan_check ok: %ld cases, %ld checks\n", cases, g_checks);
    return 0;
}
