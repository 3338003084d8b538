// order_search_check -- the arithmetic of the order search
// (csrc/order_search_dev.h) on the host.
//   1. the images: a float's and a double's are monotone over every class --
//      +-0 (one image), denormals, normals of both signs, the extremes -- and
//      the float's inverts; an entry key's maximum is the maximal score at its
//      least index, 0 without a compatible entry;
//   2. the bookkeeping: searches on random small lists, run as the kernel runs
//      them -- the swaps' would-be terms cached, after a move the reverse
//      swap's taken from the terms just left and the two neighbours' rescanned
//      -- hold at every step the gains, terms and S of a recompute from the
//      lists; tabu, aspiration and the least-p tie rule included;
//   3. the kick: os_kick leaves a permutation, draws as mcmc_move does, and an
//      order with a -inf term is undone to the best order and its terms.
// Built plain and with AddressSanitizer + UBSan (`make sanitize`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../csrc/order_search_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                                 \
    do {                                                                                            \
        ++g_checks;                                                                                 \
        if (!(cond)) {                                                                              \
            std::fprintf(stderr, "order_search_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                           \
        }                                                                                           \
    } while (0)

const double kInf = std::numeric_limits<double>::infinity();

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

uint32_t bits_of(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

void check_images() {
    std::vector<float> f = {0.0f, -0.0f, 1e-45f, -1e-45f, 1.1e-38f, -1.1e-38f, 1.17549435e-38f, -1.17549435e-38f, 1.0f, -1.0f,
                            1.0000001f, -1.0000001f, 3.402823466e+38f, -3.402823466e+38f, -17.25f, -17.5f, 2e4f};
    for (int i = 0; i < 200; ++i) {
        const uint32_t b = (uint32_t)rnd();
        float x;
        std::memcpy(&x, &b, 4);
        if (x == x) f.push_back(x);  // no NaN: the lists' check refuses them
    }
    for (float a : f) {
        const uint32_t ia = os_float_image(bits_of(a));
        CHECK(ia != 0u);
        CHECK(os_float_bits(ia) == (a == 0.0f ? 0u : bits_of(a)));
        CHECK(os_decode(os_entry_key(bits_of(a), 7)).b == (double)a && os_decode(os_entry_key(bits_of(a), 7)).ent == 7u);
        for (float b : f) {
            CHECK((a < b) == (ia < os_float_image(bits_of(b))) && (a == b) == (ia == os_float_image(bits_of(b))));
            CHECK(((double)a < (double)b) == (os_double_image((double)a) < os_double_image((double)b)));
            CHECK(((double)a == (double)b) == (os_double_image((double)a) == os_double_image((double)b)));
        }
    }
    CHECK(os_double_image(-kInf) < os_double_image(-1e300) && os_double_image(-1e300) < os_double_image(-5e-324));
    CHECK(os_double_image(-5e-324) < os_double_image(0.0) && os_double_image(0.0) < os_double_image(5e-324) && os_double_image(-kInf) != 0);
    // the maximum at its least index; a tie of -0 and +0; nothing compatible
    const uint64_t sets[6] = {0x2, 0x0, 0x4, 0x6, 0x0, 1ull << 62};
    const float scores[6] = {5.0f, -3.0f, -1.0f, -1.0f, -3.0f, 9.0f};
    OsBest r = os_decode(os_best_serial(sets, scores, 0, 6, 0x6));
    CHECK(r.b == 5.0 && r.ent == 0u);
    r = os_decode(os_best_serial(sets, scores, 0, 6, 0x4));
    CHECK(r.b == -1.0 && r.ent == 2u);
    r = os_decode(os_best_serial(sets, scores, 1, 6, 0x0));
    CHECK(r.b == -3.0 && r.ent == 0u);  // the index counts from the list's begin
    r = os_decode(os_best_serial(sets, scores, 2, 4, 0x2));
    CHECK(r.b == -kInf && r.ent == kSearchNoEntry);
    r = os_decode(os_best_serial(sets, scores, 5, 6, 1ull << 62));
    CHECK(r.b == 9.0 && r.ent == 0u);
    const uint64_t zs[2] = {0, 0};
    const float zv[2] = {-0.0f, 0.0f};
    r = os_decode(os_best_serial(zs, zv, 0, 2, 0));
    CHECK(r.b == 0.0 && !std::signbit(r.b) && r.ent == 0u);
    CHECK(os_tabu(5, 9, 4) && !os_tabu(5, 10, 4) && !os_tabu(0, 1, 1 << 20) && !os_tabu(8, 9, 0));
    CHECK(os_admissible(-1.0, false, 0, 0) && !os_admissible(-kInf, false, 0, 0) && !os_admissible(1.0, true, -5.0, -4.0) &&
          os_admissible(1.5, true, -5.0, -4.0));
}

struct Lists {
    int n;
    std::vector<int64_t> offsets;
    std::vector<uint64_t> sets;
    std::vector<float> scores;
    OsHostLists view() const { return OsHostLists{n, offsets.data(), sets.data(), scores.data()}; }
};

// rooted: variable 0 has no empty set
Lists random_lists(int n, int per_var, bool rooted) {
    Lists L;
    L.n = n;
    L.offsets.push_back(0);
    for (int v = 0; v < n; ++v) {
        std::vector<uint64_t> mine;
        if (!(rooted && v == 0)) mine.push_back(0);
        for (int k = 0; k < per_var; ++k) {
            uint64_t P = (1ull << (rnd() % n)) | (1ull << (rnd() % n));
            P &= ~(1ull << v);
            bool dup = P == 0;
            for (uint64_t Q : mine) dup = dup || Q == P;
            if (!dup) mine.push_back(P);
        }
        for (uint64_t P : mine) {
            L.sets.push_back(P);
            L.scores.push_back(-(float)(rnd() % 64) * 0.5f);  // a coarse grid: ties
        }
        L.offsets.push_back((int64_t)L.sets.size());
    }
    return L;
}

// One search as the kernel keeps it
struct Search {
    const Lists &L;
    int n;
    std::vector<uint8_t> ord, bord;
    std::vector<double> term, c0, c1;
    std::vector<uint32_t> stamp;
    double S = 0, S_best = 0;
    int64_t t = 0, idle = 0, tenure, patience;
    uint64_t seed;

    Search(const Lists &l, uint64_t sd, int64_t ten, int64_t pat) : L(l), n(l.n), tenure(ten), patience(pat), seed(sd) {
        ord.resize(n);
        mcmc_shuffle(seed, 0, n, ord.data());
    }
    uint64_t pre(int p) const {
        uint64_t U = 0;
        for (int q = 0; q < p; ++q) U |= 1ull << ord[q];
        return U;
    }
    void side(int q, double &a, double &b) const {
        const int x = ord[q], y = ord[q + 1];
        a = os_term_serial(L.view(), y, pre(q)).b;
        b = os_term_serial(L.view(), x, pre(q) | (1ull << y)).b;
    }
    bool full() {  // false: a term of -inf
        term.assign(n, 0), c0.assign(n, 0), c1.assign(n, 0);
        bool ok = true;
        for (int p = 0; p < n; ++p) ok = (term[p] = os_term_serial(L.view(), ord[p], pre(p)).b) > -kInf && ok;
        for (int q = 0; q + 1 < n; ++q) side(q, c0[q], c1[q]);
        return ok;
    }
    double sum() const {
        double s = 0;
        for (double x : term) s += x;
        return s;
    }
    uint32_t &stamp_of(int x, int y) { return stamp[(x < y ? x : y) * n + (x < y ? y : x)]; }
    void step() {
        ++t;
        int p = -1;
        double g = -kInf;
        for (int q = 0; q + 1 < n; ++q) {
            const double gq = os_gain(c0[q], c1[q], term[q], term[q + 1]);
            double f0, f1;  // ... against the lists
            side(q, f0, f1);
            CHECK(f0 == c0[q] && f1 == c1[q]);
            if (os_admissible(gq, os_tabu(stamp_of(ord[q], ord[q + 1]), t, tenure), S, S_best) &&
                (p < 0 || os_double_image(gq) > os_double_image(g)))
                p = q, g = gq;
        }
        if (p >= 0) {
            std::swap(term[p], c0[p]);
            std::swap(term[p + 1], c1[p]);
            stamp_of(ord[p], ord[p + 1]) = (uint32_t)t;
            std::swap(ord[p], ord[p + 1]);
            if (p >= 1) side(p - 1, c0[p - 1], c1[p - 1]);
            if (p + 2 < n) side(p + 1, c0[p + 1], c1[p + 1]);
            S = S + g;
        }
        for (int q = 0; q < n; ++q) CHECK(term[q] == os_term_serial(L.view(), ord[q], pre(q)).b && term[q] > -kInf);
        CHECK(std::fabs(S - sum()) <= 1e-9);
        if (S > S_best) S_best = S, idle = 0, bord = ord;
        else ++idle;
    }
};

int g_undone = 0, g_kicked = 0;

void check_search(int n, bool rooted, int64_t tenure) {
    const Lists L = random_lists(n, 5, rooted);
    for (uint64_t seed = 1; seed <= 6; ++seed) {
        Search s(L, seed, tenure, 5);
        s.stamp.assign((size_t)n * n, 0);
        if (!s.full()) continue;  // a begin would refuse it
        s.S = s.S_best = s.sum();
        s.bord = s.ord;
        for (int k = 0; k < 60; ++k) {
            s.step();
            if (s.idle < s.patience) continue;
            const std::vector<double> best_terms = [&] {
                Search b(s);
                b.ord = b.bord;
                b.full();
                return b.term;
            }();
            s.ord = s.bord;
            os_kick(s.seed, (uint64_t)s.t, 0, n, s.ord.data());
            uint64_t seen = 0;
            for (int p = 0; p < n; ++p) seen |= 1ull << s.ord[p];
            CHECK(seen == (1ull << n) - 1);
            const bool ok = s.full();
            if (!ok) {
                s.ord = s.bord;
                CHECK(s.full() && s.term == best_terms);
                ++g_undone;
            } else {
                ++g_kicked;
            }
            s.stamp.assign((size_t)n * n, 0);
            s.S = s.sum(), s.idle = 0;
            if (ok) {
                if (s.S > s.S_best) s.S_best = s.S, s.bord = s.ord;
                else s.idle = 1;
            }
        }
    }
}

}  // namespace

int main() {
    check_images();
    for (int n = 2; n <= 9; ++n)
        for (int rooted = 0; rooted < 2; ++rooted)
            for (int64_t tenure : {0, 3, 1 << 20}) check_search(n, rooted != 0, tenure);
    CHECK(g_undone > 0 && g_kicked > 0);
    CHECK(os_kick_count(3) == 2 && os_kick_count(8) == 2 && os_kick_count(12) == 3 && os_kick_count(63) == 15);
    std::printf("order_search_check ok: %ld checks, %d kicks, %d undone\n", g_checks, g_kicked, g_undone);
    return 0;
}
