// dagfeat_check -- the host side of csrc/dagfeat_dev.h, the rules of
// ulg_dag_features: the same closure step, blanket, v-structure and Meek-pass
// functions that the lanes of csrc/dagfeat.hip run, here over arrays
// (DfHostLane), in the kernel's own sequence, against a brute force inside
// this program:
//   ancestors     reachability by search
//   blanket       parents, children, the children's parents, by loops
//   v-structures  every pair of non-adjacent parents
//   compelled     n <= 4: the definition -- the same direction in every DAG
//                 with the same skeleton and v-structures, over all DAGs;
//                 larger n: Meek's R1-R3 on adjacency matrices, edge by edge
// for all DAGs of n <= 4 (1, 3, 25, 543), random ones up to n = 63, and the
// structured graphs whose answers are known in closed form.
// Built with AddressSanitizer + UBSan by `make sanitize` (tests/test_dagfeat_ref.py).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../csrc/dagfeat_dev.h"

using namespace ulg;

namespace {

long g_checks = 0;

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        ++g_checks;                                                                            \
        if (!(cond)) {                                                                         \
            std::fprintf(stderr, "dagfeat_check: %s:%d: %s fails\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                      \
        }                                                                                      \
    } while (0)

typedef std::vector<uint64_t> Rows;

struct Features {
    bool cyclic = false;
    Rows anc, blanket, compelled;
    std::vector<int> vs;  // (v * n + u) * n + w, ascending
    int passes = 0;       // Meek passes that added something
};

Rows transpose(int n, const Rows &x) {
    Rows out(n, 0);
    for (int v = 0; v < n; ++v)
        for (int u = 0; u < n; ++u)
            if ((x[v] >> u) & 1ull) out[u] |= df_bit(v);
    return out;
}

uint64_t nonzero(int n, const Rows &x) {
    uint64_t m = 0;
    for (int v = 0; v < n; ++v)
        if (x[v]) m |= df_bit(v);
    return m;
}

// dagfeat_kernel's sequence for one DAG, a lane after the other
Features rules(int n, const Rows &pa) {
    Features f;
    f.anc = pa;
    for (int s = 0; s < n; ++s) {
        const uint64_t row = f.anc[s];
        for (int v = 0; v < n; ++v) f.anc[v] = df_closure_step(f.anc[v], row, s);
    }
    for (int v = 0; v < n; ++v) f.cyclic = f.cyclic || ((f.anc[v] >> v) & 1ull);
    if (f.cyclic) return f;
    const Rows ch = transpose(n, pa);
    Rows adj(n);
    for (int v = 0; v < n; ++v) adj[v] = pa[v] | ch[v];
    const uint64_t has_pa = nonzero(n, pa), has_ch = nonzero(n, ch);
    f.blanket.resize(n);
    Rows D(n);
    for (int v = 0; v < n; ++v) {
        const DfHostLane w{v};
        f.blanket[v] = df_blanket(w, pa.data(), ch.data(), has_pa);
        for (uint64_t m = has_ch; m; m &= m - 1) {
            const int u = df_ctz(m);
            if ((pa[v] >> u) & 1ull)
                for (uint64_t x = df_vs_partners(pa[v], adj[u], u) & df_above(u); x; x &= x - 1)
                    f.vs.push_back((v * n + u) * n + df_ctz(x));
        }
        D[v] = df_vs_parents(w, pa.data(), adj.data(), has_ch);
    }
    Rows Dch = transpose(n, D), U(n), add(n);
    for (;;) {
        for (int v = 0; v < n; ++v) U[v] = adj[v] & ~D[v] & ~Dch[v];
        const uint64_t active = nonzero(n, U);
        bool any = false;
        for (int v = 0; v < n; ++v) {
            add[v] = df_meek_pass(DfHostLane{v}, D.data(), Dch.data(), U.data(), adj.data(), active);
            any = any || add[v];
        }
        if (!any) break;
        ++f.passes;
        for (int v = 0; v < n; ++v) D[v] |= add[v];
        Dch = transpose(n, D);
    }
    f.compelled = D;
    return f;
}

// ---- the brute force
bool adjacent(const Rows &pa, int a, int b) { return ((pa[a] >> b) & 1ull) || ((pa[b] >> a) & 1ull); }

Rows brute_anc(int n, const Rows &pa) {
    Rows anc(n, 0);
    for (int v = 0; v < n; ++v) {
        std::vector<int> stack;
        for (int u = 0; u < n; ++u)
            if ((pa[v] >> u) & 1ull) stack.push_back(u);
        while (!stack.empty()) {
            const int u = stack.back();
            stack.pop_back();
            if ((anc[v] >> u) & 1ull) continue;
            anc[v] |= df_bit(u);
            for (int x = 0; x < n; ++x)
                if ((pa[u] >> x) & 1ull) stack.push_back(x);
        }
    }
    return anc;
}

Rows brute_blanket(int n, const Rows &pa) {
    Rows b(n, 0);
    for (int v = 0; v < n; ++v)
        for (int u = 0; u < n; ++u) {
            if (u == v) continue;
            bool in = adjacent(pa, u, v);
            for (int c = 0; c < n && !in; ++c) in = ((pa[c] >> v) & 1ull) && ((pa[c] >> u) & 1ull);
            if (in) b[v] |= df_bit(u);
        }
    return b;
}

std::vector<int> brute_vs(int n, const Rows &pa) {
    std::vector<int> out;
    for (int v = 0; v < n; ++v)
        for (int u = 0; u < n; ++u)
            for (int w = u + 1; w < n; ++w)
                if (((pa[v] >> u) & 1ull) && ((pa[v] >> w) & 1ull) && !adjacent(pa, u, w)) out.push_back((v * n + u) * n + w);
    return out;
}

// Meek's R1-R3 on matrices: dir[a][c] = a -> c compelled
Rows brute_meek(int n, const Rows &pa) {
    std::vector<std::vector<char>> dir(n, std::vector<char>(n, 0));
    for (int code : brute_vs(n, pa)) {
        const int w = code % n, u = code / n % n, v = code / n / n;
        dir[u][v] = dir[w][v] = 1;
    }
    auto und = [&](int a, int b) { return adjacent(pa, a, b) && !dir[a][b] && !dir[b][a]; };
    for (bool changed = true; changed;) {
        changed = false;
        for (int a = 0; a < n; ++a)
            for (int c = 0; c < n; ++c) {
                if (a == c || !und(a, c)) continue;
                bool hit = false;
                for (int x = 0; x < n && !hit; ++x) {
                    if (x == a || x == c) continue;
                    hit = (dir[x][a] && !adjacent(pa, x, c)) || (dir[a][x] && dir[x][c]);
                    for (int y = x + 1; y < n && !hit; ++y)
                        hit = y != a && y != c && und(a, x) && und(a, y) && dir[x][c] && dir[y][c] && !adjacent(pa, x, y);
                }
                if (hit) {
                    CHECK((pa[c] >> a) & 1ull);  // never against the DAG
                    dir[a][c] = 1;
                    changed = true;
                }
            }
    }
    Rows D(n, 0);
    for (int a = 0; a < n; ++a)
        for (int c = 0; c < n; ++c)
            if (dir[a][c]) D[c] |= df_bit(a);
    return D;
}

void check_against_brute(int n, const Rows &pa, bool meek) {
    const Features f = rules(n, pa);
    const Rows anc = brute_anc(n, pa);
    bool cyc = false;
    for (int v = 0; v < n; ++v) cyc = cyc || ((anc[v] >> v) & 1ull);
    CHECK(f.cyclic == cyc);
    if (cyc) return;
    CHECK(f.anc == anc);
    CHECK(f.blanket == brute_blanket(n, pa));
    CHECK(f.vs == brute_vs(n, pa));
    if (meek) CHECK(f.compelled == brute_meek(n, pa));
    for (int v = 0; v < n; ++v) CHECK((f.compelled[v] & ~pa[v]) == 0);
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// a random order; each earlier variable a parent with probability num / 8, at most max_pa of them
Rows random_dag(int n, unsigned num, int max_pa) {
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(order[i], order[rnd() % (uint64_t)(i + 1)]);
    Rows pa(n, 0);
    for (int i = 0; i < n; ++i)
        for (int j = 0, have = 0; j < i && have < max_pa; ++j)
            if (rnd() % 8 < num) pa[order[i]] |= df_bit(order[j]), ++have;
    return pa;
}

int popcount(const Rows &x) {
    int c = 0;
    for (uint64_t r : x) c += __builtin_popcountll(r);
    return c;
}

}  // namespace

int main() {
    CHECK(df_above(0) == ~1ull && df_above(62) == 1ull << 63 && df_vs_partners(0b1011, 0b0010, 0) == 0b1000);
    CHECK(4 * kDagfeatLdsMaxVars * kDagfeatLdsMaxVars * 8 <= 65536 && 4 * (kDagfeatLdsMaxVars + 1) * (kDagfeatLdsMaxVars + 1) * 8 > 65536);
    // ---- every graph of n <= 4 (cyclic ones included): the brute force; and the compelled edges of
    // every DAG against the definition by classes
    const long want_dags[5] = {0, 1, 3, 25, 543}, want_classes[5] = {0, 1, 2, 11, 185};
    for (int n = 1; n <= 4; ++n) {
        std::map<std::pair<Rows, std::vector<int>>, std::vector<Rows>> classes;  // (skeleton, v-structures) -> members
        std::vector<Rows> dags;
        const uint64_t per = 1ull << (n - 1);
        uint64_t graphs = 1;
        for (int v = 0; v < n; ++v) graphs *= per;
        for (uint64_t code = 0; code < graphs; ++code) {
            Rows pa(n);
            uint64_t rest = code;
            for (int v = 0; v < n; ++v, rest /= per) {
                const uint64_t x = rest % per, low = x & (df_bit(v) - 1ull);  // the own bit spliced out
                pa[v] = low | ((x ^ low) << 1);
            }
            check_against_brute(n, pa, true);
            const Features f = rules(n, pa);
            if (f.cyclic) continue;
            Rows skel(n);
            const Rows ch = transpose(n, pa);
            for (int v = 0; v < n; ++v) skel[v] = pa[v] | ch[v];
            classes[{skel, f.vs}].push_back(pa);
            dags.push_back(pa);
        }
        CHECK((long)dags.size() == want_dags[n] && (long)classes.size() == want_classes[n]);
        for (const auto &cls : classes) {
            Rows common(n, ~0ull);
            for (const Rows &pa : cls.second)
                for (int v = 0; v < n; ++v) common[v] &= pa[v];
            for (const Rows &pa : cls.second) CHECK(rules(n, pa).compelled == common);
        }
    }
    // ---- random DAGs up to n = 63, sparse and dense
    for (int n : {5, 6, 7, 12, 27, 31, 32, 33, 45, 46, 62, 63})
        for (int rep = 0; rep < 6; ++rep) {
            check_against_brute(n, random_dag(n, rep % 2 ? 4 : 2, rep % 2 ? n : 2), n <= 33 || rep < 2);
            check_against_brute(n, random_dag(n, 1 + rep, 3), n <= 33 || rep < 2);
        }
    // ---- the structured graphs at n = 63
    {
        const int n = 63;
        Rows chain(n, 0), collider(n, 0), complete(n), star(n, 0), cyc(n);
        for (int v = 1; v < n; ++v) chain[v] = df_bit(v - 1);
        collider = chain;
        collider[1] = 0, collider[2] = 0b11;
        for (int v = 0; v < n; ++v) complete[v] = df_bit(v) - 1ull, cyc[v] = df_bit((v + n - 1) % n);
        star[n - 1] = df_bit(n - 1) - 1ull;
        Features f = rules(n, chain);
        CHECK(!f.cyclic && popcount(f.compelled) == 0 && f.vs.empty() && f.passes == 0);
        for (int v = 0; v < n; ++v) CHECK(f.anc[v] == df_bit(v) - 1ull);
        f = rules(n, collider);
        CHECK(f.compelled == collider && f.vs.size() == 1 && f.passes == 60);  // one R1 step per chain edge
        f = rules(n, complete);
        CHECK(popcount(f.compelled) == 0 && f.vs.empty() && f.anc == complete);
        for (int v = 0; v < n; ++v) CHECK(f.blanket[v] == ((df_bit(n) - 1ull) & ~df_bit(v)));
        f = rules(n, star);
        CHECK(f.compelled == star && (int)f.vs.size() == 62 * 61 / 2);
        f = rules(n, Rows(n, 0));
        CHECK(!f.cyclic && popcount(f.anc) + popcount(f.blanket) + popcount(f.compelled) == 0);
        CHECK(rules(n, cyc).cyclic && rules(2, Rows{2, 1}).cyclic);
        check_against_brute(n, collider, true);
        check_against_brute(n, star, true);
    }
    std::printf("dagfeat_check ok: %ld checks\n", g_checks);
    return 0;
}
