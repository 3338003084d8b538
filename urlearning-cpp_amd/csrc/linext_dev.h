// linext_dev.h -- the arithmetic of the linear-extension count (linext.hip,
// ulg_dag_linear_extensions): the 128-bit count as two 64-bit words and its
// add with carry, the test that decides whether v contributes a term to c(S),
// the table's (layer, colex rank) layout with the rank of S \ v, and the colex
// unranking of a layer's nodes.  Host and device: it compiles under hipcc and
// under a plain C++ compiler (host/linext_check.cpp), which also runs
// lx_count_host, the recursion itself over the same definitions.
#pragma once

#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ULG_LX_HD __host__ __device__ __forceinline__
#else
#define ULG_LX_HD inline
#endif

namespace ulg {

constexpr int kLinextMaxVars = 28;  // 28! < 2^98; a table of 2^28 counts is 2^32 bytes

// A count: lo + 2^64 hi.  16 bytes, loaded and stored as one vector access.
struct alignas(16) LxCount {
    uint64_t lo, hi;
};

// a + b mod 2^128: the carry out of the low word goes into the high one
ULG_LX_HD LxCount lx_add(LxCount a, LxCount b) {
    LxCount r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull);
    return r;
}

// Does v contribute c(S \ v) to c(S)?  v must be a member of S and every
// parent of v (par_v, without v's own bit) a member of S \ v.
ULG_LX_HD bool lx_term(uint32_t S, int v, uint32_t par_v) { return ((S >> v) & 1u) != 0u && (par_v & ~S) == 0u; }

// The binomials the ranks need, 32 bits each: bn[a * kLxBinomStride + k] =
// C(a, k) for a < 28, k < 32 (C(27, 13) = 20,058,300; 0 for k > a)
constexpr int kLxBinomStride = 32;
constexpr int kLxBinomRows = kLinextMaxVars;
constexpr int kLxBinomSize = kLxBinomRows * kLxBinomStride;

// A DAG's table holds its 2^n counts layer by layer, a layer in colex order:
// the count of the subset with l members and colex rank r is entry
// off(l) + r, off(l) = C(n, 0) + .. + C(n, l - 1).  A layer's launch then
// writes consecutive entries from consecutive lanes.  64-bit: dag 2^n + entry
// passes 2^32 entries, and 2^32 bytes already at one DAG of n = 28.
ULG_LX_HD uint64_t lx_index(uint64_t dag, int n, uint32_t off, uint32_t r) { return (dag << n) + (uint64_t)off + (uint64_t)r; }

// The subset of {0 .. n-1} with `layer` members and colex rank r < C(n, layer)
ULG_LX_HD uint32_t lx_unrank(const uint32_t *bn, int n, int layer, uint32_t r) {
    uint32_t S = 0;
    int c = n - 1;
    for (int k = layer; k >= 1; --k) {
        while (bn[c * kLxBinomStride + k] > r) --c;
        S |= 1u << c;
        r -= bn[c * kLxBinomStride + k];
        --c;
    }
    return S;
}

// The colex rank of S \ v within its layer, for the members v of S taken from
// the largest down.  With the members c_0 < .. < c_(l-1), r = sum_i C(c_i, i + 1)
// and, for v = c_j,
//   rank(S \ v) = sum_{i < j} C(c_i, i + 1) + sum_{i > j} C(c_i, i)
//               = r - hi_a + hi_b,  hi_a = sum_{i >= j} C(c_i, i + 1),  hi_b = sum_{i > j} C(c_i, i):
// the members above v move down one position.  lx_walk_step is called for
// every v = n-1 .. 0 in turn (a step for a v outside S changes nothing and its
// result means nothing), so that a wave runs one loop whatever its lanes' sets.
struct LxWalk {
    uint32_t hi_a = 0, hi_b = 0;
};
ULG_LX_HD uint32_t lx_walk_step(LxWalk &w, const uint32_t *bn, uint32_t S, uint32_t r, int v) {
    const bool in = ((S >> v) & 1u) != 0u;
    const int j = __builtin_popcount(S & ((1u << v) - 1u));  // v's position among the members
    w.hi_a += in ? bn[v * kLxBinomStride + j + 1] : 0u;
    const uint32_t rank = r - w.hi_a + w.hi_b;
    w.hi_b += in ? bn[v * kLxBinomStride + j] : 0u;
    return rank;
}

// ---- host only
// Pascal's triangle into bn[kLxBinomSize] (the device copies the same values
// out of the context's 64-bit table)
inline void lx_binom_fill(uint32_t *bn) {
    for (int a = 0; a < kLxBinomRows; ++a)
        for (int k = 0; k < kLxBinomStride; ++k)
            bn[a * kLxBinomStride + k] =
                k == 0 ? 1u : a == 0 ? 0u : bn[(a - 1) * kLxBinomStride + k - 1] + bn[(a - 1) * kLxBinomStride + k];
}

// off[l] = the first entry of layer l, l = 0 .. n + 1 (off[n + 1] = 2^n)
inline void lx_layer_offsets(int n, uint32_t *off) {
    uint64_t c = 1;  // C(n, l)
    off[0] = 0;
    for (int l = 0; l <= n; ++l) {
        off[l + 1] = off[l] + (uint32_t)c;
        c = c * (uint64_t)(n - l) / (uint64_t)(l + 1);
    }
}

// The whole recursion on the host, layer by layer over the same layout and
// helpers: ext(G) = c(V).  par[v] = the parent mask of v, n <= 28 (tests use
// small n).  table, if given, receives the 2^n counts in the layout above.
inline LxCount lx_count_host(int n, const uint32_t *par, std::vector<LxCount> *table_out = nullptr) {
    std::vector<uint32_t> bn(kLxBinomSize);
    lx_binom_fill(bn.data());
    uint32_t off[kLinextMaxVars + 2];
    lx_layer_offsets(n, off);
    std::vector<LxCount> table((size_t)1 << n);
    table[lx_index(0, n, off[0], 0)] = LxCount{1, 0};
    for (int layer = 1; layer <= n; ++layer)
        for (uint32_t r = 0; r < off[layer + 1] - off[layer]; ++r) {
            const uint32_t S = lx_unrank(bn.data(), n, layer, r);
            LxWalk w;
            LxCount acc{0, 0};
            for (int v = n - 1; v >= 0; --v) {
                const uint32_t rank = lx_walk_step(w, bn.data(), S, r, v);
                if (lx_term(S, v, par[v])) acc = lx_add(acc, table[lx_index(0, n, off[layer - 1], rank)]);
            }
            table[lx_index(0, n, off[layer], r)] = acc;
        }
    const LxCount ext = table[lx_index(0, n, off[n], 0)];
    if (table_out) table_out->swap(table);
    return ext;
}

}  // namespace ulg
