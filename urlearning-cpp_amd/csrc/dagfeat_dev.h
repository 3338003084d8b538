// dagfeat_dev.h -- the rules of ulg_dag_features (dagfeat.hip): what one
// variable's row of a DAG becomes -- its ancestors, its Markov blanket, its
// v-structures, its compelled parents in the essential graph -- stated over
// "my row" and an accessor for another variable's row.  On the device a row
// lives in a lane of a wave64 and the accessor is a cross-lane read
// (dagfeat.hip, DfWaveLane); on the host the rows are arrays (DfHostLane
// below) and host/dagfeat_check.cpp runs the same functions against a brute
// force.  Host and device: it compiles under hipcc and a plain C++ compiler.
//
// A row is a uint64 mask over the variables 0 .. n-1, n <= 63.  Of variable v:
//   pa   its parents             ch   its children (the transpose of pa)
//   adj  pa | ch                 anc  its ancestors (closure of pa)
//   D    its compelled parents   Dch  its compelled children (transpose of D)
//   U    adj & ~D & ~Dch: the neighbours whose edge is still undirected
//
// The accessor W of a lane:
//   W::Var         what names "this quantity of every variable": the lane's own
//                  register on the device, the array on the host
//   w.lane         the variable of this lane
//   w.own(x)       my row of x
//   w.row(x, k)    row k of x; k is the same in every lane (wave-uniform)
//   w.any(p)       p of some lane (device: a ballot); the host's lanes run one
//                  after the other and answer p: any() only ever skips work
//                  that changes nothing for a lane whose p is false
// Every loop below runs over a wave-uniform mask, so that the lanes of a wave
// stay together and row() is a read of a uniform lane.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ULG_DF_HD __host__ __device__ __forceinline__
#else
#define ULG_DF_HD inline
#endif

namespace ulg {

constexpr int kDagfeatMaxVars = 63;  // a row and the own bit's lane fit a wave64; bit 63 stays free
// The four n x n tables of uint64 are accumulated in the workgroup's LDS up to
// this n (4 * 45^2 * 8 = 64,800 bytes <= 64 KB) and by global atomics above it
constexpr int kDagfeatLdsMaxVars = 45;
constexpr int kDagfeatTables = 4;  // edge, ancestor, blanket, compelled: the n x n ones, in this order

ULG_DF_HD uint64_t df_bit(int v) { return 1ull << v; }
ULG_DF_HD int df_ctz(uint64_t x) { return __builtin_ctzll(x); }

// ---- ancestors: one Warshall pass, step k = 0 .. n-1 in turn over every row at once.
// anc starts as pa; a row that holds k takes row k in.  After step n-1 a row
// holds its own bit iff its variable lies on a directed cycle.
ULG_DF_HD uint64_t df_closure_step(uint64_t anc_v, uint64_t anc_k, int k) { return ((anc_v >> k) & 1ull) ? (anc_v | anc_k) : anc_v; }

// ---- Markov blanket: parents, children and the children's other parents.
// has_pa: the variables with a parent (any superset of them does).
template <class W>
ULG_DF_HD uint64_t df_blanket(const W &w, typename W::Var pa, typename W::Var ch, uint64_t has_pa) {
    const uint64_t my_ch = w.own(ch);
    uint64_t b = w.own(pa) | my_ch;
    for (uint64_t m = has_pa; m; m &= m - 1) {
        const int c = df_ctz(m);
        const uint64_t pa_c = w.row(pa, c);
        if ((my_ch >> c) & 1ull) b |= pa_c;
    }
    return b & ~df_bit(w.lane);
}

// ---- v-structures at v through its parent u: the parents w of v that are not
// adjacent to u.  u -> v <- w is counted once, at w > u (df_above).
ULG_DF_HD uint64_t df_vs_partners(uint64_t pa_v, uint64_t adj_u, int u) { return pa_v & ~adj_u & ~df_bit(u); }
ULG_DF_HD uint64_t df_above(int u) { return ~((2ull << u) - 1ull); }  // u <= 62

// The essential graph's start: the parents of v that take part in a
// v-structure at v.  has_ch: the variables with a child (or a superset).
template <class W>
ULG_DF_HD uint64_t df_vs_parents(const W &w, typename W::Var pa, typename W::Var adj, uint64_t has_ch) {
    const uint64_t my_pa = w.own(pa);
    uint64_t d = 0;
    for (uint64_t m = has_ch; m; m &= m - 1) {
        const int u = df_ctz(m);
        const uint64_t adj_u = w.row(adj, u);
        if (((my_pa >> u) & 1ull) && df_vs_partners(my_pa, adj_u, u)) d |= df_bit(u);
    }
    return d;
}

// ---- Meek's rules R1-R3, one pass for lane c over the state as the pass found
// it: the neighbours a in U[c] that the rules orient a -> c.
//   R1  some x -> a compelled with x, c not adjacent:   D[a] & ~adj[c] & ~bit(c)
//   R2  a -> k -> c compelled:                          Dch[a] & D[c]
//   R3  a - k1, a - k2, k1 -> c <- k2 compelled, k1, k2 not adjacent:
//       X = U[a] & D[c] has a member k with X & ~adj[k] & ~bit(k) != 0
// active: the variables with an undirected edge (a superset does).  The caller
// ORs the result into D, transposes it into Dch, takes both out of U, and
// repeats until no lane adds anything.  The rules only ever add, and what a
// rule needs stays true once it is, so the closure is the least fixpoint of a
// monotone operator: unique, whatever the order or grouping of the firings.
template <class W>
ULG_DF_HD uint64_t df_meek_pass(const W &w, typename W::Var D, typename W::Var Dch, typename W::Var U, typename W::Var adj,
                                uint64_t active) {
    const uint64_t D_c = w.own(D), U_c = w.own(U), not_adj_c = ~w.own(adj) & ~df_bit(w.lane);
    uint64_t add = 0;
    for (uint64_t m = active; m; m &= m - 1) {
        const int a = df_ctz(m);
        const uint64_t D_a = w.row(D, a), Dch_a = w.row(Dch, a), U_a = w.row(U, a);
        const bool mine = ((U_c >> a) & 1ull) != 0;
        bool hit = mine && ((D_a & not_adj_c) != 0 || (Dch_a & D_c) != 0);
        const uint64_t X = U_a & D_c;
        const bool open = mine && !hit && (X & (X - 1)) != 0;  // R3 needs two members
        if (w.any(open))
            for (uint64_t mk = U_a; mk; mk &= mk - 1) {
                const int k = df_ctz(mk);
                const uint64_t adj_k = w.row(adj, k);
                if (open && ((X >> k) & 1ull) && (X & ~adj_k & ~df_bit(k))) hit = true;
            }
        if (hit) add |= df_bit(a);
    }
    return add;
}

// The host's lane: rows in arrays.
struct DfHostLane {
    using Var = const uint64_t *;
    int lane;
    uint64_t own(Var x) const { return x[lane]; }
    uint64_t row(Var x, int k) const { return x[k]; }
    bool any(bool p) const { return p; }
};

}  // namespace ulg
