// dagfeat.hip -- structural features of a batch of DAGs as exact integer sums
// (ulg_dag_features; contract: include/ulg.h): edges, directed paths, Markov
// blankets, compelled edges of the essential graph and v-structures, each
// weighted by the DAG's integer weight and summed over the acyclic graphs.
//
//   dagfeat_kernel<lds>  one wave64 per DAG, lane v holding row v (dagfeat_dev.h
//                        states the rules); a persistent grid, wave w of W
//                        taking DAGs w, w + W, ...
// A lane loads its parent mask with one 8-byte load; every other row is read
// across lanes: v_readlane of a wave-uniform index for row k, a ballot for a
// transpose (children out of parents, compelled children out of compelled
// parents).  The graph never touches LDS.  Per DAG: n ballots for the
// children, n Warshall steps for the ancestors (a set own bit = a cycle: the
// wave counts the graph and adds nothing), then loops over the variables that
// have a child (v-structures, the start of the essential graph), that have a
// parent (blanket), and per Meek pass over the variables that still have an
// undirected edge.
// Accumulation is integer: every lane adds the DAG's weight to the entries
// [u * n + v] of its row's members u.  Up to n = kDagfeatLdsMaxVars the four
// n x n tables live in the workgroup's LDS (ds_add_u64) and each workgroup
// flushes its nonzero entries once by global 64-bit atomic adds; above it the
// lanes add to global memory directly.  The n^3 v-structure table is sparse
// and always takes global atomics.  Integer adds commute, so the sums do not
// depend on the grid, the batching or the order of the atomics.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "dagfeat_dev.h"
#include "ulg_internal.h"

using namespace ulg;

namespace {

constexpr int kB = 256;                  // four waves
constexpr int kWaves = kB / 64;
constexpr int64_t kDefaultGrid = 2048;   // 8 workgroups on each of 256 CUs
constexpr size_t kChunkBytes = 1u << 28;  // parent masks uploaded per launch

enum : unsigned { kWantEdge = 1, kWantAnc = 2, kWantBlanket = 4, kWantCompelled = 8, kWantVs = 16 };

typedef unsigned long long u64;

__device__ __forceinline__ uint64_t df_readlane(uint64_t x, int k) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), k);
    return ((uint64_t)hi << 32) | lo;
}

// The device's lane: a row is the lane's own register, row k a v_readlane.
struct DfWaveLane {
    using Var = uint64_t;
    int lane;
    __device__ __forceinline__ uint64_t own(Var x) const { return x; }
    __device__ __forceinline__ uint64_t row(Var x, int k) const { return df_readlane(x, k); }
    __device__ __forceinline__ bool any(bool p) const { return __ballot(p) != 0ull; }
};

// out[u] = the lanes v whose x holds u, for the u of `over` (wave-uniform); the other lanes keep `init`
__device__ __forceinline__ uint64_t df_transpose(uint64_t x, uint64_t over, int lane, uint64_t init) {
    uint64_t out = init;
    for (uint64_t m = over; m; m &= m - 1) {
        const int u = df_ctz(m);
        const uint64_t b = __ballot((x >> u) & 1ull);
        if (lane == u) out |= b;
    }
    return out;
}

// q into the entries [u * n + v] of row's members u
__device__ __forceinline__ void df_add_row(u64 *tab, int n, int v, uint64_t row, u64 q) {
    for (; row; row &= row - 1) atomicAdd(&tab[df_ctz(row) * n + v], q);
}

// out: kDagfeatTables tables of n * n, the v-structure table of n^3, total, cyclic
template <bool kLds>
__global__ void __launch_bounds__(kB) dagfeat_kernel(const uint64_t *__restrict__ parents, const uint64_t *__restrict__ weight, int n,
                                                     int64_t count, unsigned want, u64 *out) {
    extern __shared__ u64 lds_tab[];
    const int nn = n * n;
    if (kLds) {
        for (int i = threadIdx.x; i < kDagfeatTables * nn; i += kB) lds_tab[i] = 0;
        __syncthreads();
    }
    u64 *tab = kLds ? lds_tab : out;
    u64 *vs = out + (size_t)kDagfeatTables * nn;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const DfWaveLane w{lane};
    const uint64_t all = (1ull << n) - 1ull;
    u64 total = 0, cyclic = 0;
    for (int64_t k = (int64_t)blockIdx.x * kWaves + wave; k < count; k += (int64_t)gridDim.x * kWaves) {
        const uint64_t pa = lane < n ? parents[k * n + lane] : 0ull;
        const u64 q = weight ? weight[k] : 1ull;
        uint64_t anc = pa;
        for (int s = 0; s < n; ++s) anc = df_closure_step(anc, df_readlane(anc, s), s);
        if (__ballot((anc >> lane) & 1ull)) {  // a directed cycle: counted, adds nothing
            ++cyclic;
            continue;
        }
        total += q;
        if (q == 0) continue;
        const uint64_t has_pa = __ballot(pa != 0);
        const uint64_t ch = df_transpose(pa, all, lane, 0ull);
        const uint64_t has_ch = __ballot(ch != 0);
        const uint64_t adj = pa | ch;
        if (lane < n) {
            if (want & kWantEdge) df_add_row(tab, n, lane, pa, q);
            if (want & kWantAnc) df_add_row(tab + nn, n, lane, anc, q);
        }
        if (want & kWantBlanket) {
            const uint64_t bl = df_blanket(w, pa, ch, has_pa);
            if (lane < n) df_add_row(tab + 2 * nn, n, lane, bl, q);
        }
        if (want & kWantVs)
            for (uint64_t m = has_ch; m; m &= m - 1) {
                const int u = df_ctz(m);
                const uint64_t adj_u = df_readlane(adj, u);
                if ((pa >> u) & 1ull)
                    for (uint64_t x = df_vs_partners(pa, adj_u, u) & df_above(u); x; x &= x - 1)
                        atomicAdd(&vs[((size_t)lane * n + u) * n + df_ctz(x)], q);
            }
        if (want & kWantCompelled) {
            uint64_t D = df_vs_parents(w, pa, adj, has_ch);
            uint64_t Dch = df_transpose(D, has_ch, lane, 0ull);
            uint64_t U = adj & ~D & ~Dch;
            if (__ballot(D != 0))  // without a v-structure no rule ever fires
                for (;;) {
                    const uint64_t active = __ballot(U != 0);
                    const uint64_t add = df_meek_pass(w, D, Dch, U, adj, active);
                    if (!__ballot(add != 0)) break;
                    D |= add;
                    Dch = df_transpose(add, active, lane, Dch);
                    U = adj & ~D & ~Dch;
                }
            if (lane < n) df_add_row(tab + 3 * nn, n, lane, D, q);
        }
    }
    if (lane == 0) {
        if (total) atomicAdd(&vs[(size_t)nn * n], total);
        if (cyclic) atomicAdd(&vs[(size_t)nn * n + 1], cyclic);
    }
    if (kLds) {
        __syncthreads();
        for (int i = threadIdx.x; i < kDagfeatTables * nn; i += kB) {
            const u64 x = lds_tab[i];
            if (x) atomicAdd(&out[i], x);
        }
    }
}

}  // namespace

extern "C" {

int ulg_dag_features(ulg_ctx *c, int n, int64_t count, const uint64_t *parents, const uint64_t *weight, uint64_t *edge,
                     uint64_t *ancestor, uint64_t *blanket, uint64_t *compelled, uint64_t *vstruct, uint64_t *total,
                     int64_t *cyclic) {
    if (!c) return ULG_ERR_ARG;
    const char *who = "ulg_dag_features";
    if (n < 1) return set_err(c, ULG_ERR_ARG, std::string(who) + ": n < 1");
    char buf[256];
    if (n > kDagfeatMaxVars) {
        std::snprintf(buf, sizeof buf, "%s: n = %d; at most %d variables", who, n, kDagfeatMaxVars);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    if (count < 0) return set_err(c, ULG_ERR_ARG, std::string(who) + ": negative count");
    if ((count > 0 && !parents) || !total) return set_err(c, ULG_ERR_ARG, std::string(who) + ": bad arguments");
    // every mask and the weight sum, before any device work
    const uint64_t outside = ~((1ull << n) - 1ull);
    for (int64_t k = 0; k < count; ++k)
        for (int v = 0; v < n; ++v) {
            const uint64_t m = parents[(size_t)k * n + v];
            if ((m & outside) || ((m >> v) & 1ull)) {
                std::snprintf(buf, sizeof buf, "%s: DAG %lld, variable %d: a parent mask with %s", who, (long long)k, v,
                              (m & outside) ? "a bit >= n" : "the variable's own bit");
                return set_err(c, ULG_ERR_ARG, buf);
            }
        }
    constexpr uint64_t kLimit = 1ull << 63;
    uint64_t sum = weight ? 0ull : (uint64_t)count;
    for (int64_t k = 0; weight && k < count; ++k) {
        if (weight[k] >= kLimit - sum) return set_err(c, ULG_ERR_ARG, std::string(who) + ": the weights sum to 2^63 or more");
        sum += weight[k];
    }
    const size_t nn = (size_t)n * n, n3 = nn * n;
    uint64_t *const tables[kDagfeatTables] = {edge, ancestor, blanket, compelled};
    c->dagfeat_grid = 0;
    if (count == 0) {  // no device work
        for (uint64_t *t : tables)
            if (t) std::fill(t, t + nn, 0ull);
        if (vstruct) std::fill(vstruct, vstruct + n3, 0ull);
        *total = 0;
        if (cyclic) *cyclic = 0;
        return ULG_OK;
    }
    unsigned want = vstruct ? kWantVs : 0u;
    for (int t = 0; t < kDagfeatTables; ++t)
        if (tables[t]) want |= 1u << t;
    ULG_HIP(c, hipSetDevice(c->device));
    // the call's own buffers: freed when it returns, on every path
    const int64_t chunk = std::min<int64_t>(count, std::max<int64_t>(1, (int64_t)(kChunkBytes / (8u * (size_t)n))));
    const size_t out_elems = kDagfeatTables * nn + n3 + 2;
    DevBuf<uint64_t> d_par, d_w, d_out;
    int rc;
    if ((rc = ensure(c, d_par, (size_t)chunk * n)) || (rc = ensure(c, d_out, out_elems)) ||
        (weight && (rc = ensure(c, d_w, (size_t)chunk))))
        return rc;
    ULG_HIP(c, hipMemsetAsync(d_out.p, 0, out_elems * sizeof(uint64_t), c->stream));
    const bool lds = n <= kDagfeatLdsMaxVars;
    for (int64_t first = 0; first < count; first += chunk) {
        const int64_t dags = std::min(chunk, count - first);
        ULG_HIP(c, hipMemcpyAsync(d_par.p, parents + (size_t)first * n, (size_t)dags * n * sizeof(uint64_t), hipMemcpyHostToDevice,
                                  c->stream));
        if (weight)
            ULG_HIP(c, hipMemcpyAsync(d_w.p, weight + first, (size_t)dags * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        const int64_t grid =
            c->opt.dagfeat_grid > 0 ? c->opt.dagfeat_grid : std::min<int64_t>(kDefaultGrid, (dags + kWaves - 1) / kWaves);
        if (first == 0) c->dagfeat_grid = grid;
        prof_begin(c, "dagfeat");
        if (lds)
            dagfeat_kernel<true><<<dim3((unsigned)grid), kB, kDagfeatTables * nn * sizeof(u64), c->stream>>>(
                d_par.p, weight ? d_w.p : nullptr, n, dags, want, (u64 *)d_out.p);
        else
            dagfeat_kernel<false><<<dim3((unsigned)grid), kB, 0, c->stream>>>(d_par.p, weight ? d_w.p : nullptr, n, dags, want,
                                                                               (u64 *)d_out.p);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
        // the next chunk's copies overwrite what this launch reads: the stream orders them
    }
    std::vector<uint64_t> h_out;
    try {
        h_out.resize(out_elems);
    } catch (const std::exception &) {
        return set_err(c, ULG_ERR_UNSUPPORTED, std::string(who) + ": the tables do not fit the host memory");
    }
    // everything when the n^3 table is wanted; else the n x n tables and the two scalars after the n^3 table
    const size_t head = vstruct ? out_elems : kDagfeatTables * nn, tail = kDagfeatTables * nn + n3;
    ULG_HIP(c, hipMemcpyAsync(h_out.data(), d_out.p, head * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (!vstruct)
        ULG_HIP(c, hipMemcpyAsync(h_out.data() + tail, d_out.p + tail, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (int t = 0; t < kDagfeatTables; ++t)
        if (tables[t]) std::copy(h_out.begin() + t * nn, h_out.begin() + (t + 1) * nn, tables[t]);
    if (vstruct) std::copy(h_out.begin() + kDagfeatTables * nn, h_out.begin() + kDagfeatTables * nn + n3, vstruct);
    *total = h_out[kDagfeatTables * nn + n3];
    if (cyclic) *cyclic = (int64_t)h_out[kDagfeatTables * nn + n3 + 1];
    return ULG_OK;
}

}  // extern "C"
