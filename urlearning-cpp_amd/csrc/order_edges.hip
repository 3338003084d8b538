// order_edges.hip -- Rao-Blackwellised edge posteriors of given orders over the
// lists of the order MCMC (ulg_order_edges; contract: include/ulg.h).  For
// every order and position the closed form p(u -> v | order) = N_u / T over the
// very entries the order's term scans, as g = floor(N_u / T 2^40), added into
// the order's group table with 64-bit integer adds.
//
// Kernels:
//   edges_empty_kernel    one lane per list entry: which variables list the
//                         empty set (their terms are finite under every order)
//   edges_flag_kernel     one wave per (order, position) whose variable lacks
//                         the empty set: no compatible entry marks the order
//                         (probability 0: it adds nothing anywhere)
//   edges_scatter_kernel  one wave per (order, position), workgroups striding
//                         the pairs; lane u owns N_u in registers:
//     maximum  lanes stride the list for the maximum of the compatible
//              scores, as wave_term does (order_mcmc.hip);
//     blocks   per 64 entries each lane forms its entry's q (0 when
//              incompatible), adds it to its share of T and parks it in the
//              wave's 512 B of LDS; for each u of U one ballot of "bit u of my
//              counted set" lands in lane u, which then adds the parked q of
//              its ballot's bits (one word within a block: 64 weights stay
//              below 2^58) and the block's sum into N_u (two words, lx_add);
//     ratio    T is reduced across the wave as word pairs; lane u of U forms
//              g and issues one 64-bit global integer atomic add.
// Those adds are the kernel's only atomics and are integer: no output depends
// on lanes, waves, the grid or the batching.  No scratch, every loop bounded
// by the list, the 64 bits of a mask or the pairs of the call.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "order_edges_dev.h"
#include "order_mcmc_state.h"

using namespace ulg;

namespace {

constexpr int kWave = 64;
constexpr int kB = 256;                  // four waves to a workgroup
constexpr int kWaves = kB / kWave;
constexpr int64_t kDefaultGrid = 65536;  // workgroups at most without option "edges_grid"

// blockIdx.y = the variable
__global__ void __launch_bounds__(kB) edges_empty_kernel(const uint64_t *sets, const int64_t *offsets, uint8_t *has_empty) {
    const int v = blockIdx.y;
    const int64_t b = offsets[v], e = offsets[v + 1];
    for (int64_t i = b + (int64_t)blockIdx.x * kB + threadIdx.x; i < e; i += (int64_t)gridDim.x * kB)
        if (sets[i] == 0) has_empty[v] = 1;  // at most one entry per variable: the lists hold no set twice
}

// the predecessors of position p of `ord`: a lane per position, n <= 63
__device__ __forceinline__ uint64_t wave_pred(const uint8_t *ord, int p, int lane) {
    uint64_t U = lane < p ? 1ull << ord[lane] : 0ull;
    for (int d = kWave / 2; d > 0; d >>= 1) U |= __shfl_xor((unsigned long long)U, d, kWave);
    return U;
}

__global__ void __launch_bounds__(kB) edges_flag_kernel(const uint64_t *sets, const int64_t *offsets, const uint8_t *has_empty, int n,
                                                        const uint8_t *orders, uint64_t pairs, uint8_t *dead) {
    const int lane = threadIdx.x & (kWave - 1);
    for (uint64_t pair = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); pair < pairs; pair += (uint64_t)gridDim.x * kWaves) {
        const int64_t k = (int64_t)(pair / (uint64_t)n);
        const int p = (int)(pair % (uint64_t)n);
        const uint8_t *ord = orders + k * n;
        const int v = ord[p];
        if (has_empty[v]) continue;  // the whole wave
        const uint64_t outside = ~wave_pred(ord, p, lane);
        bool some = false;
        for (int64_t i = offsets[v] + lane, e = offsets[v + 1]; i < e; i += kWave) some = some || !(sets[i] & outside);
        if (!__ballot(some) && lane == 0) dead[k] = 1;
    }
}

struct EdgeArgs {
    const uint64_t *sets;
    const float *scores;
    const int64_t *offsets;
    const uint8_t *orders;
    const uint8_t *dead;
    unsigned long long *edge;  // [groups][n][n]
    int n;
    uint64_t pairs;  // count n
    int64_t groups;
};

__global__ void __launch_bounds__(kB) edges_scatter_kernel(const EdgeArgs a) {
    __shared__ uint64_t park[kWaves][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int n = a.n;
    uint64_t *const mine = park[wave];
    for (uint64_t pair = (uint64_t)blockIdx.x * kWaves + wave; pair < a.pairs; pair += (uint64_t)gridDim.x * kWaves) {
        const int64_t k = (int64_t)(pair / (uint64_t)n);
        const int p = (int)(pair % (uint64_t)n);
        if (p == 0 || a.dead[k]) continue;  // the whole wave; position 0 has no predecessor
        const uint8_t *ord = a.orders + k * n;
        const int v = ord[p];
        const uint64_t Uv = wave_pred(ord, p, lane);
        // the same bits in every lane: held in scalar registers, so the loops over U below are the wave's
        const uint32_t Ulo = __builtin_amdgcn_readfirstlane((uint32_t)Uv), Uhi = __builtin_amdgcn_readfirstlane((uint32_t)(Uv >> 32));
        const uint64_t outside = ~(((uint64_t)Uhi << 32) | Ulo);
        const int64_t b = a.offsets[v], e = a.offsets[v + 1];
        float mx = -__builtin_huge_valf();
        for (int64_t i = b + lane; i < e; i += kWave) {
            const uint64_t S = a.sets[i];
            const float s = a.scores[i];
            if (!(S & outside)) mx = fmaxf(mx, s);
        }
        for (int d = kWave / 2; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, kWave));
        if (!(mx > -__builtin_huge_valf())) continue;  // a dead order: edges_flag_kernel has marked it
        const double m = (double)mx;
        LxCount T{0, 0}, N{0, 0};
        for (int64_t c0 = b; c0 < e; c0 += kWave) {  // wave-uniform
            const int64_t i = c0 + lane;
            uint64_t S = 0, q = 0;
            if (i < e) {
                S = a.sets[i];
                if (!(S & outside)) q = post_weight_q((double)a.scores[i] - m);
            }
            if (!q) S = 0;  // an entry of weight 0 adds nothing to any N
            T = lx_add(T, LxCount{q, 0});
            if (!__ballot(S != 0)) continue;  // no counted entry with a parent: only T moves
            mine[lane] = q;
            const uint32_t Slo = (uint32_t)S, Shi = (uint32_t)(S >> 32);
            unsigned long long got = 0;  // lane u: the entries of the block that hold u
            for (uint32_t w = Ulo; w; w &= w - 1) {
                const int u = __builtin_ctz(w);
                const unsigned long long hit = __ballot((Slo >> u) & 1u);
                if (lane == u) got = hit;
            }
            for (uint32_t w = Uhi; w; w &= w - 1) {
                const int u = __builtin_ctz(w);
                const unsigned long long hit = __ballot((Shi >> u) & 1u);
                if (lane == 32 + u) got = hit;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            uint64_t part = 0;  // 64 weights of at most 2^52 stay below 2^58: one word within a block, the carry once per block
            for (; got; got &= got - 1) part += mine[__builtin_ctzll(got)];  // at most 64 turns
            N = lx_add(N, LxCount{part, 0});
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();  // every lane has read before the next block parks
        }
        for (int d = kWave / 2; d > 0; d >>= 1) {
            LxCount o;
            o.lo = __shfl_xor((unsigned long long)T.lo, d, kWave);
            o.hi = __shfl_xor((unsigned long long)T.hi, d, kWave);
            T = lx_add(T, o);
        }
        const uint64_t g = edge_g(N, T);  // 0 for a lane outside U: its N is 0
        if (g) atomicAdd(a.edge + ((uint64_t)(k % a.groups) * n + lane) * n + v, (unsigned long long)g);
    }
}

bool is_permutation(const uint8_t *row, int n) {
    uint64_t seen = 0;
    for (int p = 0; p < n; ++p) {
        if (row[p] >= n || ((seen >> row[p]) & 1ull)) return false;
        seen |= 1ull << row[p];
    }
    return true;
}

}  // namespace

extern "C" int ulg_order_edges(ulg_ctx *c, int64_t count, const uint8_t *orders, int64_t groups, uint64_t *edge, int64_t *zero) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_edges";
    if (!c->mcmc || !c->mcmc->ready) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_mcmc_begin");
    OrderMcmcState &s = *c->mcmc;
    const int n = s.n;
    if (count < 0 || count > kEdgeMaxOrders) return set_err(c, ULG_ERR_ARG, who + ": count must be 0..2^22");
    if (groups < 1 || groups > std::max<int64_t>(count, 1)) return set_err(c, ULG_ERR_ARG, who + ": groups must be 1..max(count, 1)");
    if (!edge || (count > 0 && !orders)) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
    for (int64_t k = 0; k < count; ++k)
        if (!is_permutation(orders + k * n, n))
            return set_err(c, ULG_ERR_ARG, who + ": order " + std::to_string(k) + " is not a permutation");
    const size_t cells = (size_t)groups * (size_t)n * (size_t)n;
    if (count == 0) {
        c->edges_grid = 0;  // nothing is launched
        std::memset(edge, 0, cells * 8);
        if (zero) *zero = 0;
        return ULG_OK;
    }
    ULG_HIP(c, hipSetDevice(c->device));
    const size_t rows = (size_t)count * (size_t)n;
    {
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        // the orders and the tables, and beside them a byte per order and per variable
        const double need = (double)rows + 8.0 * (double)cells + (double)count + n + 4 * 16.0 + 256.0;
        if (need > (double)free_b) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld orders of n = %d in %lld groups need %.0f bytes of device memory, %.0f are free",
                          who.c_str(), (long long)count, n, (long long)groups, need, (double)free_b);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    // the call's own buffers, freed on every return
    DevBuf<uint8_t> d_orders, d_dead, d_empty;
    DevBuf<unsigned long long> d_edge;
    int rc;
    if ((rc = ensure(c, d_orders, rows)) || (rc = ensure(c, d_dead, (size_t)count)) || (rc = ensure(c, d_empty, (size_t)n)) ||
        (rc = ensure(c, d_edge, cells)))
        return rc;
    ULG_HIP(c, hipMemcpyAsync(d_orders.p, orders, rows, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemsetAsync(d_dead.p, 0, (size_t)count, c->stream));
    ULG_HIP(c, hipMemsetAsync(d_empty.p, 0, (size_t)n, c->stream));
    ULG_HIP(c, hipMemsetAsync(d_edge.p, 0, cells * 8, c->stream));
    int64_t longest = 1;
    for (int v = 0; v < n; ++v) longest = std::max(longest, s.offsets[v + 1] - s.offsets[v]);
    const uint64_t pairs = (uint64_t)rows;
    const int64_t grid = c->opt.edges_grid > 0 ? c->opt.edges_grid : std::min<int64_t>(kDefaultGrid, (int64_t)((pairs + kWaves - 1) / kWaves));
    c->edges_grid = grid;
    prof_begin(c, "edges_empty");
    edges_empty_kernel<<<dim3((unsigned)std::min<int64_t>((longest + kB - 1) / kB, 4096), (unsigned)n), kB, 0, c->stream>>>(
        s.d_sets.p, s.d_offsets.p, d_empty.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    prof_begin(c, "edges_flag");
    edges_flag_kernel<<<dim3((unsigned)grid), kB, 0, c->stream>>>(s.d_sets.p, s.d_offsets.p, d_empty.p, n, d_orders.p, pairs, d_dead.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    EdgeArgs a;
    a.sets = s.d_sets.p, a.scores = s.d_scores.p, a.offsets = s.d_offsets.p;
    a.orders = d_orders.p, a.dead = d_dead.p, a.edge = d_edge.p;
    a.n = n, a.pairs = pairs, a.groups = groups;
    prof_begin(c, "edges_scatter");
    edges_scatter_kernel<<<dim3((unsigned)grid), kB, 0, c->stream>>>(a);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    std::vector<uint8_t> h_dead((size_t)count);
    ULG_HIP(c, hipMemcpyAsync(edge, d_edge.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipMemcpyAsync(h_dead.data(), d_dead.p, (size_t)count, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (zero) {
        int64_t z = 0;
        for (uint8_t d : h_dead) z += d;
        *zero = z;
    }
    return ULG_OK;
}
