// order_mcmc.hip -- order MCMC over the per-variable lists (ulg_order_mcmc_begin,
// ulg_order_mcmc_begin_from_scores, ulg_order_mcmc_run, ulg_order_mcmc_state,
// ulg_order_score; contract: include/ulg.h).  Metropolis-Hastings over linear
// orders with the swap of two positions as the proposal; the stationary law is
// the order marginal of the model ulg_posterior sums exactly, without its
// tables: memory is the lists and O(n) per chain, so neither 35 GB nor
// n <= 28 binds.
//
// Kernels:
//   mcmc_check_lists_kernel  one lane per list entry: the set's bits, the
//                            score, and the set's slot in a hash table of the
//                            call (a second taker of a (variable, set) is a
//                            duplicate)
//   mcmc_shuffle_kernel      one lane per chain: the initial order
//   mcmc_score_kernel        one wave per (order, position): the term a_p
//                            (ulg_order_score, and every chain's terms at begin)
//   mcmc_scan_kernel         one lane per chain: the least chain with a -inf term
//   mcmc_run_kernel<W>       one workgroup of W waves per chain, the chain's
//                            order, predecessor masks and terms in LDS, all
//                            steps of the launch:
//     move      every lane forms the step's draw (wave-uniform integer work);
//     terms     wave w takes the affected positions lo + w, lo + w + W, ..;
//               its lanes stride the variable's list, once for the maximum of
//               the compatible scores, once for the integer sum of their
//               weights, reduced across the wave as (lo, hi) word pairs with
//               carry (wave_term, the device function of every path);
//     decision  after the workgroup's barrier every lane adds the new and the
//               old terms of lo .. hi in ascending order and applies
//               mcmc_accept: the same bits in every lane, no broadcast;
//     record    at t mod thin = 0: the order, the full sum of the terms and,
//               if asked, a parent set per position by the sampler's
//               scan-and-ballot pick, waves striding the positions.
// A term is an integer sum, a decision a fixed FP64 expression of terms: no
// output depends on W, on the steps per launch or on the number of chains.
// Plain vector stores only; no floating-point atomics, no communication
// between workgroups.  The host bounds a launch by option "mcmc_launch_steps"
// and loops launches over the chains' state in device memory.
// Under option "mcmc_tables" the two begins build the log-sum tables of
// order_sumtables.hip and ulg_order_mcmc_run launches its kernel instead.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "order_mcmc_dev.h"
#include "order_mcmc_run.h"
#include "order_mcmc_state.h"

namespace ulg {

void order_mcmc_delete(ulg_ctx *c) {
    partition_mcmc_delete(c);  // its chains read these lists
    order_search_delete(c);    // ... as do the searches
    delete c->mcmc;
    c->mcmc = nullptr;
}

}  // namespace ulg

using namespace ulg;

namespace {

constexpr int kWave = 64;
constexpr int kB = 256;  // the small kernels' workgroup

// blocks x threads along x stay below 2^32: larger launches spread over y
constexpr uint64_t kGridX = 1ull << 20;
inline dim3 flat_grid(uint64_t blocks) {
    return dim3((unsigned)std::min<uint64_t>(blocks, kGridX), (unsigned)((blocks + kGridX - 1) / kGridX));
}
__device__ __forceinline__ uint64_t flat_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

// ---- the lists' checks
__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// blockIdx.y = the variable.  table: `mask` + 1 >= 2 x (list entries) slots of
// 0, a power of two; a slot takes the index + 1 of the first entry that
// hashes to it, later ones walk on, so every walk ends at a free slot.
__global__ void __launch_bounds__(kB) mcmc_check_lists_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets,
                                                              int n, unsigned long long *table, uint64_t mask, unsigned int *err) {
    const int v = blockIdx.y;
    const int64_t b = offsets[v], e = offsets[v + 1];
    const uint64_t bad = ~((1ull << n) - 1ull) | (1ull << v);  // n <= 63
    for (int64_t i = b + (int64_t)blockIdx.x * kB + threadIdx.x; i < e; i += (int64_t)gridDim.x * kB) {
        const uint64_t S = sets[i];
        const float s = scores[i];
        unsigned w = 0;
        if (S & bad) w |= kErrSet;
        if (!(fabsf(s) <= 3.402823466e+38f)) w |= kErrScore;  // false for a NaN too
        if (!w) {
            uint64_t h = mix64(S ^ ((uint64_t)(v + 1) * 0x9E3779B97F4A7C15ull)) & mask;
            for (;;) {
                const unsigned long long prev = atomicCAS(&table[h], 0ull, (unsigned long long)i + 1ull);
                if (prev == 0ull) break;
                const int64_t occ = (int64_t)prev - 1;
                if (occ >= b && occ < e && sets[occ] == S) {
                    w |= kErrDup;
                    break;
                }
                h = (h + 1) & mask;
            }
        }
        if (w) atomicOr(err, w);
    }
}

__global__ void __launch_bounds__(kB) mcmc_shuffle_kernel(uint8_t *order, int64_t chains, int n, uint64_t seed) {
    const int64_t c = (int64_t)flat_block() * kB + threadIdx.x;
    if (c < chains) mcmc_shuffle(seed, (uint32_t)c, n, order + c * n);
}

// ---- the term: one wave, every lane returns the same bits
__device__ __forceinline__ double wave_term(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t U, int lane) {
    const uint64_t outside = ~U;
    float mx = -__builtin_huge_valf();
    for (int64_t i = b + lane; i < e; i += kWave) {
        const uint64_t S = sets[i];
        const float s = scores[i];
        if (!(S & outside)) mx = fmaxf(mx, s);  // float -> double is monotone: the maximum first, converted once
    }
    for (int d = kWave / 2; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, kWave));
    if (!(mx > -__builtin_huge_valf())) return neg_inf();  // scores are finite: no compatible entry
    const double m = (double)mx;
    LxCount T{0, 0};
    for (int64_t i = b + lane; i < e; i += kWave) {
        const uint64_t S = sets[i];
        const float s = scores[i];
        if (!(S & outside)) T = lx_add(T, LxCount{post_weight_q((double)s - m), 0});
    }
    for (int d = kWave / 2; d > 0; d >>= 1) {
        LxCount o;
        o.lo = __shfl_xor((unsigned long long)T.lo, d, kWave);
        o.hi = __shfl_xor((unsigned long long)T.hi, d, kWave);
        T = lx_add(T, o);
    }
    return mcmc_term(m, T);
}

// terms[k * n + p] of `count` orders: a wave per (k, p), 4 to a workgroup
__global__ void __launch_bounds__(kB) mcmc_score_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets, int n,
                                                        const uint8_t *orders, int64_t count, double *terms) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t pair = flat_block() * (kB / kWave) + (threadIdx.x >> 6);
    if (pair >= (uint64_t)count * (uint64_t)n) return;  // the whole wave
    const int64_t k = (int64_t)(pair / (uint64_t)n);
    const int p = (int)(pair % (uint64_t)n);
    const uint8_t *ord = orders + k * n;
    uint64_t U = lane < p ? 1ull << ord[lane] : 0ull;  // n <= 63: a lane per position
    for (int d = kWave / 2; d > 0; d >>= 1) U |= __shfl_xor((unsigned long long)U, d, kWave);
    const int v = ord[p];
    const double a = wave_term(sets, scores, offsets[v], offsets[v + 1], U, lane);
    if (lane == 0) terms[k * n + p] = a;
}

__global__ void __launch_bounds__(kB) mcmc_scan_kernel(const double *terms, int64_t chains, int n, unsigned int *least) {
    const int64_t c = (int64_t)flat_block() * kB + threadIdx.x;
    if (c >= chains) return;
    bool bad = false;
    for (int p = 0; p < n; ++p) bad = bad || !(terms[c * n + p] > neg_inf());
    if (bad) atomicMin(least, (unsigned int)c);
}

template <int W>
__global__ void __launch_bounds__(kWave *W) mcmc_run_kernel(const RunArgs a) {
    __shared__ uint8_t ord[kWave];       // the variable at each position
    __shared__ uint64_t pre[kWave];      // the variables before each position
    __shared__ double term[kWave], fresh[kWave];
    __shared__ double picked[kWave];     // a record's chosen scores, by variable
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int n = a.n;
    const int64_t c = (int64_t)blockIdx.x;  // chains <= 2^20
    if (tid < n) {
        ord[tid] = a.order[c * n + tid];
        term[tid] = a.terms[c * n + tid];
    }
    __syncthreads();
    if (tid < n) {
        uint64_t U = 0;
        for (int q = 0; q < tid; ++q) U |= 1ull << ord[q];
        pre[tid] = U;
    }
    unsigned long long acc = a.accepted[c];
    __syncthreads();
    for (int64_t s = 0; s < a.nsteps; ++s) {
        const int64_t t = a.t_begin + s + 1;
        double delta = neg_inf();
        bool take = false;
        if (n > 1) {
            uint32_t w[4];
            mcmc_draw(a.seed, (uint64_t)t, (uint32_t)c, 0u, w);
            const McmcMove mv = mcmc_move(w, n);
            const int lo = mv.i < mv.j ? mv.i : mv.j, hi = mv.i < mv.j ? mv.j : mv.i;
            const int va = ord[lo], vb = ord[hi];
            const uint64_t flip = (1ull << va) ^ (1ull << vb);
            for (int p = lo + wave; p <= hi; p += W) {
                const int v = p == lo ? vb : p == hi ? va : ord[p];
                const uint64_t U = p == lo ? pre[lo] : pre[p] ^ flip;
                const double x = wave_term(a.sets, a.scores, a.offsets[v], a.offsets[v + 1], U, lane);
                if (lane == 0) fresh[p] = x;
            }
            __syncthreads();
            double now = 0.0, was = 0.0;
            bool none = false;
            for (int p = lo; p <= hi; ++p) {
                const double x = fresh[p];
                none = none || !(x > neg_inf());
                now += x;
                was += term[p];
            }
            if (!none) delta = now - was;
            take = mcmc_accept(delta, mv.u_acc);
            __syncthreads();  // every lane has read the old terms
            if (take) {
                if (tid >= lo && tid <= hi) {
                    term[tid] = fresh[tid];
                    if (tid > lo) pre[tid] ^= flip;
                    if (tid == lo) ord[lo] = (uint8_t)vb;
                    if (tid == hi) ord[hi] = (uint8_t)va;
                }
                ++acc;
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int64_t at = (t - a.t_call - 1) * a.chains + c;
            if (a.t_delta) a.t_delta[at] = delta;
            if (a.t_accept) a.t_accept[at] = take ? 1 : 0;
        }
        if (t % a.thin == 0) {
            const int64_t idx = (t / a.thin - a.t_call / a.thin - 1) * a.chains + c;
            if (a.r_order && tid < n) a.r_order[idx * n + tid] = ord[tid];
            if (a.r_score && tid == 0) {
                double sum = 0.0;
                for (int p = 0; p < n; ++p) sum += term[p];
                a.r_score[idx] = sum;
            }
            if (a.r_parents) {
                for (int p = wave; p < n; p += W) {
                    uint32_t w[4];
                    mcmc_draw(a.seed, (uint64_t)t, (uint32_t)c, (uint32_t)(1 + p), w);
                    const uint64_t u_set = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
                    const int v = ord[p];
                    const int64_t e = wave_pick(a.sets, a.scores, a.offsets[v], a.offsets[v + 1], pre[p], term[p], u_set, lane);
                    if (lane == 0) {
                        if (e < 0) {
                            atomicOr(a.err, kErrPick);  // a finite term has an entry of weight 2^52 / (its list's length) at least
                            a.r_parents[idx * n + v] = 0;
                            picked[v] = 0.0;
                        } else {
                            a.r_parents[idx * n + v] = a.sets[e];
                            picked[v] = (double)a.scores[e];
                        }
                    }
                }
                __syncthreads();
                if (a.r_weight && tid == 0) {
                    double sum = 0.0;
                    for (int v = 0; v < n; ++v) sum += picked[v];
                    a.r_weight[idx] = sum;
                }
                __syncthreads();  // before the next record's picks
            }
        }
    }
    if (tid < n) {
        a.order[c * n + tid] = ord[tid];
        a.terms[c * n + tid] = term[tid];
    }
    if (tid == 0) a.accepted[c] = acc;
}

// ---- tempered ladders (ulg_order_mc3_*): one workgroup of W waves per ladder.
// LDS holds every replica's ord, pre, term and fresh by slot (1600 B each, the
// launch's dynamic LDS).  Lane r < R of EVERY wave holds rung r's scalars --
// the slot on the rung, beta, the step's move -- so a wave reads another
// rung's by readlane and nothing of it needs LDS or a barrier: an exchange
// trades two lanes' slot numbers, in every wave alike.
//   move      lane r forms rung r's draw (one Philox per wave and step, R
//             lanes busy); the spans hi - lo + 1 are prefix-summed across the
//             lanes into the ladder's item table: item q belongs to the last
//             rung whose start is <= q (a ballot), at position lo + q - start;
//   terms     wave w takes items w, w + W, ..: one wave_term each.  A rung
//             with a short span leaves its share of the waves to the others;
//             the barrier waits for the pooled items, not for R separate maxima;
//   decision  lane r adds rung r's new and old terms in ascending order and
//             applies mc3_accept; the ballot of the decisions is the same in
//             every wave.  Barrier; wave r, r + W, .. writes an accepted
//             rung's state, lane = position; barrier;
//   exchange  at t mod E = 0 lane r adds its replica's n terms, takes the
//             next rung's sum by a shuffle, decides pair (r, r + 1) and both
//             lanes take the other's slot.  No barrier, no LDS write;
//   record    rung 0's replica, by the chains' code with its slot's arrays.
// The arguments are one struct in device memory (Mc3Args).
__device__ __forceinline__ int lane_get(int x, int r) { return __builtin_amdgcn_readlane(x, r); }

constexpr int kMc3SlotBytes = kWave * 25;  // pre, term, fresh: 8 B a position; ord: 1

template <int W>
__global__ void __launch_bounds__(kWave *W) mc3_run_kernel(const Mc3Args *g, int64_t t_begin, int64_t nsteps) {
    extern __shared__ double mc3_lds[];
    __shared__ double picked[kWave];  // a record's chosen scores, by variable
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int n = g->n, R = g->rungs;
    const int64_t L = g->ladders, l = (int64_t)blockIdx.x;  // ladders <= 2^20
    uint64_t *pre = reinterpret_cast<uint64_t *>(mc3_lds);  // [R][64] each, by slot
    double *term = mc3_lds + R * kWave, *fresh = mc3_lds + 2 * R * kWave;
    uint8_t *ord = reinterpret_cast<uint8_t *>(mc3_lds + 3 * R * kWave);
    const uint64_t *sets = g->sets;
    const float *scores = g->scores;
    const int64_t *offsets = g->offsets;
    const uint64_t seed = g->seed;
    const int64_t t_call = g->t_call, thin = g->thin, E = g->swap_every;
    uint8_t *g_order = g->order + l * R * n;
    double *g_terms = g->terms + l * R * n;
    for (int idx = tid; idx < R * kWave; idx += kWave * W) {
        const int p = idx & (kWave - 1);
        if (p < n) {
            ord[idx] = g_order[(idx >> 6) * n + p];
            term[idx] = g_terms[(idx >> 6) * n + p];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < R * kWave; idx += kWave * W) {
        const int p = idx & (kWave - 1);
        if (p < n) {
            uint64_t U = 0;
            for (int q = 0; q < p; ++q) U |= 1ull << ord[(idx & ~(kWave - 1)) + q];
            pre[idx] = U;
        }
    }
    const bool rung = lane < R;
    int slot = rung ? g->perm[l * R + lane] : 0;
    const double beta = rung ? g->betas[lane] : 0.0;
    const double beta_next = __shfl_down(beta, 1, kWave);
    unsigned long long acc = rung ? g->accepted[l * R + lane] : 0ull;
    unsigned long long swp = lane < R - 1 ? g->swaps[l * (R - 1) + lane] : 0ull;
    __syncthreads();
    for (int64_t s = 0; s < nsteps; ++s) {
        const int64_t t = t_begin + s + 1;
        double delta = neg_inf();
        bool take = false;
        if (n > 1) {
            int lo = 0, hi = -1, va = 0, vb = 0;
            uint64_t u_acc = 0;
            if (rung) {
                uint32_t w[4];
                mcmc_draw(seed, (uint64_t)t, (uint32_t)(l * R + slot), 0u, w);
                const McmcMove mv = mcmc_move(w, n);
                lo = mv.i < mv.j ? mv.i : mv.j, hi = mv.i < mv.j ? mv.j : mv.i;
                va = ord[slot * kWave + lo], vb = ord[slot * kWave + hi];
                u_acc = mv.u_acc;
            }
            const int span = hi - lo + 1;  // 0 beyond the rungs
            int incl = span;
            for (int d = 1; d < kMc3MaxRungs; d <<= 1) {
                const int y = __shfl_up(incl, d, kWave);
                if (lane >= d) incl += y;
            }
            const int start = incl - span, total = lane_get(incl, R - 1);
            for (int q = wave; q < total; q += W) {
                const int r = __popcll(__ballot(rung && start <= q)) - 1;
                const int rlo = lane_get(lo, r), rhi = lane_get(hi, r), rva = lane_get(va, r), rvb = lane_get(vb, r);
                const int base = lane_get(slot, r) * kWave, p = rlo + q - lane_get(start, r);
                const uint64_t flip = (1ull << rva) ^ (1ull << rvb);
                const int v = p == rlo ? rvb : p == rhi ? rva : ord[base + p];
                const uint64_t U = p == rlo ? pre[base + rlo] : pre[base + p] ^ flip;
                const double x = wave_term(sets, scores, offsets[v], offsets[v + 1], U, lane);
                if (lane == 0) fresh[base + p] = x;
            }
            __syncthreads();
            if (rung) {
                double now = 0.0, was = 0.0;
                bool none = false;
                for (int p = lo; p <= hi; ++p) {
                    const double x = fresh[slot * kWave + p];
                    none = none || !(x > neg_inf());
                    now += x;
                    was += term[slot * kWave + p];
                }
                if (!none) delta = now - was;
                take = mc3_accept(beta, delta, u_acc);
            }
            const unsigned long long takes = __ballot(take);
            __syncthreads();  // every wave has read the old terms
            for (int r = wave; r < R; r += W) {
                if (!((takes >> r) & 1ull)) continue;
                const int rlo = lane_get(lo, r), rhi = lane_get(hi, r), rva = lane_get(va, r), rvb = lane_get(vb, r);
                const int at = lane_get(slot, r) * kWave + lane;
                if (lane >= rlo && lane <= rhi) {
                    term[at] = fresh[at];
                    if (lane > rlo) pre[at] ^= (1ull << rva) ^ (1ull << rvb);
                    if (lane == rlo) ord[at] = (uint8_t)rvb;
                    if (lane == rhi) ord[at] = (uint8_t)rva;
                }
            }
            if (take) ++acc;
            __syncthreads();
        }
        if (wave == 0 && rung) {
            const int64_t at = ((t - t_call - 1) * L + l) * R + lane;
            if (g->t_delta) g->t_delta[at] = delta;
            if (g->t_accept) g->t_accept[at] = take ? 1 : 0;
        }
        if (R > 1 && t % E == 0) {
            const int64_t x = t / E;
            double S = 0.0;
            if (rung)
                for (int p = 0; p < n; ++p) S += term[slot * kWave + p];
            const double S_next = __shfl_down(S, 1, kWave);
            double d = neg_inf();
            bool sw = false;
            if (rung && mc3_pair_considered(x, lane, R)) {
                uint32_t w[4];
                mcmc_draw(seed, (uint64_t)t, (uint32_t)(l * R + lane), kMc3SwapDomain, w);
                d = mc3_swap_d(beta, beta_next, S, S_next);
                sw = mc3_swap_accept(d, (uint64_t)w[0] | ((uint64_t)w[1] << 32));
            }
            const unsigned long long sws = __ballot(sw);
            const int above = __shfl_down(slot, 1, kWave), below = __shfl_up(slot, 1, kWave);
            if (sw) slot = above;
            else if (lane > 0 && ((sws >> (lane - 1)) & 1ull)) slot = below;
            if (wave == 0 && lane < R - 1) {
                const int64_t at = ((x - t_call / E - 1) * L + l) * (R - 1) + lane;
                if (g->t_swap_d) g->t_swap_d[at] = d;
                if (g->t_swap_accept) g->t_swap_accept[at] = sw ? 1 : 0;
                if (sw) ++swp;
            }
        }
        if (t % thin == 0) {
            const int cold = lane_get(slot, 0), base = cold * kWave;
            const uint32_t c = (uint32_t)(l * R + cold);
            const int64_t idx = (t / thin - t_call / thin - 1) * L + l;
            uint8_t *r_order = g->r_order;
            double *r_score = g->r_score, *r_weight = g->r_weight;
            uint64_t *r_parents = g->r_parents;
            if (r_order && tid < n) r_order[idx * n + tid] = ord[base + tid];
            if (r_score && tid == 0) {
                double sum = 0.0;
                for (int p = 0; p < n; ++p) sum += term[base + p];
                r_score[idx] = sum;
            }
            if (r_parents) {
                for (int p = wave; p < n; p += W) {
                    uint32_t w[4];
                    mcmc_draw(seed, (uint64_t)t, c, (uint32_t)(1 + p), w);
                    const uint64_t u_set = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
                    const int v = ord[base + p];
                    const int64_t e = wave_pick(sets, scores, offsets[v], offsets[v + 1], pre[base + p], term[base + p], u_set, lane);
                    if (lane == 0) {
                        if (e < 0) {
                            atomicOr(g->err, kErrPick);  // as in mcmc_run_kernel
                            r_parents[idx * n + v] = 0;
                            picked[v] = 0.0;
                        } else {
                            r_parents[idx * n + v] = sets[e];
                            picked[v] = (double)scores[e];
                        }
                    }
                }
                __syncthreads();
                if (r_weight && tid == 0) {
                    double sum = 0.0;
                    for (int v = 0; v < n; ++v) sum += picked[v];
                    r_weight[idx] = sum;
                }
                __syncthreads();  // before the next record's picks
            }
        }
    }
    for (int idx = tid; idx < R * kWave; idx += kWave * W) {
        const int p = idx & (kWave - 1);
        if (p < n) {
            g_order[(idx >> 6) * n + p] = ord[idx];
            g_terms[(idx >> 6) * n + p] = term[idx];
        }
    }
    if (wave == 0 && rung) {
        g->perm[l * R + lane] = (uint8_t)slot;
        g->accepted[l * R + lane] = acc;
    }
    if (wave == 0 && lane < R - 1) g->swaps[l * (R - 1) + lane] = swp;
}

// ---- host
OrderMcmcState &state(ulg_ctx *c) {
    if (!c->mcmc) c->mcmc = new OrderMcmcState();
    return *c->mcmc;
}

uint64_t table_slots(int64_t total) {
    uint64_t cap = 64;
    while (cap < 2 * (uint64_t)total) cap <<= 1;
    return cap;
}

bool is_permutation(const uint8_t *row, int n) {
    uint64_t seen = 0;
    for (int p = 0; p < n; ++p) {
        if (row[p] >= n || ((seen >> row[p]) & 1ull)) return false;
        seen |= 1ull << row[p];
    }
    return true;
}

int launch_score(ulg_ctx *c, OrderMcmcState &s, const uint8_t *d_orders, int64_t count, double *d_terms) {
    const uint64_t pairs = (uint64_t)count * (uint64_t)s.n;
    prof_begin(c, "mcmc_score");
    mcmc_score_kernel<<<flat_grid((pairs + kB / kWave - 1) / (kB / kWave)), kB, 0, c->stream>>>(s.d_sets.p, s.d_scores.p, s.d_offsets.p,
                                                                                               s.n, d_orders, count, d_terms);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    return ULG_OK;
}

// The arguments that need no device, for both begins
int check_begin_args(ulg_ctx *c, const std::string &who, int n, int64_t chains, const uint8_t *init_order, const char *what = "chain") {
    if (n < 1) return set_err(c, ULG_ERR_ARG, who + ": n < 1");
    if (n > kMcmcMaxVars) return set_err(c, ULG_ERR_UNSUPPORTED, who + ": n = " + std::to_string(n) + "; at most 63 variables");
    if (chains < 1 || chains > kMcmcMaxChains) return set_err(c, ULG_ERR_ARG, who + ": chains must be 1..2^20");
    if (init_order)
        for (int64_t k = 0; k < chains; ++k)
            if (!is_permutation(init_order + k * n, n))
                return set_err(c, ULG_ERR_ARG, who + ": the initial order of " + what + " " + std::to_string(k) + " is not a permutation");
    return ULG_OK;
}

// Lists and chains beyond the free device memory (what the state already
// holds counts as free: its buffers are reused or replaced).  Nothing has
// been allocated yet.
int refuse_size(ulg_ctx *c, const std::string &who, int n, int64_t total, int64_t chains, double per_chain = 0.0) {
    size_t free_b = 0, total_b = 0;
    ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const double need = 12.0 * (double)total + 8.0 * (n + 1) + 8.0 * (double)table_slots(total) + (9.0 * n + 8.0 + per_chain) * (double)chains + 8.0 * 16 + 256.0;
    const double have = (double)free_b + (c->mcmc ? (double)c->mcmc->held_bytes() : 0.0);
    if (need > have) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "%s: n = %d with %lld sets and %lld chains needs %.0f bytes of device memory, %.0f are free",
                      who.c_str(), n, (long long)total, (long long)chains, need, have);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    return ULG_OK;
}

// The lists are on the device in s (variable order) with s.n and s.total set,
// s.offsets their offsets on the host: the checks, the initial orders, the terms.
// lists_only: the checks alone, for the partition MCMC (partition_mcmc.hip), which keeps its own chains.
// tables: option "mcmc_tables" of ulg_order_mcmc_begin* -- the log-sum tables are built and the chains' terms read from them;
// picks: option "mcmc_table_picks" with it -- the build keeps the stage tables and the entry map for the records' DAGs.
int begin(ulg_ctx *c, const std::string &who, OrderMcmcState &s, int64_t chains, uint64_t seed, const uint8_t *init_order,
          const char *what = "chain", bool lists_only = false, bool tables = false, bool picks = false) {
    const std::vector<int64_t> &offs = s.offsets;
    const int n = s.n;
    s.ready = false;
    s.tables = false;
    if (!tables) order_sumtables_drop(s);
    if (!picks) order_picktables_drop(s);
    DevBuf<unsigned long long> table;  // the call's own
    const uint64_t slots = table_slots(s.total);
    int rc;
    if ((rc = ensure(c, table, (size_t)slots)) || (rc = ensure(c, s.d_err, 2))) return rc;
    if (!lists_only && ((rc = ensure(c, s.d_order, (size_t)(chains * n))) || (rc = ensure(c, s.d_terms, (size_t)(chains * n))) ||
                        (rc = ensure(c, s.d_accepted, (size_t)chains))))
        return rc;
    static const unsigned int err0[2] = {0u, 0xFFFFFFFFu};  // static: the copy's source outlives every return
    ULG_HIP(c, hipMemcpyAsync(s.d_err.p, err0, sizeof err0, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemsetAsync(table.p, 0, (size_t)slots * 8, c->stream));
    if (!lists_only) ULG_HIP(c, hipMemsetAsync(s.d_accepted.p, 0, (size_t)chains * 8, c->stream));
    int64_t longest = 1;
    for (int v = 0; v < n; ++v) longest = std::max(longest, offs[v + 1] - offs[v]);
    prof_begin(c, "mcmc_check_lists");
    mcmc_check_lists_kernel<<<dim3((unsigned)std::min<int64_t>((longest + kB - 1) / kB, 4096), (unsigned)n), kB, 0, c->stream>>>(
        s.d_sets.p, s.d_scores.p, s.d_offsets.p, n, table.p, slots - 1, s.d_err.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    unsigned int err[2] = {0, 0};
    ULG_HIP(c, hipMemcpyAsync(err, s.d_err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    if (err[0]) {
        std::string msg = who + ":";
        if (err[0] & kErrSet) msg += " a set holds its own variable or a bit >= n;";
        if (err[0] & kErrScore) msg += " a score is NaN or infinite;";
        if (err[0] & kErrDup) msg += " a variable lists a set twice;";
        msg.pop_back();
        return set_err(c, ULG_ERR_ARG, msg);
    }
    if (lists_only) return ULG_OK;
    s.table_picks = tables && picks;  // read by the plan and the build
    if (tables && ((rc = order_sumtables_plan(c, who, s)) || (rc = order_sumtables_build(c, s)))) {
        order_picktables_drop(s);  // a refused begin keeps no stage table or map
        return rc;
    }
    if (init_order) {
        ULG_HIP(c, hipMemcpyAsync(s.d_order.p, init_order, (size_t)(chains * n), hipMemcpyHostToDevice, c->stream));
        ULG_HIP(c, hipStreamSynchronize(c->stream));  // init_order is the caller's again, whatever returns below
    } else {
        prof_begin(c, "mcmc_shuffle");
        mcmc_shuffle_kernel<<<flat_grid(((uint64_t)chains + kB - 1) / kB), kB, 0, c->stream>>>(s.d_order.p, chains, n, seed);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    if ((rc = s.tables ? order_sumtables_terms(c, s, chains) : launch_score(c, s, s.d_order.p, chains, s.d_terms.p))) return rc;
    prof_begin(c, "mcmc_scan");
    mcmc_scan_kernel<<<flat_grid(((uint64_t)chains + kB - 1) / kB), kB, 0, c->stream>>>(s.d_terms.p, chains, n, s.d_err.p + 1);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    ULG_HIP(c, hipMemcpyAsync(err, s.d_err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (err[1] != 0xFFFFFFFFu)
        return set_err(c, ULG_ERR_ARG,
                       who + ": the initial order of " + what + " " + std::to_string(err[1]) +
                           " has a variable without a stored parent set among its predecessors (a term of -inf: probability 0)");
    s.chains = chains;
    s.rungs = 0;
    s.seed = seed;
    s.step = 0;
    s.ready = true;
    return ULG_OK;
}

// option "mcmc_table_picks" descends the tables of option "mcmc_tables": refused without them
int check_table_picks(ulg_ctx *c, const std::string &who) {
    if (c->opt.mcmc_table_picks && !c->opt.mcmc_tables)
        return set_err(c, ULG_ERR_ARG, who + ": option \"mcmc_table_picks\" requires option \"mcmc_tables\" = 1");
    return ULG_OK;
}

template <int W>
void launch_run(ulg_ctx *c, const RunArgs &a) {
    mcmc_run_kernel<W><<<dim3((unsigned)a.chains), kWave * W, 0, c->stream>>>(a);
}

// Both kinds of begin on the caller's lists (`chains` chains, or as many
// replicas of ladders: `what` names them in a refusal, per_chain is what a
// ladder's replica holds beyond a chain's bytes)
int begin_on_lists(ulg_ctx *c, const std::string &who, int n, const int64_t *offsets, const uint64_t *sets, const float *scores,
                   int device_ptrs, int64_t chains, uint64_t seed, const uint8_t *init_order, const char *what, double per_chain,
                   bool lists_only = false, bool tables = false, bool picks = false) {
    if (!offsets) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
    if (int rc = check_begin_args(c, who, n, chains, init_order, what)) return rc;
    for (int v = 0; v < n; ++v)
        if (offsets[v + 1] < offsets[v]) return set_err(c, ULG_ERR_ARG, who + ": offsets not ascending");
    const int64_t total = offsets[n] - offsets[0];
    if (total && (!sets || !scores)) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
    ULG_HIP(c, hipSetDevice(c->device));
    if (int rc = refuse_size(c, who, n, total, chains, per_chain)) return rc;
    OrderMcmcState &s = state(c);
    s.ready = false;
    int rc;
    if ((rc = ensure(c, s.d_sets, (size_t)total)) || (rc = ensure(c, s.d_scores, (size_t)total)) ||
        (rc = ensure(c, s.d_offsets, (size_t)n + 1)))
        return rc;
    s.n = n;
    s.total = total;
    std::vector<int64_t> &offs = s.offsets;
    offs.assign((size_t)n + 1, 0);
    for (int v = 0; v <= n; ++v) offs[v] = offsets[v] - offsets[0];
    const hipMemcpyKind kind = device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (total) {
        ULG_HIP(c, hipMemcpyAsync(s.d_sets.p, sets + offsets[0], (size_t)total * 8, kind, c->stream));
        ULG_HIP(c, hipMemcpyAsync(s.d_scores.p, scores + offsets[0], (size_t)total * 4, kind, c->stream));
    }
    ULG_HIP(c, hipMemcpyAsync(s.d_offsets.p, offs.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    return begin(c, who, s, chains, seed, init_order, what, lists_only, tables, picks);
}

// ... and on the lists of the last scoring call
int begin_on_scored(ulg_ctx *c, const std::string &who, int64_t chains, uint64_t seed, const uint8_t *init_order, const char *what,
                    double per_chain, bool lists_only = false, bool tables = false, bool picks = false) {
    if (int rc0 = finish_pending(c)) return rc0;
    if (!c->scored) return set_err(c, ULG_ERR_STATE, who + ": no scoring call yet");
    const int n = c->n;
    std::vector<int> where((size_t)std::max(n, 1), -1);
    bool all = c->nv == n && n >= 1;
    for (int i = 0; all && i < n; ++i) {
        const int v = c->vars[i];
        all = v >= 0 && v < n && where[v] < 0;
        if (all) where[v] = i;
    }
    if (!all) return set_err(c, ULG_ERR_STATE, who + ": every variable must be scored in this context");
    if (int rc = check_begin_args(c, who, n, chains, init_order, what)) return rc;
    ULG_HIP(c, hipSetDevice(c->device));
    std::vector<int64_t> src((size_t)n + 1);
    ULG_HIP(c, hipMemcpyAsync(src.data(), c->out_offsets.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t total = src[n];
    if (int rc = refuse_size(c, who, n, total, chains, per_chain)) return rc;
    OrderMcmcState &s = state(c);
    s.ready = false;
    int rc;
    if ((rc = ensure(c, s.d_sets, (size_t)total)) || (rc = ensure(c, s.d_scores, (size_t)total)) ||
        (rc = ensure(c, s.d_offsets, (size_t)n + 1)))
        return rc;
    s.n = n;
    s.total = total;
    // the lists by variable index, each variable's sets in their stored order
    std::vector<int64_t> &offs = s.offsets;
    offs.assign((size_t)n + 1, 0);
    for (int v = 0; v < n; ++v) {
        const int i = where[v];
        const int64_t cnt = src[i + 1] - src[i];
        offs[v + 1] = offs[v] + cnt;
        if (cnt) {
            ULG_HIP(c, hipMemcpyAsync(s.d_sets.p + offs[v], c->out_sets.p + src[i], (size_t)cnt * 8, hipMemcpyDeviceToDevice, c->stream));
            ULG_HIP(c, hipMemcpyAsync(s.d_scores.p + offs[v], c->out_scores.p + src[i], (size_t)cnt * 4, hipMemcpyDeviceToDevice,
                                      c->stream));
        }
    }
    ULG_HIP(c, hipMemcpyAsync(s.d_offsets.p, offs.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    return begin(c, who, s, chains, seed, init_order, what, lists_only, tables, picks);
}

// ---- ladders
constexpr double kMc3ReplicaBytes = 9.0;  // beyond a chain's: the rung's slot byte and the pair's count

// What ulg_order_mc3_begin* refuse before any device work
int mc3_check_args(ulg_ctx *c, const std::string &who, int64_t ladders, int rungs, const double *betas, int64_t swap_every) {
    if (rungs < 1 || rungs > kMc3MaxRungs) return set_err(c, ULG_ERR_ARG, who + ": rungs must be 1..16");
    if (ladders < 1 || ladders > kMcmcMaxChains / rungs) return set_err(c, ULG_ERR_ARG, who + ": ladders x rungs must be 1..2^20");
    if (!betas || betas[0] != 1.0) return set_err(c, ULG_ERR_ARG, who + ": betas[0] must be 1");
    for (int r = 1; r < rungs; ++r)  // false for a NaN too; below 1, so finite
        if (!(betas[r] > 0.0) || !(betas[r] < betas[r - 1]))
            return set_err(c, ULG_ERR_ARG, who + ": betas must be strictly descending and > 0");
    if (swap_every < 1) return set_err(c, ULG_ERR_ARG, who + ": swap_every must be >= 1");
    return ULG_OK;
}

// After begin() made ladders x rungs replicas as chains: the rungs' slots, the
// pairs' counts, and the state's reading as ladders.
int mc3_make_ladders(ulg_ctx *c, int64_t ladders, int rungs, const double *betas, int64_t swap_every) {
    OrderMcmcState &s = *c->mcmc;
    s.ready = false;
    const size_t reps = (size_t)ladders * (size_t)rungs, pairs = (size_t)ladders * (size_t)(rungs - 1);
    int rc;
    if ((rc = ensure(c, s.d_perm, reps)) || (rc = ensure(c, s.d_swaps, pairs)) || (rc = ensure(c, s.d_args, 1))) return rc;
    std::vector<uint8_t> perm(reps);
    for (size_t k = 0; k < reps; ++k) perm[k] = (uint8_t)(k % (size_t)rungs);
    ULG_HIP(c, hipMemcpyAsync(s.d_perm.p, perm.data(), reps, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemsetAsync(s.d_swaps.p, 0, std::max<size_t>(pairs, 1) * 8, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));  // perm is read until here
    s.chains = ladders;
    s.rungs = rungs;
    s.swap_every = swap_every;
    for (int r = 0; r < kMc3MaxRungs; ++r) s.betas[r] = r < rungs ? betas[r] : 0.0;
    s.ready = true;
    return ULG_OK;
}

template <int W>
void launch_mc3(ulg_ctx *c, const OrderMcmcState &s, int64_t t_begin, int64_t nsteps) {
    mc3_run_kernel<W><<<dim3((unsigned)s.chains), kWave * W, (size_t)s.rungs * kMc3SlotBytes, c->stream>>>(s.d_args.p, t_begin, nsteps);
}

}  // namespace

namespace ulg {

// The partition MCMC's lists: uploaded and checked as a begin's, kept in the
// order MCMC's state with its chains ended.
int order_mcmc_take_lists(ulg_ctx *c, const std::string &who, int n, const int64_t *offsets, const uint64_t *sets, const float *scores,
                          int device_ptrs, int64_t chains) {
    if (c->mcmc) c->mcmc->ready = false;
    return begin_on_lists(c, who, n, offsets, sets, scores, device_ptrs, chains, 0, nullptr, "chain", 0.0, true);
}
int order_mcmc_take_scored(ulg_ctx *c, const std::string &who, int64_t chains) {
    if (c->mcmc) c->mcmc->ready = false;
    return begin_on_scored(c, who, chains, 0, nullptr, "chain", 0.0, true);
}

}  // namespace ulg

extern "C" {

int ulg_order_mcmc_begin(ulg_ctx *c, int n, const int64_t *offsets, const uint64_t *sets, const float *scores, int device_ptrs,
                         int64_t chains, uint64_t seed, const uint8_t *init_order) {
    if (!c) return ULG_ERR_ARG;
    partition_mcmc_end(c);  // a begin of either family ends the partition chains
    order_search_end(c);    // ... and the searches
    if (c->mcmc) c->mcmc->ready = false;  // a begin that is refused, for whatever reason, leaves no chains
    if (int rc = check_table_picks(c, "ulg_order_mcmc_begin")) return rc;
    return begin_on_lists(c, "ulg_order_mcmc_begin", n, offsets, sets, scores, device_ptrs, chains, seed, init_order, "chain", 0.0, false,
                          c->opt.mcmc_tables != 0, c->opt.mcmc_table_picks != 0);
}

int ulg_order_mcmc_begin_from_scores(ulg_ctx *c, int64_t chains, uint64_t seed, const uint8_t *init_order) {
    if (!c) return ULG_ERR_ARG;
    partition_mcmc_end(c);  // a begin of either family ends the partition chains
    order_search_end(c);    // ... and the searches
    if (c->mcmc) c->mcmc->ready = false;  // as ulg_order_mcmc_begin
    if (int rc = check_table_picks(c, "ulg_order_mcmc_begin_from_scores")) return rc;
    return begin_on_scored(c, "ulg_order_mcmc_begin_from_scores", chains, seed, init_order, "chain", 0.0, false, c->opt.mcmc_tables != 0,
                           c->opt.mcmc_table_picks != 0);
}

int ulg_order_mcmc_run(ulg_ctx *c, int64_t steps, int64_t thin, uint8_t *order, double *log_score, uint64_t *parents,
                       double *log_weight, int64_t *accepted, double *trace_delta, uint8_t *trace_accept, int64_t *records) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_mcmc_run";
    if (!c->mcmc || !c->mcmc->ready || c->mcmc->rungs) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_mcmc_begin");
    OrderMcmcState &s = *c->mcmc;
    if (steps < 0 || thin < 1) return set_err(c, ULG_ERR_ARG, who + ": steps must be >= 0 and thin >= 1");
    if (steps > INT64_MAX - s.step) return set_err(c, ULG_ERR_ARG, who + ": the step count passes 2^63");
    if (log_weight && !parents) return set_err(c, ULG_ERR_ARG, who + ": log_weight needs parents");
    const int n = s.n;
    const int64_t chains = s.chains, t0 = s.step;
    const int64_t recs = (t0 + steps) / thin - t0 / thin;
    ULG_HIP(c, hipSetDevice(c->device));
    // the device buffers of the call, before anything is allocated (what the
    // state holds of an earlier run counts as free: reused or replaced)
    const double cells = (double)recs * (double)chains, moves = (double)steps * (double)chains;
    {
        const double need = cells * ((order ? n : 0) + (log_score ? 8.0 : 0.0) + (parents ? 8.0 * n : 0.0) + (log_weight ? 8.0 : 0.0)) +
                            moves * ((trace_delta ? 8.0 : 0.0) + (trace_accept ? 1.0 : 0.0)) + 6 * 16.0 + 256.0;
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        const double have = (double)free_b + (double)s.run_bytes();
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld records and %lld steps of %lld chains need %.0f bytes of device memory, %.0f are free",
                          who.c_str(), (long long)recs, (long long)steps, (long long)chains, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    const size_t ncell = (size_t)recs * (size_t)chains, nmove = (size_t)steps * (size_t)chains;
    int rc;
    if ((order && (rc = ensure(c, s.r_order, ncell * n))) || (log_score && (rc = ensure(c, s.r_score, ncell))) ||
        (parents && (rc = ensure(c, s.r_parents, ncell * n))) || (log_weight && (rc = ensure(c, s.r_weight, ncell))) ||
        (trace_delta && (rc = ensure(c, s.r_tdelta, nmove))) || (trace_accept && (rc = ensure(c, s.r_taccept, nmove))))
        return rc;
    ULG_HIP(c, hipMemsetAsync(s.d_err.p, 0, sizeof(unsigned int), c->stream));
    RunArgs a;
    a.sets = s.d_sets.p, a.scores = s.d_scores.p, a.offsets = s.d_offsets.p;
    a.order = s.d_order.p, a.terms = s.d_terms.p, a.accepted = s.d_accepted.p;
    a.n = n, a.chains = chains, a.seed = s.seed;
    a.t_call = t0, a.thin = thin;
    a.r_order = order ? s.r_order.p : nullptr;
    a.r_score = log_score ? s.r_score.p : nullptr;
    a.r_parents = parents ? s.r_parents.p : nullptr;
    a.r_weight = log_weight ? s.r_weight.p : nullptr;
    a.t_delta = trace_delta ? s.r_tdelta.p : nullptr;
    a.t_accept = trace_accept ? s.r_taccept.p : nullptr;
    a.err = s.d_err.p;
    const int64_t cap = c->opt.mcmc_launch_steps;
    for (int64_t done = 0; done < steps; done += a.nsteps) {
        a.t_begin = t0 + done;
        a.nsteps = std::min(cap, steps - done);
        prof_begin(c, s.table_picks ? "opick_run" : s.tables ? "ostab_run" : "mcmc_run");
        if (s.table_picks) {
            order_picktables_run(c, s, a);
        } else if (s.tables) {
            order_sumtables_run(c, s, a);
        } else {
            switch (c->opt.mcmc_waves) {
                case 1: launch_run<1>(c, a); break;
                case 2: launch_run<2>(c, a); break;
                case 8: launch_run<8>(c, a); break;
                default: launch_run<4>(c, a); break;
            }
        }
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    unsigned int err = 0;
    ULG_HIP(c, hipMemcpyAsync(&err, s.d_err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    s.step = t0 + steps;  // the chains have moved, whatever becomes of the copies below
    if (err) return set_err(c, ULG_ERR_STATE, who + ": a record's parent-set step found no entry of positive weight");
    if (order && ncell) ULG_HIP(c, hipMemcpyAsync(order, s.r_order.p, ncell * n, hipMemcpyDeviceToHost, c->stream));
    if (log_score && ncell) ULG_HIP(c, hipMemcpyAsync(log_score, s.r_score.p, ncell * 8, hipMemcpyDeviceToHost, c->stream));
    if (parents && ncell) ULG_HIP(c, hipMemcpyAsync(parents, s.r_parents.p, ncell * n * 8, hipMemcpyDeviceToHost, c->stream));
    if (log_weight && ncell) ULG_HIP(c, hipMemcpyAsync(log_weight, s.r_weight.p, ncell * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace_delta && nmove) ULG_HIP(c, hipMemcpyAsync(trace_delta, s.r_tdelta.p, nmove * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace_accept && nmove) ULG_HIP(c, hipMemcpyAsync(trace_accept, s.r_taccept.p, nmove, hipMemcpyDeviceToHost, c->stream));
    if (accepted) ULG_HIP(c, hipMemcpyAsync(accepted, s.d_accepted.p, (size_t)chains * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    if (records) *records = recs;
    return ULG_OK;
}

int ulg_order_mcmc_state(ulg_ctx *c, uint8_t *order, double *terms, int64_t *step) {
    if (!c) return ULG_ERR_ARG;
    if (!c->mcmc || !c->mcmc->ready || c->mcmc->rungs) return set_err(c, ULG_ERR_STATE, "ulg_order_mcmc_state: no ulg_order_mcmc_begin");
    OrderMcmcState &s = *c->mcmc;
    const size_t cells = (size_t)s.chains * (size_t)s.n;
    ULG_HIP(c, hipSetDevice(c->device));
    if (order) ULG_HIP(c, hipMemcpyAsync(order, s.d_order.p, cells, hipMemcpyDeviceToHost, c->stream));
    if (terms) ULG_HIP(c, hipMemcpyAsync(terms, s.d_terms.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    if (step) *step = s.step;
    return ULG_OK;
}

int ulg_order_score(ulg_ctx *c, int64_t count, const uint8_t *orders, double *terms) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_score";
    if (!c->mcmc || !c->mcmc->ready) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_mcmc_begin");
    OrderMcmcState &s = *c->mcmc;
    const int n = s.n;
    if (count < 0 || (count > 0 && (!orders || !terms))) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
    if (count > (int64_t)1 << 40) return set_err(c, ULG_ERR_ARG, who + ": count out of range");
    for (int64_t k = 0; k < count; ++k)
        if (!is_permutation(orders + k * n, n))
            return set_err(c, ULG_ERR_ARG, who + ": order " + std::to_string(k) + " is not a permutation");
    if (count == 0) return ULG_OK;
    ULG_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)count * (size_t)n;
    {
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        const double need = 9.0 * (double)cells + 2 * 16.0 + 256.0, have = (double)free_b + (double)s.run_bytes();
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld orders of n = %d need %.0f bytes of device memory, %.0f are free", who.c_str(),
                          (long long)count, n, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    int rc;
    if ((rc = ensure(c, s.r_order, cells)) || (rc = ensure(c, s.r_score, cells))) return rc;
    ULG_HIP(c, hipMemcpyAsync(s.r_order.p, orders, cells, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_score(c, s, s.r_order.p, count, s.r_score.p))) return rc;
    ULG_HIP(c, hipMemcpyAsync(terms, s.r_score.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ULG_OK;
}

int ulg_order_mc3_begin(ulg_ctx *c, int n, const int64_t *offsets, const uint64_t *sets, const float *scores, int device_ptrs,
                        int64_t ladders, int rungs, const double *betas, int64_t swap_every, uint64_t seed, const uint8_t *init_order) {
    if (!c) return ULG_ERR_ARG;
    partition_mcmc_end(c);  // a begin of either family ends the partition chains
    order_search_end(c);    // ... and the searches
    const std::string who = "ulg_order_mc3_begin";
    if (c->mcmc) c->mcmc->ready = false;  // as ulg_order_mcmc_begin: a refused begin leaves neither chains nor ladders
    if (int rc = mc3_check_args(c, who, ladders, rungs, betas, swap_every)) return rc;
    if (int rc = begin_on_lists(c, who, n, offsets, sets, scores, device_ptrs, ladders * rungs, seed, init_order, "replica",
                                kMc3ReplicaBytes))
        return rc;
    return mc3_make_ladders(c, ladders, rungs, betas, swap_every);
}

int ulg_order_mc3_begin_from_scores(ulg_ctx *c, int64_t ladders, int rungs, const double *betas, int64_t swap_every, uint64_t seed,
                                    const uint8_t *init_order) {
    if (!c) return ULG_ERR_ARG;
    partition_mcmc_end(c);  // a begin of either family ends the partition chains
    order_search_end(c);    // ... and the searches
    const std::string who = "ulg_order_mc3_begin_from_scores";
    if (c->mcmc) c->mcmc->ready = false;
    if (int rc = mc3_check_args(c, who, ladders, rungs, betas, swap_every)) return rc;
    if (int rc = begin_on_scored(c, who, ladders * rungs, seed, init_order, "replica", kMc3ReplicaBytes)) return rc;
    return mc3_make_ladders(c, ladders, rungs, betas, swap_every);
}

int ulg_order_mc3_run(ulg_ctx *c, int64_t steps, int64_t thin, uint8_t *order, double *log_score, uint64_t *parents, double *log_weight,
                      int64_t *accepted, int64_t *swaps, double *trace_delta, uint8_t *trace_accept, double *trace_swap_d,
                      uint8_t *trace_swap_accept, int64_t *records) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_mc3_run";
    if (!c->mcmc || !c->mcmc->ready || !c->mcmc->rungs) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_mc3_begin");
    OrderMcmcState &s = *c->mcmc;
    if (steps < 0 || thin < 1) return set_err(c, ULG_ERR_ARG, who + ": steps must be >= 0 and thin >= 1");
    if (steps > INT64_MAX - s.step) return set_err(c, ULG_ERR_ARG, who + ": the step count passes 2^63");
    if (log_weight && !parents) return set_err(c, ULG_ERR_ARG, who + ": log_weight needs parents");
    const int n = s.n, R = s.rungs;
    const int64_t L = s.chains, t0 = s.step, E = s.swap_every;
    const int64_t recs = (t0 + steps) / thin - t0 / thin, rounds = (t0 + steps) / E - t0 / E;
    ULG_HIP(c, hipSetDevice(c->device));
    const double cells = (double)recs * (double)L, moves = (double)steps * (double)L * R, pairs = (double)rounds * (double)L * (R - 1);
    {
        const double need = cells * ((order ? n : 0) + (log_score ? 8.0 : 0.0) + (parents ? 8.0 * n : 0.0) + (log_weight ? 8.0 : 0.0)) +
                            moves * ((trace_delta ? 8.0 : 0.0) + (trace_accept ? 1.0 : 0.0)) +
                            pairs * ((trace_swap_d ? 8.0 : 0.0) + (trace_swap_accept ? 1.0 : 0.0)) + 8 * 16.0 + 256.0;
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        const double have = (double)free_b + (double)s.run_bytes();
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld records and %lld steps of %lld ladders need %.0f bytes of device memory, %.0f are free",
                          who.c_str(), (long long)recs, (long long)steps, (long long)L, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    const size_t ncell = (size_t)recs * (size_t)L, nmove = (size_t)steps * (size_t)L * R, npair = (size_t)rounds * (size_t)L * (R - 1);
    int rc;
    if ((order && (rc = ensure(c, s.r_order, ncell * n))) || (log_score && (rc = ensure(c, s.r_score, ncell))) ||
        (parents && (rc = ensure(c, s.r_parents, ncell * n))) || (log_weight && (rc = ensure(c, s.r_weight, ncell))) ||
        (trace_delta && (rc = ensure(c, s.r_tdelta, nmove))) || (trace_accept && (rc = ensure(c, s.r_taccept, nmove))) ||
        (trace_swap_d && (rc = ensure(c, s.r_tswapd, npair))) || (trace_swap_accept && (rc = ensure(c, s.r_tswapacc, npair))))
        return rc;
    ULG_HIP(c, hipMemsetAsync(s.d_err.p, 0, sizeof(unsigned int), c->stream));
    Mc3Args &a = s.args;
    a.sets = s.d_sets.p, a.scores = s.d_scores.p, a.offsets = s.d_offsets.p;
    a.order = s.d_order.p, a.terms = s.d_terms.p, a.perm = s.d_perm.p, a.accepted = s.d_accepted.p, a.swaps = s.d_swaps.p;
    a.n = n, a.rungs = R, a.ladders = L, a.seed = s.seed, a.swap_every = E;
    a.t_call = t0, a.thin = thin;
    a.r_order = order ? s.r_order.p : nullptr;
    a.r_score = log_score ? s.r_score.p : nullptr;
    a.r_parents = parents ? s.r_parents.p : nullptr;
    a.r_weight = log_weight ? s.r_weight.p : nullptr;
    a.t_delta = trace_delta ? s.r_tdelta.p : nullptr;
    a.t_accept = trace_accept ? s.r_taccept.p : nullptr;
    a.t_swap_d = trace_swap_d ? s.r_tswapd.p : nullptr;
    a.t_swap_accept = trace_swap_accept ? s.r_tswapacc.p : nullptr;
    a.err = s.d_err.p;
    for (int r = 0; r < kMc3MaxRungs; ++r) a.betas[r] = s.betas[r];
    ULG_HIP(c, hipMemcpyAsync(s.d_args.p, &a, sizeof a, hipMemcpyHostToDevice, c->stream));
    const int64_t cap = c->opt.mcmc_launch_steps;
    for (int64_t done = 0; done < steps;) {
        const int64_t now = std::min(cap, steps - done);
        prof_begin(c, "mc3_run");
        switch (c->opt.mc3_waves) {
            case 1: launch_mc3<1>(c, s, t0 + done, now); break;
            case 2: launch_mc3<2>(c, s, t0 + done, now); break;
            case 4: launch_mc3<4>(c, s, t0 + done, now); break;
            case 8: launch_mc3<8>(c, s, t0 + done, now); break;
            default: launch_mc3<16>(c, s, t0 + done, now); break;
        }
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
        done += now;
    }
    unsigned int err = 0;
    ULG_HIP(c, hipMemcpyAsync(&err, s.d_err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    s.step = t0 + steps;  // the ladders have moved, whatever becomes of the copies below
    if (err) return set_err(c, ULG_ERR_STATE, who + ": a record's parent-set step found no entry of positive weight");
    if (order && ncell) ULG_HIP(c, hipMemcpyAsync(order, s.r_order.p, ncell * n, hipMemcpyDeviceToHost, c->stream));
    if (log_score && ncell) ULG_HIP(c, hipMemcpyAsync(log_score, s.r_score.p, ncell * 8, hipMemcpyDeviceToHost, c->stream));
    if (parents && ncell) ULG_HIP(c, hipMemcpyAsync(parents, s.r_parents.p, ncell * n * 8, hipMemcpyDeviceToHost, c->stream));
    if (log_weight && ncell) ULG_HIP(c, hipMemcpyAsync(log_weight, s.r_weight.p, ncell * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace_delta && nmove) ULG_HIP(c, hipMemcpyAsync(trace_delta, s.r_tdelta.p, nmove * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace_accept && nmove) ULG_HIP(c, hipMemcpyAsync(trace_accept, s.r_taccept.p, nmove, hipMemcpyDeviceToHost, c->stream));
    if (trace_swap_d && npair) ULG_HIP(c, hipMemcpyAsync(trace_swap_d, s.r_tswapd.p, npair * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace_swap_accept && npair)
        ULG_HIP(c, hipMemcpyAsync(trace_swap_accept, s.r_tswapacc.p, npair, hipMemcpyDeviceToHost, c->stream));
    if (accepted) ULG_HIP(c, hipMemcpyAsync(accepted, s.d_accepted.p, (size_t)L * R * 8, hipMemcpyDeviceToHost, c->stream));
    if (swaps && R > 1) ULG_HIP(c, hipMemcpyAsync(swaps, s.d_swaps.p, (size_t)L * (R - 1) * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    if (records) *records = recs;
    return ULG_OK;
}

int ulg_order_mc3_state(ulg_ctx *c, uint8_t *order, double *terms, int64_t *replica, int64_t *step) {
    if (!c) return ULG_ERR_ARG;
    if (!c->mcmc || !c->mcmc->ready || !c->mcmc->rungs) return set_err(c, ULG_ERR_STATE, "ulg_order_mc3_state: no ulg_order_mc3_begin");
    OrderMcmcState &s = *c->mcmc;
    const int n = s.n, R = s.rungs;
    const size_t reps = (size_t)s.chains * (size_t)R, cells = reps * (size_t)n;
    if (order || terms || replica) {
        // the device keeps the state by replica; the caller reads it by rung
        std::vector<uint8_t> perm(reps), ord(order ? cells : 0);
        std::vector<double> trm(terms ? cells : 0);
        ULG_HIP(c, hipSetDevice(c->device));
        ULG_HIP(c, hipMemcpyAsync(perm.data(), s.d_perm.p, reps, hipMemcpyDeviceToHost, c->stream));
        if (order) ULG_HIP(c, hipMemcpyAsync(ord.data(), s.d_order.p, cells, hipMemcpyDeviceToHost, c->stream));
        if (terms) ULG_HIP(c, hipMemcpyAsync(trm.data(), s.d_terms.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
        ULG_HIP(c, hipStreamSynchronize(c->stream));
        for (size_t k = 0; k < reps; ++k) {
            const size_t from = k - k % (size_t)R + perm[k];
            if (replica) replica[k] = (int64_t)from;
            if (order) std::copy(ord.begin() + from * n, ord.begin() + (from + 1) * n, order + k * n);
            if (terms) std::copy(trm.begin() + from * n, trm.begin() + (from + 1) * n, terms + k * n);
        }
    }
    if (step) *step = s.step;
    return ULG_OK;
}

}  // extern "C"
