// order_sumtables.hip -- order MCMC over dense log-sum tables (option
// "mcmc_tables", ulg_order_mcmc_table; contract: include/ulg.h, "Order MCMC
// over log-sum tables"; arithmetic: order_sumtables_dev.h).  For every variable
// v the table L_v over the subsets of its candidate parents C_v holds
// ln sum exp(s_i) over the stored sets inside the subset -- a zeta transform
// with post_logaddexp, rounds in ascending bit order -- so a chain's order
// term is one load at idx_v(U) and a swap of two positions moves the indices
// between them by two bits.  A second contract for the term: a fixed FP64
// expression tree per slot, not the lists' integer sums.
//
// Kernels:
//   ostab_cand_kernel     one workgroup per variable: C_v, the OR of its sets
//   ostab_small_kernel    K_v <= 13: one workgroup per variable builds the table
//                         in LDS (64 KB) -- slots cleared to -inf, every entry's
//                         score stored at the index of its own set, the
//                         butterfly, one coalesced write of the table
//   ostab_clear_kernel    K_v > 13: -inf into the global table
//   ostab_scatter_kernel  ... the scores into it
//   ostab_tile_kernel     ... rounds 0 .. 12 on tiles of 2^13 slots in LDS
//   ostab_high_kernel     ... round j >= 13 as a strided pass over the pairs,
//                         launched in ascending j; each of the four serves
//                         every such variable at once (blockIdx.y)
//     butterfly  (lds_butterfly) a lane owns slot 256 r + tid, so bits 0 .. 5
//              of a slot are the lane: rounds 0 .. 5 are cross-lane exchanges
//              of the slot's register inside a wave, rounds 6 .. through LDS,
//              one barrier each.  A round reads slots without its bit and
//              writes slots with it: the value of a slot does not depend on
//              which lane, tile or launch made it.  post_logaddexp's early
//              returns stay branches: a wave whose pairs are all -inf or more
//              than 38 nats apart -- most waves of a sparse table -- skips
//              exp and log1p.
//     snapshots  under option "mcmc_table_picks" (order_picktables.hip; every
//              pointer of it is null otherwise) the rounds 6, 12, 18 and 24
//              also store the pair's old values into the stage tables, and
//              the clears and scatters fill the entry map.
//   ostab_terms_kernel   one wave per chain, lane p = position p: the
//                         predecessor masks by a prefix OR across the lanes,
//                         one load per term (the begin's terms)
//   ostab_run_kernel      one wave per chain, four chains to a workgroup, all
//                         steps of the launch, no barrier and no LDS.  Lane p
//                         owns position p: its variable, C and table base, the
//                         predecessor mask, the table index and the term.
//     move     the draw is wave-uniform integer work (the chain's number is
//              made scalar, so the Philox rounds run on the scalar unit);
//     terms    lanes strictly between lo and hi move their index by
//              - bit_v(va) + bit_v(vb); lane lo takes vb's C and base from
//              lane hi and forms the index of its own mask, lane hi likewise
//              for va with its mask flipped; each of lo .. hi one gather;
//     decision the two ascending sums are a uniform loop of lane reads over
//              lo .. hi -- the contract fixes the order, so no tree -- and
//              mcmc_accept gives the same bits in every lane;
//     record   the order and the ascending sum of the terms; a DAG by the
//              lists' wave_pick, one position after the other, the chosen
//              score kept by the lane of its variable.
// The device state between launches is the list path's: order, terms,
// accepted.  Indices and masks are formed again at the head of a launch.
// Plain vector stores only, no floating-point atomics, no communication
// between waves.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "order_picktables_dev.h"
#include "order_sumtables_wave.h"

using namespace ulg;

namespace {

constexpr int kB = 256;
constexpr int kLdsSlots = 1 << kTableLdsK;

constexpr uint64_t kGridX = 1ull << 20;
inline dim3 flat_grid(uint64_t blocks) {
    return dim3((unsigned)std::min<uint64_t>(blocks, kGridX), (unsigned)((blocks + kGridX - 1) / kGridX));
}
__device__ __forceinline__ uint64_t flat_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }
__global__ void __launch_bounds__(kB) ostab_cand_kernel(const uint64_t *sets, const int64_t *offsets, uint64_t *cand) {
    __shared__ uint64_t part[kB / kWave];
    const int v = blockIdx.x, tid = threadIdx.x;
    uint64_t C = 0;
    for (int64_t i = offsets[v] + tid, e = offsets[v + 1]; i < e; i += kB) C |= sets[i];
    for (int d = kWave / 2; d > 0; d >>= 1) C |= shfl_xor64(C, d);
    if ((tid & (kWave - 1)) == 0) part[tid >> 6] = C;
    __syncthreads();
    if (tid == 0) cand[v] = part[0] | part[1] | part[2] | part[3];
}

// Rounds 0 .. K-1 on L[0 .. 2^K) in LDS, K <= kTableLdsK, by the kB lanes of the
// workgroup, all of which call it.  Begins and ends on a barrier.
// snap6, snap12 (option "mcmc_table_picks"; null: no stores but L's): where the
// image goes as it stands before round 6 and before round 12.  The lane of a
// pair holds both of its slots' old values just then, and the pairs cover the
// image: two stores beside the round's own, in runs of 2^j slots, no barrier.
__device__ __forceinline__ void lds_butterfly(double *L, int K, int tid, double *snap6, double *snap12) {
    const int slots = 1 << K, lane = tid & (kWave - 1), low = K < 6 ? K : 6;
    __syncthreads();
    for (int base = 0; base < slots; base += kB) {
        const int x = base + tid;
        double val = x < slots ? L[x] : neg_inf();
        for (int j = 0; j < low; ++j) {
            const double o = __shfl_xor(val, 1 << j, kWave);  // every lane gives; the lanes with bit j take
            if ((lane >> j) & 1) val = ost_round(val, o);
        }
        if (x < slots) L[x] = val;
    }
    __syncthreads();
    for (int j = 6; j < K; ++j) {
        double *snap = j == kPickBits ? snap6 : j == 2 * kPickBits ? snap12 : nullptr;
        for (int q = tid; q < slots / 2; q += kB) {
            const int x = ((q >> j) << (j + 1)) | (1 << j) | (q & ((1 << j) - 1));
            const double with = L[x], without = L[x ^ (1 << j)];
            if (snap) snap[x] = with, snap[x ^ (1 << j)] = without;
            L[x] = ost_round(with, without);
        }
        __syncthreads();
    }
}

// What option "mcmc_table_picks" has the build kernels write beside the table
// (all null without it): the stage tables S_{v,c} at stage[soff[v] + (c - 1) 2^K_v]
// and the entry map E_v at entry[toff[v]].
struct Snap {
    double *stage;
    const int64_t *soff;
    int32_t *entry;
};

__global__ void __launch_bounds__(kB) ostab_small_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets,
                                                         const uint64_t *cand, const int64_t *toff, double *table, const Snap sn) {
    __shared__ double L[kLdsSlots];
    const int v = blockIdx.x, tid = threadIdx.x;
    const uint64_t C = cand[v];
    const int K = ot_popcount(C);
    if (K > kTableLdsK) return;  // the whole workgroup
    const int slots = 1 << K;
    int32_t *ent = sn.entry ? sn.entry + toff[v] : nullptr;
    for (int x = tid; x < slots; x += kB) {
        L[x] = neg_inf();
        if (ent) ent[x] = -1;  // ordered before the entries' stores by the barrier, as L's are
    }
    __syncthreads();
    for (int64_t b = offsets[v], i = b + tid, e = offsets[v + 1]; i < e; i += kB) {
        const uint32_t x = ot_index(C, sets[i]);
        L[x] = (double)scores[i];
        if (ent) ent[x] = (int32_t)(i - b);
    }
    double *s6 = sn.stage ? sn.stage + sn.soff[v] : nullptr;
    lds_butterfly(L, K, tid, s6, s6 ? s6 + slots : nullptr);
    double *out = table + toff[v];
    for (int x = tid; x < slots; x += kB) out[x] = L[x];
}

// grid (2^Kmax / kB, n): every slot of every variable with K > kTableLdsK
__global__ void __launch_bounds__(kB) ostab_clear_kernel(const uint64_t *cand, const int64_t *toff, double *table, int32_t *entry) {
    const int v = blockIdx.y;
    const int K = ot_popcount(cand[v]);
    const int64_t x = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (K <= kTableLdsK || x >= ot_slots(K)) return;
    table[toff[v] + x] = neg_inf();
    if (entry) entry[toff[v] + x] = -1;
}

// grid (any, n): the entries of every variable with K > kTableLdsK
__global__ void __launch_bounds__(kB) ostab_scatter_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets,
                                                           const uint64_t *cand, const int64_t *toff, double *table, int32_t *entry) {
    const int v = blockIdx.y;
    const uint64_t C = cand[v];
    if (ot_popcount(C) <= kTableLdsK) return;
    double *out = table + toff[v];
    int32_t *ent = entry ? entry + toff[v] : nullptr;
    for (int64_t b = offsets[v], i = b + (int64_t)blockIdx.x * kB + threadIdx.x, e = offsets[v + 1]; i < e; i += (int64_t)gridDim.x * kB) {
        const uint32_t x = ot_index(C, sets[i]);
        out[x] = (double)scores[i];
        if (ent) ent[x] = (int32_t)(i - b);
    }
}

// grid (2^(Kmax - kTableLdsK), n): tile blockIdx.x of variable blockIdx.y
__global__ void __launch_bounds__(kB) ostab_tile_kernel(const uint64_t *cand, const int64_t *toff, double *table, double *stage,
                                                        const int64_t *soff) {
    __shared__ double L[kLdsSlots];
    const int v = blockIdx.y, tid = threadIdx.x;
    const int K = ot_popcount(cand[v]);
    if (K <= kTableLdsK || (int64_t)blockIdx.x >= ot_slots(K - kTableLdsK)) return;
    double *tile = table + toff[v] + (int64_t)blockIdx.x * kLdsSlots;
    for (int x = tid; x < kLdsSlots; x += kB) L[x] = tile[x];
    double *s6 = stage ? stage + soff[v] + (int64_t)blockIdx.x * kLdsSlots : nullptr;  // this tile of S_{v,1}, and of S_{v,2} behind it
    lds_butterfly(L, kTableLdsK, tid, s6, s6 ? s6 + ot_slots(K) : nullptr);
    for (int x = tid; x < kLdsSlots; x += kB) tile[x] = L[x];
}

// grid (2^(Kmax - 1) / kB, n): round j >= kTableLdsK, a lane per pair of slots.
// stage (non-null in rounds 18 and 24 under "mcmc_table_picks"): the pair's old
// values go to S_{v, j / 6} as the round reads them -- the copy fused into the pass.
__global__ void __launch_bounds__(kB) ostab_high_kernel(const uint64_t *cand, const int64_t *toff, double *table, int j, double *stage,
                                                        const int64_t *soff) {
    const int v = blockIdx.y;
    const int K = ot_popcount(cand[v]);
    const int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (K <= j || q >= ot_slots(K - 1)) return;
    const int64_t bit = (int64_t)1 << j, x = ((q >> j) << (j + 1)) | bit | (q & (bit - 1));
    double *L = table + toff[v];
    const double with = L[x], without = L[x ^ bit];
    if (stage) {
        double *snap = stage + soff[v] + (int64_t)(j / kPickBits - 1) * ot_slots(K);
        snap[x] = with, snap[x ^ bit] = without;
    }
    L[x] = ost_round(with, without);
}

// terms[c n + p] of every chain's order: a wave per chain
__global__ void __launch_bounds__(kB) ostab_terms_kernel(const uint64_t *cand, const int64_t *toff, const double *table, int n,
                                                         const uint8_t *order, int64_t chains, double *terms) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t c = flat_block() * (kB / kWave) + (threadIdx.x >> 6);
    if (c >= (uint64_t)chains) return;  // the whole wave
    const bool on = lane < n;
    const int v = on ? order[c * n + lane] : 0;
    const Place pl = place_of(cand, toff, v, on, lane);
    if (on) terms[c * n + lane] = table[pl.base + pl.idx];
}

__global__ void __launch_bounds__(kWave *kRunWaves) ostab_run_kernel(const RunArgs a, const uint64_t *cand, const int64_t *toff,
                                                                      const double *table) {
    const int lane = threadIdx.x & (kWave - 1);
    const int n = a.n;
    const int64_t c = (int64_t)blockIdx.x * kRunWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar
    if (c >= a.chains) return;  // the whole wave; the kernel has no barrier
    const bool on = lane < n;
    const int64_t at = c * n + lane;
    int v = on ? a.order[at] : 0;
    double term = on ? a.terms[at] : 0.0;
    Place pl = place_of(cand, toff, v, on, lane);  // masks and indices are not kept between launches
    unsigned long long acc = a.accepted[c];
    for (int64_t s = 0; s < a.nsteps; ++s) {
        const int64_t t = a.t_begin + s + 1;
        double delta = neg_inf();
        bool take = false;
        if (n > 1) {
            uint32_t w[4];
            mcmc_draw(a.seed, (uint64_t)t, (uint32_t)c, 0u, w);
            const McmcMove mv = mcmc_move(w, n);
            const int lo = mv.i < mv.j ? mv.i : mv.j, hi = mv.i < mv.j ? mv.j : mv.i;
            const int va = lane_get(v, lo), vb = lane_get(v, hi);
            const uint64_t flip = (1ull << va) ^ (1ull << vb);
            // the proposal's state of this lane: lo takes vb with its own mask, hi takes va with
            // its mask flipped, the lanes between keep their variable and trade va for vb
            const uint64_t Ca = lane_get64(pl.C, lo), Cb = lane_get64(pl.C, hi);  // read with every lane active
            const int64_t base_a = (int64_t)lane_get64((uint64_t)pl.base, lo), base_b = (int64_t)lane_get64((uint64_t)pl.base, hi);
            int nv = v;
            Place np = pl;
            if (lane == lo) {
                nv = vb, np.C = Cb, np.base = base_b;
                np.idx = ot_index(np.C, pl.pre);
            } else if (lane == hi) {
                nv = va, np.C = Ca, np.base = base_a;
                np.pre = pl.pre ^ flip;
                np.idx = ot_index(np.C, np.pre);
            } else if (lane > lo && lane < hi) {
                np.pre = pl.pre ^ flip;
                np.idx = pl.idx - ot_bit(pl.C, va) + ot_bit(pl.C, vb);
            }
            const bool touched = lane >= lo && lane <= hi;
            const double fresh = touched ? table[np.base + np.idx] : 0.0;  // the step's one gather
            double now = 0.0, was = 0.0;
            bool none = false;
            for (int p = lo; p <= hi; ++p) {  // ascending, as the contract has it
                const double x = lane_getd(fresh, p);
                none = none || !(x > neg_inf());
                now += x;
                was += lane_getd(term, p);
            }
            if (!none) delta = now - was;
            take = mcmc_accept(delta, mv.u_acc);
            if (take) {
                if (touched) v = nv, pl = np, term = fresh;
                ++acc;
            }
        }
        if (lane == 0) {
            const int64_t row = (t - a.t_call - 1) * a.chains + c;
            if (a.t_delta) a.t_delta[row] = delta;
            if (a.t_accept) a.t_accept[row] = take ? 1 : 0;
        }
        if (t % a.thin == 0) {
            const int64_t idx = (t / a.thin - a.t_call / a.thin - 1) * a.chains + c;
            if (a.r_order && on) a.r_order[idx * n + lane] = (uint8_t)v;
            if (a.r_score) {
                double sum = 0.0;
                for (int p = 0; p < n; ++p) sum += lane_getd(term, p);
                if (lane == 0) a.r_score[idx] = sum;
            }
            if (a.r_parents) {
                double picked = 0.0;  // lane u: the chosen score of variable u
                for (int p = 0; p < n; ++p) {
                    uint32_t w[4];
                    mcmc_draw(a.seed, (uint64_t)t, (uint32_t)c, (uint32_t)(1 + p), w);
                    const uint64_t u_set = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
                    const int u = lane_get(v, p);
                    const int64_t e = wave_pick(a.sets, a.scores, a.offsets[u], a.offsets[u + 1], lane_get64(pl.pre, p), lane_getd(term, p),
                                                u_set, lane);
                    if (lane == u) {
                        if (e < 0) {
                            atomicOr(a.err, kErrPick);  // the term is within K rounding steps of ln of the compatible weights' sum: as on the lists
                            a.r_parents[idx * n + u] = 0;
                        } else {
                            a.r_parents[idx * n + u] = a.sets[e];
                            picked = (double)a.scores[e];
                        }
                    }
                }
                if (a.r_weight) {
                    double sum = 0.0;
                    for (int u = 0; u < n; ++u) sum += lane_getd(picked, u);
                    if (lane == 0) a.r_weight[idx] = sum;
                }
            }
        }
    }
    if (on) {
        a.order[at] = (uint8_t)v;
        a.terms[at] = term;
    }
    if (lane == 0) a.accepted[c] = acc;
}

}  // namespace

namespace ulg {

void order_sumtables_drop(OrderMcmcState &s) {
    order_picktables_drop(s);
    s.tables = false;
    s.d_sumtable.reset();
    s.d_cand.reset();
    s.d_toff.reset();
}

int order_sumtables_plan(ulg_ctx *c, const std::string &who, OrderMcmcState &s) {
    const int n = s.n;
    s.tables = false;
    int rc;
    if ((rc = ensure(c, s.d_cand, (size_t)n)) || (rc = ensure(c, s.d_toff, (size_t)n + 1))) return rc;
    prof_begin(c, "ostab_cand");
    ostab_cand_kernel<<<dim3((unsigned)n), kB, 0, c->stream>>>(s.d_sets.p, s.d_offsets.p, s.d_cand.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    s.cand.assign((size_t)n, 0);
    ULG_HIP(c, hipMemcpyAsync(s.cand.data(), s.d_cand.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    s.toff.assign((size_t)n + 1, 0);
    int big = 0;
    for (int v = 0; v < n; ++v) {
        const int K = ot_popcount(s.cand[v]);
        if (K > kTableMaxK) {
            char buf[256];
            std::snprintf(buf, sizeof buf,
                          "%s: option \"mcmc_tables\": variable %d has %d candidate parents, its table would take %.0f bytes; at most %d "
                          "candidates are supported",
                          who.c_str(), v, K, 8.0 * std::ldexp(1.0, K), kTableMaxK);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
        s.toff[v + 1] = s.toff[v] + ot_slots(K);
        if (K > ot_popcount(s.cand[big])) big = v;
    }
    if (s.table_picks) {  // its own count, of every table, stage table and map together, stands for the one below
        if (int rc2 = order_picktables_plan(c, who, s, big)) return rc2;
    }
    // decided before the tables are allocated (an earlier begin's table is reused or replaced)
    size_t free_b = 0, total_b = 0;
    ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const double need = 8.0 * (double)s.toff[n] + 16.0, have = (double)free_b + 8.0 * (double)s.d_sumtable.cap;
    if (!s.table_picks && need > have) {
        char buf[320];
        std::snprintf(buf, sizeof buf,
                      "%s: the tables of option \"mcmc_tables\" need %.0f bytes of device memory (the largest, variable %d's, %.0f), %.0f "
                      "are free",
                      who.c_str(), need, big, 8.0 * (double)(s.toff[big + 1] - s.toff[big]), have);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    ULG_HIP(c, hipMemcpyAsync(s.d_toff.p, s.toff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    return ULG_OK;
}

int order_sumtables_build(ulg_ctx *c, OrderMcmcState &s) {
    const int n = s.n;
    if (int rc = ensure(c, s.d_sumtable, (size_t)s.toff[n])) return rc;
    int Kmax = 0;
    for (int v = 0; v < n; ++v) Kmax = std::max(Kmax, ot_popcount(s.cand[v]));
    const uint64_t *cand = s.d_cand.p;
    const int64_t *toff = s.d_toff.p;
    double *table = s.d_sumtable.p;
    Snap sn{nullptr, nullptr, nullptr};
    if (s.table_picks) {  // allocated by order_picktables_plan
        sn.stage = s.d_stage.p, sn.soff = s.d_soff.p, sn.entry = s.d_entry.p;
    }
    if (Kmax > kTableLdsK) {  // the large tables: cleared, the scores stored, the low rounds by tiles
        prof_begin(c, "ostab_clear");
        ostab_clear_kernel<<<dim3((unsigned)(ot_slots(Kmax) / kB), (unsigned)n), kB, 0, c->stream>>>(cand, toff, table, sn.entry);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
        prof_begin(c, "ostab_scatter");
        ostab_scatter_kernel<<<dim3(64, (unsigned)n), kB, 0, c->stream>>>(s.d_sets.p, s.d_scores.p, s.d_offsets.p, cand, toff, table, sn.entry);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
        prof_begin(c, "ostab_tile");
        ostab_tile_kernel<<<dim3((unsigned)ot_slots(Kmax - kTableLdsK), (unsigned)n), kB, 0, c->stream>>>(cand, toff, table, sn.stage,
                                                                                                                  sn.soff);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
        for (int j = kTableLdsK; j < Kmax; ++j) {  // ... and the high rounds in ascending order, one pass each
            prof_begin(c, "ostab_high");
            ostab_high_kernel<<<dim3((unsigned)(ot_slots(Kmax - 1) / kB), (unsigned)n), kB, 0, c->stream>>>(
                cand, toff, table, j, j % kPickBits == 0 ? sn.stage : nullptr, sn.soff);
            prof_end(c);
            ULG_HIP(c, hipGetLastError());
        }
    }
    prof_begin(c, "ostab_small");
    ostab_small_kernel<<<dim3((unsigned)n), kB, 0, c->stream>>>(s.d_sets.p, s.d_scores.p, s.d_offsets.p, cand, toff, table, sn);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    s.tables = true;
    return ULG_OK;
}

int order_sumtables_terms(ulg_ctx *c, OrderMcmcState &s, int64_t chains) {
    prof_begin(c, "ostab_terms");
    ostab_terms_kernel<<<flat_grid(((uint64_t)chains + kB / kWave - 1) / (kB / kWave)), kB, 0, c->stream>>>(
        s.d_cand.p, s.d_toff.p, s.d_sumtable.p, s.n, s.d_order.p, chains, s.d_terms.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    return ULG_OK;
}

void order_sumtables_run(ulg_ctx *c, const OrderMcmcState &s, const RunArgs &a) {
    ostab_run_kernel<<<dim3((unsigned)((a.chains + kRunWaves - 1) / kRunWaves)), kWave * kRunWaves, 0, c->stream>>>(
        a, s.d_cand.p, s.d_toff.p, s.d_sumtable.p);
}

}  // namespace ulg

extern "C" int ulg_order_mcmc_table(ulg_ctx *c, int v, uint64_t *candidates, int64_t *slots, double *table) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_mcmc_table";
    if (!c->mcmc || !c->mcmc->ready || c->mcmc->rungs) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_mcmc_begin");
    OrderMcmcState &s = *c->mcmc;
    if (!s.tables) return set_err(c, ULG_ERR_STATE, who + ": the chains were begun without option \"mcmc_tables\"");
    if (v < 0 || v >= s.n) return set_err(c, ULG_ERR_ARG, who + ": v out of range");
    const int64_t count = s.toff[v + 1] - s.toff[v];
    if (candidates) *candidates = s.cand[v];
    if (slots) *slots = count;
    if (table) {
        ULG_HIP(c, hipSetDevice(c->device));
        ULG_HIP(c, hipMemcpyAsync(table, s.d_sumtable.p + s.toff[v], (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
        ULG_HIP(c, hipStreamSynchronize(c->stream));
    }
    return ULG_OK;
}
