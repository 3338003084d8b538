// order_picktables.hip -- order MCMC over the log-sum tables with a record's
// DAG drawn from the tables too (option "mcmc_table_picks",
// ulg_order_mcmc_stage_table; contract: include/ulg.h, "Order MCMC: a record's
// DAG from the tables"; arithmetic: order_picktables_dev.h).  The ascending
// butterfly that builds L_v passes, before round 6 c, through the conditional
// log-sums a descent needs that fixes the picked set's index bits from the top,
// six at a time: the build kernels of order_sumtables.hip keep those images
// (the stage tables S_{v,c}) and an entry map E_v, and a pick is nch_v <= 5
// dependent gather rounds of one wave64 -- lane l is the pattern l of the six
// bits -- where the list pick strides over the whole list twice.
//
//   opick_run_kernel   a copy of ostab_run_kernel (the step loop word for
//                      word, so that the option-off kernel keeps its code): one
//                      wave per chain, four chains to a workgroup, no barrier,
//                      no LDS, no scratch.  A record's picks:
//     state    lane p keeps its position's fixed bits and a_cur (3 VGPRs);
//     levels   outermost, c = 4 .. 0; a level with no position in it is
//              skipped.  The n picks of a level are independent: positions go
//              in groups of kGroup = 4, whose gathers -- one slot per lane and
//              position -- are all issued before the first is weighed (4 loads
//              of 8 B in flight per lane; at level 0 four of E, then four of
//              the scores), so a record waits for about n nch / 4 gather
//              latencies, not n nch;
//     a pick   per level: post_weight_q of the lane's value, the scan across
//              the wave, the threshold from the level's own draw (domain
//              1 + p + 64 c), the first lane above it, a lane read of its
//              value as the next a_cur;
//     entry    after level 0 every lane looks up E at its own fixed bits: one
//              gather for all n positions, then the set and the score.
// Hosts the plan (sizes and the memory check), the drop, the launch and the
// tests' read-back.  Plain vector stores only.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "order_picktables_dev.h"
#include "order_sumtables_wave.h"

using namespace ulg;

namespace {

constexpr int kGroup = 4;             // positions whose gathers are in flight together
constexpr uint32_t kDead = ~0u;       // a position whose level found no weight: no lower level, no entry

struct PickArgs {
    const double *stage;
    const int64_t *soff;
    const int32_t *entry;
};

// What lane p keeps of its position's pick, and what every lane reads of it
struct PickLane {
    int K;
    uint32_t x, fixed;
    int64_t base, sbase, lbase;  // the first slot of E_v (and L_v), of S_{v,1}, the first list entry
    double a_cur;
};

// Level c of the positions p0 .. p0 + kGroup - 1 (below n).  LEAF: c = 0, the
// values are the stored scores behind E; else the stage table's slots.
template <bool LEAF>
__device__ __forceinline__ void pick_level(const RunArgs &a, const PickArgs &pk, PickLane &me, int c, int p0, int n, uint64_t t,
                                           uint32_t chain, int lane) {
    double val[kGroup];
    bool live[kGroup];
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {  // the gathers: every address is inside its buffer, whether the lane counts or not
        const int p = p0 + g < n ? p0 + g : n - 1;
        const int K = lane_get(me.K, p);
        const uint32_t x = (uint32_t)lane_get((int)me.x, p), fixed = (uint32_t)lane_get((int)me.fixed, p);
        live[g] = p0 + g < n && fixed != kDead && c < opt_chunks(K);
        const bool lane_on = live[g] && opt_lane_on(K, x, c, lane);
        const uint32_t slot = opt_slot(fixed, x, c, lane);
        if (LEAF) {
            const int64_t base = (int64_t)lane_get64((uint64_t)me.base, p), lbase = (int64_t)lane_get64((uint64_t)me.lbase, p);
            const int32_t e = pk.entry[lane_on ? base + slot : 0];
            const bool has = lane_on && e >= 0;
            const float sc = a.scores[has ? lbase + e : 0];
            val[g] = has ? (double)sc : neg_inf();
        } else {
            const int64_t sbase = (int64_t)lane_get64((uint64_t)me.sbase, p);
            const double s = pk.stage[lane_on ? sbase + (((int64_t)(c - 1)) << K) + slot : 0];
            val[g] = lane_on ? s : neg_inf();
        }
    }
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
        if (!live[g]) continue;  // wave-uniform
        const int p = p0 + g;
        const uint64_t C = wave_scan(post_weight_q(val[g] - lane_getd(me.a_cur, p)), lane);  // -inf - a = -inf: weight 0
        const uint64_t T = __shfl((unsigned long long)C, kWave - 1, kWave);
        uint32_t w[4];
        mcmc_draw(a.seed, t, chain, 1u + (uint32_t)p + kPickDomain * (uint32_t)c, w);
        const int j = first_above(C, post_pick_threshold((uint64_t)w[0] | ((uint64_t)w[1] << 32), T));
        if (j < 0) {  // T = 0
            if (lane == p) me.fixed = kDead;
        } else {
            const double chosen = lane_getd(val[g], j);
            if (lane == p) me.fixed |= (uint32_t)j << (kPickBits * c), me.a_cur = chosen;
        }
    }
}

__global__ void __launch_bounds__(kWave *kRunWaves) opick_run_kernel(const RunArgs a, const uint64_t *cand, const int64_t *toff,
                                                                      const double *table, const PickArgs pk) {
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
        if (n > 1) {  // the step of ostab_run_kernel
            uint32_t w[4];
            mcmc_draw(a.seed, (uint64_t)t, (uint32_t)c, 0u, w);
            const McmcMove mv = mcmc_move(w, n);
            const int lo = mv.i < mv.j ? mv.i : mv.j, hi = mv.i < mv.j ? mv.j : mv.i;
            const int va = lane_get(v, lo), vb = lane_get(v, hi);
            const uint64_t flip = (1ull << va) ^ (1ull << vb);
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
                PickLane me;
                me.K = ot_popcount(pl.C), me.x = pl.idx, me.fixed = 0, me.a_cur = term;
                me.base = pl.base, me.sbase = on ? pk.soff[v] : 0, me.lbase = on ? a.offsets[v] : 0;
                const int nch = opt_chunks(me.K);
                for (int lv = kPickMaxChunks - 1; lv >= 1; --lv) {
                    if (!__ballot(on && nch > lv)) continue;  // no table this deep in the order's variables
                    for (int p0 = 0; p0 < n; p0 += kGroup) pick_level<false>(a, pk, me, lv, p0, n, (uint64_t)t, (uint32_t)c, lane);
                }
                for (int p0 = 0; p0 < n; p0 += kGroup) pick_level<true>(a, pk, me, 0, p0, n, (uint64_t)t, (uint32_t)c, lane);
                // the entries: every lane its own position's
                double got = 0.0;  // lane p: the chosen score of the variable at position p
                if (on) {
                    const int32_t e = me.fixed != kDead ? pk.entry[me.base + me.fixed] : -1;  // >= 0: the chosen lane's weight was positive
                    if (e < 0) {
                        atomicOr(a.err, kErrPick);  // as on the lists: the term is within rounding of ln of the weights' sum
                        a.r_parents[idx * n + v] = 0;
                    } else {
                        a.r_parents[idx * n + v] = a.sets[me.lbase + e];
                        got = (double)a.scores[me.lbase + e];
                    }
                }
                if (a.r_weight) {
                    double picked = 0.0;  // lane u: the chosen score of variable u
                    for (int p = 0; p < n; ++p) {
                        const int u = lane_get(v, p);
                        const double x = lane_getd(got, p);
                        if (lane == u) picked = x;
                    }
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

void order_picktables_drop(OrderMcmcState &s) {
    s.table_picks = false;
    s.d_soff.reset();
    s.d_stage.reset();
    s.d_entry.reset();
}

int order_picktables_plan(ulg_ctx *c, const std::string &who, OrderMcmcState &s, int big) {
    const int n = s.n;
    s.soff.assign((size_t)n + 1, 0);
    double need = 8.0 * (n + 1) + 32.0;
    for (int v = 0; v < n; ++v) {
        if (s.offsets[v + 1] - s.offsets[v] > INT32_MAX) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: option \"mcmc_table_picks\": variable %d lists %lld sets, the entry map holds at most 2^31 - 1",
                          who.c_str(), v, (long long)(s.offsets[v + 1] - s.offsets[v]));
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
        const int K = ot_popcount(s.cand[v]);
        s.soff[v + 1] = s.soff[v] + (int64_t)(opt_chunks(K) - 1) * ot_slots(K);
        need += opt_bytes(K, true);
    }
    // decided before any of the tables is allocated (an earlier begin's are reused or replaced)
    size_t free_b = 0, total_b = 0;
    ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const double have = (double)free_b + 8.0 * (double)(s.d_sumtable.cap + s.d_stage.cap + s.d_soff.cap) + 4.0 * (double)s.d_entry.cap;
    if (need > have) {
        char buf[360];
        std::snprintf(buf, sizeof buf,
                      "%s: the tables of options \"mcmc_tables\" and \"mcmc_table_picks\" need %.0f bytes of device memory (the largest, "
                      "variable %d's, %.0f), %.0f are free",
                      who.c_str(), need, big, opt_bytes(ot_popcount(s.cand[big]), true), have);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    int rc;
    if ((rc = ensure(c, s.d_soff, (size_t)n + 1)) || (rc = ensure(c, s.d_stage, (size_t)std::max<int64_t>(s.soff[n], 1))) ||
        (rc = ensure(c, s.d_entry, (size_t)s.toff[n])))
        return rc;
    ULG_HIP(c, hipMemcpyAsync(s.d_soff.p, s.soff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    return ULG_OK;
}

void order_picktables_run(ulg_ctx *c, const OrderMcmcState &s, const RunArgs &a) {
    const PickArgs pk{s.d_stage.p, s.d_soff.p, s.d_entry.p};
    opick_run_kernel<<<dim3((unsigned)((a.chains + kRunWaves - 1) / kRunWaves)), kWave * kRunWaves, 0, c->stream>>>(
        a, s.d_cand.p, s.d_toff.p, s.d_sumtable.p, pk);
}

}  // namespace ulg

extern "C" int ulg_order_mcmc_stage_table(ulg_ctx *c, int v, int stage, int64_t *slots, double *table, int32_t *entries) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_mcmc_stage_table";
    if (!c->mcmc || !c->mcmc->ready || c->mcmc->rungs) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_mcmc_begin");
    OrderMcmcState &s = *c->mcmc;
    if (!s.tables || !s.table_picks) return set_err(c, ULG_ERR_STATE, who + ": the chains were begun without option \"mcmc_table_picks\"");
    if (v < 0 || v >= s.n) return set_err(c, ULG_ERR_ARG, who + ": v out of range");
    const int64_t count = s.toff[v + 1] - s.toff[v];
    const int nch = opt_chunks(ot_popcount(s.cand[v]));
    if (stage < 0 || stage > nch - 1) return set_err(c, ULG_ERR_ARG, who + ": stage out of range");
    if (slots) *slots = count;
    ULG_HIP(c, hipSetDevice(c->device));
    if (stage >= 1 && table)
        ULG_HIP(c, hipMemcpyAsync(table, s.d_stage.p + s.soff[v] + (int64_t)(stage - 1) * count, (size_t)count * 8, hipMemcpyDeviceToHost,
                                  c->stream));
    if (stage == 0 && entries)
        ULG_HIP(c, hipMemcpyAsync(entries, s.d_entry.p + s.toff[v], (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    return ULG_OK;
}
