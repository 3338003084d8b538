// partition_mcmc.hip -- partition MCMC over the per-variable lists
// (ulg_partition_mcmc_begin, ulg_partition_mcmc_begin_from_scores,
// ulg_partition_mcmc_run, ulg_partition_mcmc_state, ulg_partition_score;
// contract: include/ulg.h, "Partition MCMC").  Metropolis-Hastings over ordered
// partitions of the variables (Kuipers & Moffa 2017): a DAG belongs to exactly
// one partition -- its sources, then the sources of what is left, and so on --
// so the DAGs drawn from the chain's states follow prod_v w_v(Pa_v) with no
// linear-extension factor: the prior uniform over DAGs of the stored families.
// Memory is the lists and O(n) per chain, as for the order MCMC, whose device
// copy of the lists (OrderMcmcState) these chains read.
//
// Kernels:
//   part_score_kernel   one wave per (partition, variable): lane u holds u's
//                       part, two ballots give the variable's allowed and
//                       required masks, then the term (ulg_partition_score, and
//                       every chain's terms at begin)
//   part_scan_kernel    one lane per chain: the least (chain, variable) with a
//                       -inf term
//   part_run_kernel<W>  one workgroup of W waves per chain; LDS holds the
//                       state -- part_of[n], the part masks, their exclusive
//                       prefix unions, the n terms by variable -- and the
//                       proposed state beside it:
//     plan      wave 0 forms the step's two draws and the move's plan
//               (part_plan: wave-uniform integer work on the LDS state).  Lane
//               j takes the mask of part j after the move (part_new_mask), a
//               cross-lane prefix-OR gives every new part's allowed set, the
//               neighbour lane's mask its required set; lane v takes v's new
//               part (part_new_index), reads both pairs (A, R) -- the new one
//               by a lane permute, the old one from LDS -- and one ballot is D,
//               the variables whose pair changed.  No loop over n or m: a
//               move changes the number of parts and D is no interval;
//     terms     after a barrier the waves stride D's variables in ascending
//               order; a wave's lanes stride the variable's list (12 B an
//               entry, coalesced), once for the maximum of the eligible
//               scores, once for the integer sum of their weights, reduced
//               across the wave as word pairs with carry (wave_part_term);
//     decision  after a barrier every lane adds the new and the old terms of
//               D ascending, adds ln rho and applies mcmc_accept: the same
//               bits in every lane; barrier; an accepted state is copied,
//               lane = variable / part; barrier;
//     record    at t mod thin = 0: part_of, m, the full sum of the terms and,
//               if asked, a parent set per variable by the sampler's
//               scan-and-ballot pick over the eligible entries.
// A term is an integer sum, a decision a fixed FP64 expression of terms: no
// output depends on W, on the steps per launch or on the number of chains.
// Plain vector stores only; no floating-point atomics, no communication
// between workgroups.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "order_mcmc_state.h"
#include "partition_mcmc_dev.h"

namespace ulg {

// What a context keeps of the partition MCMC beside the order MCMC's state,
// which holds the lists: per chain the part indices, the terms by variable
// and the accepted count, the global step, and the buffers a run's records
// and traces pass through.
struct PartitionMcmcState {
    int n = 0;
    int64_t chains = 0;
    uint64_t seed = 0;
    int64_t step = 0;
    bool ready = false;
    DevBuf<uint8_t> d_part;                 // [chains][n]
    DevBuf<double> d_terms;                 // [chains][n] by variable
    DevBuf<unsigned long long> d_accepted;  // [chains]
    DevBuf<unsigned int> d_err;             // [2]: an error word, the least chain * 64 + variable with a -inf term
    DevBuf<uint8_t> r_part, r_taccept;
    DevBuf<int32_t> r_parts;
    DevBuf<double> r_score, r_weight, r_tdelta;
    DevBuf<uint64_t> r_parents;
    size_t run_bytes() const {
        return r_part.cap + r_taccept.cap + r_parts.cap * 4 + (r_score.cap + r_weight.cap + r_tdelta.cap) * 8 + r_parents.cap * 8;
    }
};

void partition_mcmc_delete(ulg_ctx *c) {
    delete c->pmcmc;
    c->pmcmc = nullptr;
}

void partition_mcmc_end(ulg_ctx *c) {
    if (c->pmcmc) c->pmcmc->ready = false;
}

}  // namespace ulg

using namespace ulg;

namespace {

constexpr int kWave = 64;
constexpr int kB = 256;  // the small kernels' workgroup
constexpr unsigned kErrPick = 8;

constexpr uint64_t kGridX = 1ull << 20;
inline dim3 flat_grid(uint64_t blocks) {
    return dim3((unsigned)std::min<uint64_t>(blocks, kGridX), (unsigned)((blocks + kGridX - 1) / kGridX));
}
__device__ __forceinline__ uint64_t flat_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }
__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

// ---- the term: one wave, every lane returns the same bits
__device__ __forceinline__ double wave_part_term(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t A, uint64_t R,
                                                 int lane) {
    float mx = -__builtin_huge_valf();
    for (int64_t i = b + lane; i < e; i += kWave) {
        const uint64_t S = sets[i];
        const float s = scores[i];
        if (part_eligible(S, A, R)) mx = fmaxf(mx, s);  // float -> double is monotone: the maximum first, converted once
    }
    for (int d = kWave / 2; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, kWave));
    if (!(mx > -__builtin_huge_valf())) return neg_inf();  // scores are finite: no eligible entry
    const double m = (double)mx;
    LxCount T{0, 0};
    for (int64_t i = b + lane; i < e; i += kWave) {
        const uint64_t S = sets[i];
        const float s = scores[i];
        if (part_eligible(S, A, R)) T = lx_add(T, LxCount{post_weight_q((double)s - m), 0});
    }
    for (int d = kWave / 2; d > 0; d >>= 1) {
        LxCount o;
        o.lo = __shfl_xor((unsigned long long)T.lo, d, kWave);
        o.hi = __shfl_xor((unsigned long long)T.hi, d, kWave);
        T = lx_add(T, o);
    }
    return mcmc_term(m, T);
}

// ---- a record's parent set: the sampler's set step over the eligible entries
__device__ __forceinline__ uint64_t wave_scan(uint64_t x, int lane) {
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, d, kWave);
        if (lane >= d) x += y;
    }
    return x;
}
__device__ __forceinline__ int first_above(uint64_t C, uint64_t t) {
    const unsigned long long hit = __ballot(C > t);
    return hit ? __ffsll(hit) - 1 : -1;
}
__device__ __forceinline__ int64_t wave_part_pick(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t A, uint64_t R,
                                                  double a, uint64_t u_set, int lane) {
    auto weigh = [&](int64_t idx) -> uint64_t {
        if (idx >= e) return 0;
        if (!part_eligible(sets[idx], A, R)) return 0;
        return post_weight_q((double)scores[idx] - a);
    };
    if (e - b <= kWave) {
        const uint64_t C = wave_scan(weigh(b + lane), lane);
        const uint64_t t = post_pick_threshold(u_set, __shfl((unsigned long long)C, kWave - 1, kWave));
        const int j = first_above(C, t);
        return j >= 0 ? b + j : -1;
    }
    uint64_t T = 0;
    for (int64_t idx = b + lane; idx < e; idx += kWave) T += weigh(idx);
    for (int s = kWave / 2; s > 0; s >>= 1) T += __shfl_xor((unsigned long long)T, s, kWave);
    const uint64_t t = post_pick_threshold(u_set, T);
    uint64_t base = 0;
    for (int64_t c0 = b; c0 < e; c0 += kWave) {
        const uint64_t C = base + wave_scan(weigh(c0 + lane), lane);
        const int j = first_above(C, t);
        if (j >= 0) return c0 + j;
        base = __shfl((unsigned long long)C, kWave - 1, kWave);
    }
    return -1;
}

// inclusive OR over the lanes 0 .. lane
__device__ __forceinline__ uint64_t wave_prefix_or(uint64_t x, int lane) {
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, d, kWave);
        if (lane >= d) x |= y;
    }
    return x;
}

// terms[k * n + v] of `count` partitions: a wave per (k, v), 4 to a workgroup
__global__ void __launch_bounds__(kB) part_score_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets, int n,
                                                        const uint8_t *parts, int64_t count, double *terms) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t pair = flat_block() * (kB / kWave) + (threadIdx.x >> 6);
    if (pair >= (uint64_t)count * (uint64_t)n) return;  // the whole wave
    const int64_t k = (int64_t)(pair / (uint64_t)n);
    const int v = (int)(pair % (uint64_t)n);
    const uint8_t *row = parts + k * n;
    const int pu = lane < n ? row[lane] : 255, pv = row[v];  // n <= 63: a lane per variable
    const uint64_t A = __ballot(lane < n && pu < pv), R = __ballot(lane < n && pu + 1 == pv);
    const double a = wave_part_term(sets, scores, offsets[v], offsets[v + 1], A, R, lane);
    if (lane == 0) terms[k * n + v] = a;
}

__global__ void __launch_bounds__(kB) part_scan_kernel(const double *terms, int64_t chains, int n, unsigned int *least) {
    const int64_t c = (int64_t)flat_block() * kB + threadIdx.x;
    if (c >= chains) return;
    for (int v = 0; v < n; ++v)
        if (!(terms[c * n + v] > neg_inf())) {
            atomicMin(least, (unsigned int)(c * kWave + v));  // chains <= 2^20
            return;
        }
}

struct PartArgs {
    const uint64_t *sets;
    const float *scores;
    const int64_t *offsets;
    uint8_t *part;                 // [chains][n] the chains' state ...
    double *terms;                 // [chains][n]
    unsigned long long *accepted;  // [chains]
    int n;
    int64_t chains;
    uint64_t seed;
    int64_t t_begin, nsteps;  // the launch makes steps t_begin + 1 .. t_begin + nsteps
    int64_t t_call, thin;     // the call began after step t_call: records and traces are indexed from there
    uint8_t *r_part;          // each may be null
    int32_t *r_parts;
    double *r_score;
    uint64_t *r_parents;
    double *r_weight;
    double *t_delta;
    uint8_t *t_accept;
    unsigned int *err;
};

template <int W>
__global__ void __launch_bounds__(kWave *W) part_run_kernel(const PartArgs a) {
    __shared__ uint8_t part_of[kWave], np[kWave];  // the part of each variable, now and as proposed
    __shared__ uint64_t mask[kWave], pre[kWave];   // part j's variables, and those of the parts before it
    __shared__ uint64_t nmask[kWave], npre[kWave];
    __shared__ double term[kWave], fresh[kWave];   // by variable
    __shared__ double picked[kWave];               // a record's chosen scores, by variable
    __shared__ uint64_t s_D, s_uacc;               // the step's plan, from wave 0 to all
    __shared__ double s_lr;
    __shared__ int s_mnew;                         // -1: a no-op
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int n = a.n;
    const int64_t c = (int64_t)blockIdx.x;  // chains <= 2^20
    if (tid < kWave) {
        part_of[tid] = tid < n ? a.part[c * n + tid] : (uint8_t)255;
        term[tid] = tid < n ? a.terms[c * n + tid] : 0.0;
    }
    __syncthreads();
    int m = lane < n ? part_of[lane] + 1 : 0;  // the number of parts, the same in every lane
    for (int d = kWave / 2; d > 0; d >>= 1) m = max(m, __shfl_xor(m, d, kWave));
    if (wave == 0) {  // once per launch: a ballot per part
        uint64_t mine = 0;
        for (int j = 0; j < m; ++j) {
            const uint64_t b = __ballot(lane < n && part_of[lane] == j);
            if (lane == j) mine = b;
        }
        mask[lane] = mine;
        pre[lane] = wave_prefix_or(mine, lane) ^ mine;  // the parts are disjoint
    }
    unsigned long long acc = a.accepted[c];
    __syncthreads();
    for (int64_t s = 0; s < a.nsteps; ++s) {
        const int64_t t = a.t_begin + s + 1;
        if (wave == 0) {
            uint32_t w[4], x[4];
            mcmc_draw(a.seed, (uint64_t)t, (uint32_t)c, 0u, w);
            mcmc_draw(a.seed, (uint64_t)t, (uint32_t)c, kPartAuxDomain, x);
            const PartPlan pl = part_plan(w, (uint64_t)x[2] | ((uint64_t)x[3] << 32), n, m, part_of, mask);
            uint64_t D = 0;
            if (!pl.noop) {
                const int p = lane < n ? part_of[lane] : 0;
                const int q = lane < n ? part_new_index(pl, lane, p) : 0;
                const uint64_t nb = lane < pl.m_new ? part_new_mask(pl, lane, mask) : 0ull;
                const uint64_t before = wave_prefix_or(nb, lane) ^ nb;
                uint64_t below = __shfl_up((unsigned long long)nb, 1, kWave);  // the required set of part `lane`
                if (lane == 0) below = 0;
                const uint64_t A2 = __shfl((unsigned long long)before, q, kWave), R2 = __shfl((unsigned long long)below, q, kWave);
                const uint64_t A1 = pre[p], R1 = p ? mask[p - 1] : 0ull;
                D = __ballot(lane < n && (A1 != A2 || R1 != R2));
                np[lane] = (uint8_t)q;
                nmask[lane] = nb;
                npre[lane] = before;
            }
            if (lane == 0) {
                s_D = D;
                s_uacc = (uint64_t)x[0] | ((uint64_t)x[1] << 32);
                s_lr = pl.noop ? 0.0 : part_log_rho(pl);
                s_mnew = pl.noop ? -1 : pl.m_new;
            }
        }
        __syncthreads();
        const int m_new = s_mnew;
        const uint64_t D = s_D;
        double delta = neg_inf();
        bool take = false;
        if (m_new >= 0) {
            int at = 0;
            for (uint64_t rest = D; rest; rest &= rest - 1, ++at) {
                if (at % W != wave) continue;
                const int v = __builtin_ctzll(rest), q = np[v];
                const double x = wave_part_term(a.sets, a.scores, a.offsets[v], a.offsets[v + 1], npre[q], q ? nmask[q - 1] : 0ull, lane);
                if (lane == 0) fresh[v] = x;
            }
            __syncthreads();
            double now = 0.0, was = 0.0;
            bool none = false;
            for (uint64_t rest = D; rest; rest &= rest - 1) {
                const int v = __builtin_ctzll(rest);
                const double x = fresh[v];
                none = none || !(x > neg_inf());
                now += x;
                was += term[v];
            }
            if (!none) delta = (now - was) + s_lr;
            take = mcmc_accept(delta, s_uacc);
            __syncthreads();  // every lane has read the old terms
            if (take) {
                if (tid < kWave) {
                    if (tid < n) part_of[tid] = np[tid];
                    if ((D >> tid) & 1ull) term[tid] = fresh[tid];
                    mask[tid] = nmask[tid];
                    pre[tid] = npre[tid];
                }
                m = m_new;
                ++acc;
            }
        }
        __syncthreads();  // the state stands, and the plan's words are free for the next step
        if (tid == 0) {
            const int64_t at = (t - a.t_call - 1) * a.chains + c;
            if (a.t_delta) a.t_delta[at] = delta;
            if (a.t_accept) a.t_accept[at] = take ? 1 : 0;
        }
        if (t % a.thin == 0) {
            const int64_t idx = (t / a.thin - a.t_call / a.thin - 1) * a.chains + c;
            if (a.r_part && tid < n) a.r_part[idx * n + tid] = part_of[tid];
            if (a.r_parts && tid == 0) a.r_parts[idx] = m;
            if (a.r_score && tid == 0) {
                double sum = 0.0;
                for (int v = 0; v < n; ++v) sum += term[v];
                a.r_score[idx] = sum;
            }
            if (a.r_parents) {
                for (int v = wave; v < n; v += W) {
                    uint32_t w[4];
                    mcmc_draw(a.seed, (uint64_t)t, (uint32_t)c, (uint32_t)(1 + v), w);
                    const uint64_t u_set = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
                    const int q = part_of[v];
                    const int64_t e = wave_part_pick(a.sets, a.scores, a.offsets[v], a.offsets[v + 1], pre[q], q ? mask[q - 1] : 0ull,
                                                     term[v], u_set, lane);
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
        a.part[c * n + tid] = part_of[tid];
        a.terms[c * n + tid] = term[tid];
    }
    if (tid == 0) a.accepted[c] = acc;
}

// ---- host
bool is_partition(const uint8_t *row, int n) {
    uint64_t mask[kMcmcMaxVars];
    return part_masks(n, row, mask) > 0;
}

int launch_score(ulg_ctx *c, const OrderMcmcState &l, const uint8_t *d_parts, int64_t count, double *d_terms) {
    const uint64_t pairs = (uint64_t)count * (uint64_t)l.n;
    prof_begin(c, "partition_score");
    part_score_kernel<<<flat_grid((pairs + kB / kWave - 1) / (kB / kWave)), kB, 0, c->stream>>>(l.d_sets.p, l.d_scores.p, l.d_offsets.p,
                                                                                               l.n, d_parts, count, d_terms);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    return ULG_OK;
}

int check_init(ulg_ctx *c, const std::string &who, int n, int64_t chains, const uint8_t *init_part) {
    if (!init_part || n < 1 || n > kMcmcMaxVars || chains < 1 || chains > kMcmcMaxChains) return ULG_OK;  // the lists' loader refuses
    for (int64_t k = 0; k < chains; ++k)
        if (!is_partition(init_part + k * n, n))
            return set_err(c, ULG_ERR_ARG, who + ": the initial partition of chain " + std::to_string(k) + " does not use exactly the parts 0 .. m-1");
    return ULG_OK;
}

// The lists stand checked in c->mcmc: the chains' parts and terms.
int begin(ulg_ctx *c, const std::string &who, int64_t chains, uint64_t seed, const uint8_t *init_part) {
    const OrderMcmcState &l = *c->mcmc;
    const int n = l.n;
    if (!c->pmcmc) c->pmcmc = new PartitionMcmcState();
    PartitionMcmcState &s = *c->pmcmc;
    s.ready = false;
    int rc;
    if ((rc = ensure(c, s.d_err, 2)) || (rc = ensure(c, s.d_part, (size_t)(chains * n))) ||
        (rc = ensure(c, s.d_terms, (size_t)(chains * n))) || (rc = ensure(c, s.d_accepted, (size_t)chains)))
        return rc;
    static const unsigned int err0[2] = {0u, 0xFFFFFFFFu};  // static: the copy's source outlives every return
    ULG_HIP(c, hipMemcpyAsync(s.d_err.p, err0, sizeof err0, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemsetAsync(s.d_accepted.p, 0, (size_t)chains * 8, c->stream));
    if (init_part) {
        ULG_HIP(c, hipMemcpyAsync(s.d_part.p, init_part, (size_t)(chains * n), hipMemcpyHostToDevice, c->stream));
        ULG_HIP(c, hipStreamSynchronize(c->stream));  // init_part is the caller's again, whatever returns below
    } else {
        ULG_HIP(c, hipMemsetAsync(s.d_part.p, 0, (size_t)(chains * n), c->stream));  // every variable in part 0: the empty DAG
    }
    if ((rc = launch_score(c, l, s.d_part.p, chains, s.d_terms.p))) return rc;
    prof_begin(c, "partition_scan");
    part_scan_kernel<<<flat_grid(((uint64_t)chains + kB - 1) / kB), kB, 0, c->stream>>>(s.d_terms.p, chains, n, s.d_err.p + 1);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    unsigned int err[2] = {0, 0};
    ULG_HIP(c, hipMemcpyAsync(err, s.d_err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (err[1] != 0xFFFFFFFFu)
        return set_err(c, ULG_ERR_ARG,
                       who + ": in the initial partition of chain " + std::to_string(err[1] / kWave) + " variable " +
                           std::to_string(err[1] % kWave) + " has no eligible stored parent set (a term of -inf: probability 0" +
                           (init_part ? ")" : "; without init_part every variable needs the empty set)"));
    s.n = n;
    s.chains = chains;
    s.seed = seed;
    s.step = 0;
    s.ready = true;
    return ULG_OK;
}

template <int W>
void launch_run(ulg_ctx *c, const PartArgs &a) {
    part_run_kernel<W><<<dim3((unsigned)a.chains), kWave * W, 0, c->stream>>>(a);
}

PartitionMcmcState *live(ulg_ctx *c) { return c->pmcmc && c->pmcmc->ready && c->mcmc ? c->pmcmc : nullptr; }

}  // namespace

extern "C" {

int ulg_partition_mcmc_begin(ulg_ctx *c, int n, const int64_t *offsets, const uint64_t *sets, const float *scores, int device_ptrs,
                             int64_t chains, uint64_t seed, const uint8_t *init_part) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_partition_mcmc_begin";
    partition_mcmc_end(c);  // a begin that is refused, for whatever reason, leaves no chains of any family
    order_search_end(c);
    if (c->mcmc) c->mcmc->ready = false;
    if (int rc = check_init(c, who, n, chains, init_part)) return rc;
    if (int rc = order_mcmc_take_lists(c, who, n, offsets, sets, scores, device_ptrs, chains)) return rc;
    return begin(c, who, chains, seed, init_part);
}

int ulg_partition_mcmc_begin_from_scores(ulg_ctx *c, int64_t chains, uint64_t seed, const uint8_t *init_part) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_partition_mcmc_begin_from_scores";
    partition_mcmc_end(c);
    order_search_end(c);
    if (c->mcmc) c->mcmc->ready = false;
    if (int rc = check_init(c, who, c->n, chains, init_part)) return rc;
    if (int rc = order_mcmc_take_scored(c, who, chains)) return rc;
    return begin(c, who, chains, seed, init_part);
}

int ulg_partition_mcmc_run(ulg_ctx *c, int64_t steps, int64_t thin, uint8_t *part, int32_t *parts, double *log_score, uint64_t *parents,
                           double *log_weight, int64_t *accepted, double *trace_delta, uint8_t *trace_accept, int64_t *records) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_partition_mcmc_run";
    if (!live(c)) return set_err(c, ULG_ERR_STATE, who + ": no ulg_partition_mcmc_begin");
    PartitionMcmcState &s = *c->pmcmc;
    const OrderMcmcState &l = *c->mcmc;
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
        const double need = cells * ((part ? n : 0) + (parts ? 4.0 : 0.0) + (log_score ? 8.0 : 0.0) + (parents ? 8.0 * n : 0.0) +
                                     (log_weight ? 8.0 : 0.0)) +
                            moves * ((trace_delta ? 8.0 : 0.0) + (trace_accept ? 1.0 : 0.0)) + 7 * 16.0 + 256.0;
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
    if ((part && (rc = ensure(c, s.r_part, ncell * n))) || (parts && (rc = ensure(c, s.r_parts, ncell))) ||
        (log_score && (rc = ensure(c, s.r_score, ncell))) || (parents && (rc = ensure(c, s.r_parents, ncell * n))) ||
        (log_weight && (rc = ensure(c, s.r_weight, ncell))) || (trace_delta && (rc = ensure(c, s.r_tdelta, nmove))) ||
        (trace_accept && (rc = ensure(c, s.r_taccept, nmove))))
        return rc;
    ULG_HIP(c, hipMemsetAsync(s.d_err.p, 0, sizeof(unsigned int), c->stream));
    PartArgs a;
    a.sets = l.d_sets.p, a.scores = l.d_scores.p, a.offsets = l.d_offsets.p;
    a.part = s.d_part.p, a.terms = s.d_terms.p, a.accepted = s.d_accepted.p;
    a.n = n, a.chains = chains, a.seed = s.seed;
    a.t_call = t0, a.thin = thin;
    a.r_part = part ? s.r_part.p : nullptr;
    a.r_parts = parts ? s.r_parts.p : nullptr;
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
        prof_begin(c, "partition_run");
        switch (c->opt.mcmc_waves) {
            case 1: launch_run<1>(c, a); break;
            case 2: launch_run<2>(c, a); break;
            case 8: launch_run<8>(c, a); break;
            default: launch_run<4>(c, a); break;
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
    if (part && ncell) ULG_HIP(c, hipMemcpyAsync(part, s.r_part.p, ncell * n, hipMemcpyDeviceToHost, c->stream));
    if (parts && ncell) ULG_HIP(c, hipMemcpyAsync(parts, s.r_parts.p, ncell * 4, hipMemcpyDeviceToHost, c->stream));
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

int ulg_partition_mcmc_state(ulg_ctx *c, uint8_t *part, double *terms, int64_t *step) {
    if (!c) return ULG_ERR_ARG;
    if (!live(c)) return set_err(c, ULG_ERR_STATE, "ulg_partition_mcmc_state: no ulg_partition_mcmc_begin");
    PartitionMcmcState &s = *c->pmcmc;
    const size_t cells = (size_t)s.chains * (size_t)s.n;
    ULG_HIP(c, hipSetDevice(c->device));
    if (part) ULG_HIP(c, hipMemcpyAsync(part, s.d_part.p, cells, hipMemcpyDeviceToHost, c->stream));
    if (terms) ULG_HIP(c, hipMemcpyAsync(terms, s.d_terms.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    if (step) *step = s.step;
    return ULG_OK;
}

int ulg_partition_score(ulg_ctx *c, int64_t count, const uint8_t *part, double *terms) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_partition_score";
    if (!live(c)) return set_err(c, ULG_ERR_STATE, who + ": no ulg_partition_mcmc_begin");
    PartitionMcmcState &s = *c->pmcmc;
    const int n = s.n;
    if (count < 0 || (count > 0 && (!part || !terms))) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
    if (count > (int64_t)1 << 40) return set_err(c, ULG_ERR_ARG, who + ": count out of range");
    for (int64_t k = 0; k < count; ++k)
        if (!is_partition(part + k * n, n))
            return set_err(c, ULG_ERR_ARG, who + ": partition " + std::to_string(k) + " does not use exactly the parts 0 .. m-1");
    if (count == 0) return ULG_OK;
    ULG_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)count * (size_t)n;
    {
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        const double need = 9.0 * (double)cells + 2 * 16.0 + 256.0, have = (double)free_b + (double)s.run_bytes();
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld partitions of n = %d need %.0f bytes of device memory, %.0f are free", who.c_str(),
                          (long long)count, n, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    int rc;
    if ((rc = ensure(c, s.r_part, cells)) || (rc = ensure(c, s.r_score, cells))) return rc;
    ULG_HIP(c, hipMemcpyAsync(s.r_part.p, part, cells, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_score(c, *c->mcmc, s.r_part.p, count, s.r_score.p))) return rc;
    ULG_HIP(c, hipMemcpyAsync(terms, s.r_score.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ULG_OK;
}

}  // extern "C"
