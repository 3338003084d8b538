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
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "order_mcmc_dev.h"
#include "order_mcmc_state.h"

namespace ulg {

void order_mcmc_delete(ulg_ctx *c) {
    delete c->mcmc;
    c->mcmc = nullptr;
}

}  // namespace ulg

using namespace ulg;

namespace {

constexpr int kWave = 64;
constexpr int kB = 256;  // the small kernels' workgroup

// bits of the error word (d_err[0]); d_err[1] = the least chain with a -inf term
constexpr unsigned kErrSet = 1, kErrScore = 2, kErrDup = 4, kErrPick = 8;

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

// ---- a record's parent set: the sampler's set step (posterior_sample.hip)
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
// The entry of [b, e) chosen by u_set among those within U, weights
// floor(exp((double) s - a) 2^52); -1 when every weight is 0 (wave-uniform)
__device__ __forceinline__ int64_t wave_pick(const uint64_t *sets, const float *scores, int64_t b, int64_t e, uint64_t U, double a,
                                             uint64_t u_set, int lane) {
    const uint64_t outside = ~U;
    auto weigh = [&](int64_t idx) -> uint64_t {
        if (idx >= e) return 0;
        if (sets[idx] & outside) return 0;
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

struct RunArgs {
    const uint64_t *sets;
    const float *scores;
    const int64_t *offsets;
    uint8_t *order;                 // [chains][n] the chains' state ...
    double *terms;                  // [chains][n]
    unsigned long long *accepted;   // [chains]
    int n;
    int64_t chains;
    uint64_t seed;
    int64_t t_begin, nsteps;  // the launch makes steps t_begin + 1 .. t_begin + nsteps
    int64_t t_call, thin;     // the call began after step t_call: records and traces are indexed from there
    uint8_t *r_order;         // each may be null
    double *r_score;
    uint64_t *r_parents;
    double *r_weight;
    double *t_delta;
    uint8_t *t_accept;
    unsigned int *err;
};

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
int check_begin_args(ulg_ctx *c, const std::string &who, int n, int64_t chains, const uint8_t *init_order) {
    if (n < 1) return set_err(c, ULG_ERR_ARG, who + ": n < 1");
    if (n > kMcmcMaxVars) return set_err(c, ULG_ERR_UNSUPPORTED, who + ": n = " + std::to_string(n) + "; at most 63 variables");
    if (chains < 1 || chains > kMcmcMaxChains) return set_err(c, ULG_ERR_ARG, who + ": chains must be 1..2^20");
    if (init_order)
        for (int64_t k = 0; k < chains; ++k)
            if (!is_permutation(init_order + k * n, n))
                return set_err(c, ULG_ERR_ARG, who + ": the initial order of chain " + std::to_string(k) + " is not a permutation");
    return ULG_OK;
}

// Lists and chains beyond the free device memory (what the state already
// holds counts as free: its buffers are reused or replaced).  Nothing has
// been allocated yet.
int refuse_size(ulg_ctx *c, const std::string &who, int n, int64_t total, int64_t chains) {
    size_t free_b = 0, total_b = 0;
    ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const double need = 12.0 * (double)total + 8.0 * (n + 1) + 8.0 * (double)table_slots(total) + (9.0 * n + 8.0) * (double)chains + 8.0 * 16 + 256.0;
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
int begin(ulg_ctx *c, const std::string &who, OrderMcmcState &s, int64_t chains, uint64_t seed, const uint8_t *init_order) {
    const std::vector<int64_t> &offs = s.offsets;
    const int n = s.n;
    s.ready = false;
    DevBuf<unsigned long long> table;  // the call's own
    const uint64_t slots = table_slots(s.total);
    int rc;
    if ((rc = ensure(c, table, (size_t)slots)) || (rc = ensure(c, s.d_err, 2)) || (rc = ensure(c, s.d_order, (size_t)(chains * n))) ||
        (rc = ensure(c, s.d_terms, (size_t)(chains * n))) || (rc = ensure(c, s.d_accepted, (size_t)chains)))
        return rc;
    static const unsigned int err0[2] = {0u, 0xFFFFFFFFu};  // static: the copy's source outlives every return
    ULG_HIP(c, hipMemcpyAsync(s.d_err.p, err0, sizeof err0, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemsetAsync(table.p, 0, (size_t)slots * 8, c->stream));
    ULG_HIP(c, hipMemsetAsync(s.d_accepted.p, 0, (size_t)chains * 8, c->stream));
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
    if (init_order) {
        ULG_HIP(c, hipMemcpyAsync(s.d_order.p, init_order, (size_t)(chains * n), hipMemcpyHostToDevice, c->stream));
        ULG_HIP(c, hipStreamSynchronize(c->stream));  // init_order is the caller's again, whatever returns below
    } else {
        prof_begin(c, "mcmc_shuffle");
        mcmc_shuffle_kernel<<<flat_grid(((uint64_t)chains + kB - 1) / kB), kB, 0, c->stream>>>(s.d_order.p, chains, n, seed);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    if ((rc = launch_score(c, s, s.d_order.p, chains, s.d_terms.p))) return rc;
    prof_begin(c, "mcmc_scan");
    mcmc_scan_kernel<<<flat_grid(((uint64_t)chains + kB - 1) / kB), kB, 0, c->stream>>>(s.d_terms.p, chains, n, s.d_err.p + 1);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    ULG_HIP(c, hipMemcpyAsync(err, s.d_err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (err[1] != 0xFFFFFFFFu)
        return set_err(c, ULG_ERR_ARG,
                       who + ": the initial order of chain " + std::to_string(err[1]) +
                           " has a variable without a stored parent set among its predecessors (a term of -inf: probability 0)");
    s.chains = chains;
    s.seed = seed;
    s.step = 0;
    s.ready = true;
    return ULG_OK;
}

template <int W>
void launch_run(ulg_ctx *c, const RunArgs &a) {
    mcmc_run_kernel<W><<<dim3((unsigned)a.chains), kWave * W, 0, c->stream>>>(a);
}

}  // namespace

extern "C" {

int ulg_order_mcmc_begin(ulg_ctx *c, int n, const int64_t *offsets, const uint64_t *sets, const float *scores, int device_ptrs,
                         int64_t chains, uint64_t seed, const uint8_t *init_order) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_mcmc_begin";
    if (c->mcmc) c->mcmc->ready = false;  // a begin that is refused, for whatever reason, leaves no chains
    if (!offsets) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
    if (int rc = check_begin_args(c, who, n, chains, init_order)) return rc;
    for (int v = 0; v < n; ++v)
        if (offsets[v + 1] < offsets[v]) return set_err(c, ULG_ERR_ARG, who + ": offsets not ascending");
    const int64_t total = offsets[n] - offsets[0];
    if (total && (!sets || !scores)) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
    ULG_HIP(c, hipSetDevice(c->device));
    if (int rc = refuse_size(c, who, n, total, chains)) return rc;
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
    return begin(c, who, s, chains, seed, init_order);
}

int ulg_order_mcmc_begin_from_scores(ulg_ctx *c, int64_t chains, uint64_t seed, const uint8_t *init_order) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_mcmc_begin_from_scores";
    if (c->mcmc) c->mcmc->ready = false;  // as ulg_order_mcmc_begin
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
    if (int rc = check_begin_args(c, who, n, chains, init_order)) return rc;
    ULG_HIP(c, hipSetDevice(c->device));
    std::vector<int64_t> src((size_t)n + 1);
    ULG_HIP(c, hipMemcpyAsync(src.data(), c->out_offsets.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t total = src[n];
    if (int rc = refuse_size(c, who, n, total, chains)) return rc;
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
    return begin(c, who, s, chains, seed, init_order);
}

int ulg_order_mcmc_run(ulg_ctx *c, int64_t steps, int64_t thin, uint8_t *order, double *log_score, uint64_t *parents,
                       double *log_weight, int64_t *accepted, double *trace_delta, uint8_t *trace_accept, int64_t *records) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_mcmc_run";
    if (!c->mcmc || !c->mcmc->ready) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_mcmc_begin");
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
        prof_begin(c, "mcmc_run");
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
    if (!c->mcmc || !c->mcmc->ready) return set_err(c, ULG_ERR_STATE, "ulg_order_mcmc_state: no ulg_order_mcmc_begin");
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

}  // extern "C"
