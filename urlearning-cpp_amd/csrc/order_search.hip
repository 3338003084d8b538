// order_search.hip -- order-space tabu search over the per-variable lists
// (ulg_order_search_begin, ulg_order_search_begin_from_scores,
// ulg_order_search_run, ulg_order_search_state, ulg_order_best; contract:
// include/ulg.h, "Order search").  Teyssier & Koller's search: an order's score
// is the sum over its positions of the best stored parent set inside the
// predecessors -- the max-plus twin of the order MCMC's term -- and a step
// takes the best admissible swap of two neighbours.  Memory is the lists (the
// order MCMC's device copy, OrderMcmcState) and O(n^2) per search.
//
// Kernels:
//   osearch_shuffle_kernel   one lane per search: the initial order
//   osearch_best_kernel      one wave per (order, position): b and its entry
//                            (ulg_order_best, and every search's terms at begin)
//   osearch_init_kernel      one lane per search: S, the best-so-far, the counts,
//                            the least search with a -inf term
//   osearch_parents_kernel   one lane per (search, position): the best order's
//                            entries as parent masks by variable
//   osearch_run_kernel<W>    one workgroup of W waves per search, all steps of
//                            the launch.  LDS: the order, the predecessor masks,
//                            term[p] and its entry, for every swap p the two
//                            terms it would give (c0, c1) and their entries,
//                            the best order and its entries, the pair stamps
//                            [n][n].  S, S_best and the idle count are the same
//                            bits in every lane's registers.
//     select   every wave alike, lane p = swap p: gain_p from the four cached
//              terms (os_gain), the pair's stamp by the two variables' indices,
//              admissibility; the gain's 64-bit image is max-reduced across the
//              lanes, a ballot of the equal lanes and a find-first give the
//              least p.  No loop over n, no broadcast through LDS.  The wave
//              reads what its scan needs of the state as it stands; barrier;
//     move     one lane trades term[p], term[p+1] with c0[p], c1[p] -- the
//              reverse swap's terms are the ones just left, so gain_p needs no
//              scan -- and writes the order, the mask and the stamp, while the
//              waves stride the at most four items (swap p-1 or p+1, side):
//     scan     wave_best: the lanes stride the variable's list (8 B set, 4 B
//              score, coalesced); each keeps one 64-bit key, the score's
//              order-preserving integer image above 2^32 - 1 - index, a single
//              integer maximum per compatible entry; one cross-lane 64-bit
//              maximum yields the value and its least index.  No FP compare,
//              no transcendental, no second pass;  barrier.
//     best     S > S_best: the lane-parallel copy of the order and entries is
//              made at the head of the next step (nothing reads it earlier).
//     kick     rare: the order from the best one, one lane applies the
//              transpositions, then the full work list -- n terms and 2 (n-1)
//              swap sides, strided by the waves -- as at the head of a launch.
// A step is two barriers.  A term is a maximum of integers and every sum a
// fixed FP64 expression: no output depends on W, on the steps per launch or on
// the number of searches.  Plain vector stores only; no atomics in the run
// kernel, no communication between workgroups.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "order_search_state.h"

namespace ulg {

void order_search_delete(ulg_ctx *c) {
    delete c->osearch;
    c->osearch = nullptr;
}

void order_search_end(ulg_ctx *c) {
    if (c->osearch) c->osearch->ready = false;
}

}  // namespace ulg

using namespace ulg;

namespace {

constexpr int kWave = kSearchWave;
constexpr int kB = 256;  // the small kernels' workgroup

constexpr uint64_t kGridX = 1ull << 20;
inline dim3 flat_grid(uint64_t blocks) {
    return dim3((unsigned)std::min<uint64_t>(blocks, kGridX), (unsigned)((blocks + kGridX - 1) / kGridX));
}
__device__ __forceinline__ uint64_t flat_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }
__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

__global__ void __launch_bounds__(kB) osearch_shuffle_kernel(uint8_t *order, int64_t searches, int n, uint64_t seed) {
    const int64_t c = (int64_t)flat_block() * kB + threadIdx.x;
    if (c < searches) mcmc_shuffle(seed, (uint32_t)c, n, order + c * n);
}

// terms[k n + p], ent[k n + p] and parents[k n + v] of `count` orders: a wave
// per (k, p), 4 to a workgroup; each output may be null
__global__ void __launch_bounds__(kB) osearch_best_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets, int n,
                                                          const uint8_t *orders, int64_t count, double *terms, uint32_t *ent,
                                                          uint64_t *parents) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t pair = flat_block() * (kB / kWave) + (threadIdx.x >> 6);
    if (pair >= (uint64_t)count * (uint64_t)n) return;  // the whole wave
    const int64_t k = (int64_t)(pair / (uint64_t)n);
    const int p = (int)(pair % (uint64_t)n);
    const uint8_t *ord = orders + k * n;
    uint64_t U = lane < p ? 1ull << ord[lane] : 0ull;  // n <= 63: a lane per position
    for (int d = kWave / 2; d > 0; d >>= 1) U |= __shfl_xor((unsigned long long)U, d, kWave);
    const int v = ord[p];
    const int64_t b = offsets[v];
    const OsBest r = os_decode(wave_best(sets, scores, b, offsets[v + 1], U, lane));
    if (lane == 0) {
        if (terms) terms[k * n + p] = r.b;
        if (ent) ent[k * n + p] = r.ent;
        if (parents) parents[k * n + v] = r.ent == kSearchNoEntry ? 0ull : sets[b + r.ent];
    }
}

__global__ void __launch_bounds__(kB) osearch_init_kernel(const double *terms, const uint8_t *order, const uint32_t *ent, int64_t searches,
                                                          int n, uint8_t *best_order, uint32_t *best_ent, double *score,
                                                          double *best_score, long long *idle, long long *moves, long long *kicks,
                                                          unsigned int *least) {
    const int64_t c = (int64_t)flat_block() * kB + threadIdx.x;
    if (c >= searches) return;
    bool bad = false;
    double S = 0.0;
    for (int p = 0; p < n; ++p) {
        const double x = terms[c * n + p];
        bad = bad || !(x > neg_inf());
        S += x;
        best_order[c * n + p] = order[c * n + p];
        best_ent[c * n + p] = ent[c * n + p];
    }
    score[c] = best_score[c] = S;
    idle[c] = moves[c] = kicks[c] = 0;
    if (bad) atomicMin(least, (unsigned int)c);
}

__global__ void __launch_bounds__(kB) osearch_parents_kernel(const uint64_t *sets, const int64_t *offsets, const uint8_t *best_order,
                                                             const uint32_t *best_ent, int64_t searches, int n, uint64_t *parents) {
    const uint64_t cell = flat_block() * kB + threadIdx.x;
    if (cell >= (uint64_t)searches * (uint64_t)n) return;
    const int64_t c = (int64_t)(cell / (uint64_t)n);
    const int v = best_order[cell];
    const uint32_t e = best_ent[cell];
    const int64_t b = offsets[v];
    parents[c * n + v] = e < (uint64_t)(offsets[v + 1] - b) ? sets[b + e] : 0ull;  // a best order's terms are finite
}

template <int W>
__global__ void __launch_bounds__(kWave *W) osearch_run_kernel(const SearchArgs a) {
    __shared__ uint8_t ord[kWave], bord[kWave];  // the variable at each position; of the best order
    __shared__ uint64_t pre[kWave];              // the variables before each position
    __shared__ double term[kWave], c0[kWave], c1[kWave];  // c0[p], c1[p]: the terms of positions p, p+1 after swap p
    __shared__ uint32_t ent[kWave], e0[kWave], e1[kWave], bent[kWave];
    __shared__ uint32_t stamp[kMcmcMaxVars * kMcmcMaxVars];  // by (lesser variable) n + (greater)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int n = a.n;
    const int64_t c = (int64_t)blockIdx.x;  // searches <= 2^20
    if (tid < n) {
        ord[tid] = a.order[c * n + tid];
        bord[tid] = a.best_order[c * n + tid];
        term[tid] = a.terms[c * n + tid];
        ent[tid] = a.ent[c * n + tid];
        bent[tid] = a.best_ent[c * n + tid];
    }
    for (int i = tid; i < n * n; i += kWave * W) stamp[i] = a.stamp[c * n * n + i];
    double S = a.score[c], S_best = a.best_score[c];
    long long idle = a.idle[c], moves = a.moves[c], kicks = a.kicks[c];
    __syncthreads();

    // One scan: the wave's lanes return the term of variable v under U
    auto scan = [&](int v, uint64_t U) -> OsBest {
        return os_decode(wave_best(a.sets, a.scores, a.offsets[v], a.offsets[v + 1], U, lane));
    };
    // The work list of the order in LDS from item `first` on: items 0 .. n-1
    // are the terms, item n + 2 p + side the side of swap p (side 0: the later
    // variable moved up, side 1: the earlier one behind it).  Ends on a barrier.
    auto recompute = [&](int first) {
        if (tid < n) {
            uint64_t U = 0;
            for (int q = 0; q < tid; ++q) U |= 1ull << ord[q];
            pre[tid] = U;
        }
        __syncthreads();
        for (int item = first + wave; item < 3 * n - 2; item += W) {
            if (item < n) {
                const OsBest r = scan(ord[item], pre[item]);
                if (lane == 0) term[item] = r.b, ent[item] = r.ent;
            } else {
                const int q = (item - n) >> 1, side = (item - n) & 1;
                const int x = ord[q], y = ord[q + 1];
                const OsBest r = side ? scan(x, pre[q] | (1ull << y)) : scan(y, pre[q]);
                if (lane == 0) {
                    if (side) c1[q] = r.b, e1[q] = r.ent;
                    else c0[q] = r.b, e0[q] = r.ent;
                }
            }
        }
        __syncthreads();
    };
    recompute(n);  // the swaps' sides are not kept between launches

    bool improved = false;  // the best order's copy is due
    for (int64_t s = 0; s < a.nsteps; ++s) {
        const int64_t t = a.t_begin + s + 1;
        double g = neg_inf();
        int p = -1;
        if (n > 1) {
            if (improved && tid < n) bord[tid] = ord[tid], bent[tid] = ent[tid];
            improved = false;
            // select
            double gain = neg_inf();
            uint64_t key = 0;
            if (lane < n - 1) {
                const int x = ord[lane], y = ord[lane + 1];
                gain = os_gain(c0[lane], c1[lane], term[lane], term[lane + 1]);
                const uint32_t st = stamp[(x < y ? x : y) * n + (x < y ? y : x)];
                if (os_admissible(gain, os_tabu(st, t, a.tenure), S, S_best)) key = os_double_image(gain);
            }
            uint64_t top = key;
            for (int d = kWave / 2; d > 0; d >>= 1) {
                const uint64_t o = __shfl_xor((unsigned long long)top, d, kWave);
                top = o > top ? o : top;
            }
            const unsigned long long hit = __ballot(key == top && top != 0);
            p = hit ? __ffsll(hit) - 1 : -1;
            // what the move's items need of the state before it (w x y z at p-1 .. p+2), read ahead of the
            // barrier: the scans then run beside the lane that writes the move
            int rx = 0, ry = 0, rw = 0, rz = 0;
            uint64_t rUp = 0, rUw = 0;
            if (p >= 0) {
                g = __shfl(gain, p, kWave);
                rx = ord[p], ry = ord[p + 1], rUp = pre[p];
                if (p >= 1) rw = ord[p - 1], rUw = pre[p - 1];
                if (p + 2 < n) rz = ord[p + 2];
            }
            __syncthreads();  // every wave has read the state and the cached terms
            if (p >= 0) {
                if (tid == 0) {  // the move: swap p's reverse gives back the terms just left
                    const double t0 = term[p], t1 = term[p + 1];
                    const uint32_t u0 = ent[p], u1 = ent[p + 1];
                    term[p] = c0[p], term[p + 1] = c1[p], ent[p] = e0[p], ent[p + 1] = e1[p];
                    c0[p] = t0, c1[p] = t1, e0[p] = u0, e1[p] = u1;
                    ord[p] = (uint8_t)ry, ord[p + 1] = (uint8_t)rx;
                    pre[p + 1] = rUp | (1ull << ry);
                    stamp[(rx < ry ? rx : ry) * n + (rx < ry ? ry : rx)] = (uint32_t)t;
                }
                for (int it = wave; it < 4; it += W) {
                    if (it < 2 ? p < 1 : p + 2 >= n) continue;
                    const int side = it & 1, q = it < 2 ? p - 1 : p + 1;
                    const uint64_t Un = rUp | (1ull << ry);
                    const int v = it < 2 ? (side ? rw : ry) : (side ? rx : rz);
                    const uint64_t U = it < 2 ? (side ? rUw | (1ull << ry) : rUw) : (side ? Un | (1ull << rz) : Un);
                    const OsBest r = scan(v, U);
                    if (lane == 0) {
                        if (side) c1[q] = r.b, e1[q] = r.ent;
                        else c0[q] = r.b, e0[q] = r.ent;
                    }
                }
                S = S + g;
                ++moves;
            }
            if (S > S_best) S_best = S, idle = 0, improved = true;
            else ++idle;
            __syncthreads();  // the move and the scans stand
            if (idle >= a.patience) {  // the kick; `improved` is false here
                if (tid < n) ord[tid] = bord[tid];
                __syncthreads();
                if (tid == 0) os_kick(a.seed, (uint64_t)t, (uint32_t)c, n, ord);  // one lane: the transpositions may share positions
                __syncthreads();
                recompute(0);
                const bool bad = __ballot(lane < n && !(term[lane] > neg_inf())) != 0ull;
                __syncthreads();
                if (bad) {  // undone: back on the best order
                    if (tid < n) ord[tid] = bord[tid];
                    __syncthreads();
                    recompute(0);
                } else {
                    ++kicks;
                }
                for (int i = tid; i < n * n; i += kWave * W) stamp[i] = 0u;
                S = 0.0;
                for (int q = 0; q < n; ++q) S += term[q];
                idle = 0;
                if (!bad) {
                    if (S > S_best) S_best = S, improved = true;
                    else idle = 1;
                }
                __syncthreads();
            }
        }
        if (tid == 0) {
            const int64_t at = (t - a.t_call - 1) * a.searches + c;
            if (a.t_gain) a.t_gain[at] = g;
            if (a.t_pos) a.t_pos[at] = p >= 0 ? (uint8_t)p : kSearchNoMove;
        }
    }
    if (improved && tid < n) bord[tid] = ord[tid], bent[tid] = ent[tid];
    __syncthreads();
    if (tid < n) {
        a.order[c * n + tid] = ord[tid];
        a.best_order[c * n + tid] = bord[tid];
        a.terms[c * n + tid] = term[tid];
        a.ent[c * n + tid] = ent[tid];
        a.best_ent[c * n + tid] = bent[tid];
    }
    for (int i = tid; i < n * n; i += kWave * W) a.stamp[c * n * n + i] = stamp[i];
    if (tid == 0) {
        a.score[c] = S, a.best_score[c] = S_best;
        a.idle[c] = idle, a.moves[c] = moves, a.kicks[c] = kicks;
    }
}

// ---- host
OrderSearchState *live(ulg_ctx *c) { return order_search_live(c); }

int launch_best(ulg_ctx *c, const OrderMcmcState &l, const uint8_t *d_orders, int64_t count, double *d_terms, uint32_t *d_ent,
                uint64_t *d_parents) {
    const uint64_t pairs = (uint64_t)count * (uint64_t)l.n;
    prof_begin(c, "osearch_best");
    osearch_best_kernel<<<flat_grid((pairs + kB / kWave - 1) / (kB / kWave)), kB, 0, c->stream>>>(
        l.d_sets.p, l.d_scores.p, l.d_offsets.p, l.n, d_orders, count, d_terms, d_ent, d_parents);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    return ULG_OK;
}

// What both begins refuse before any device work
int check_args(ulg_ctx *c, const std::string &who, int64_t searches, int64_t tenure, int64_t patience) {
    if (searches < 1 || searches > kMcmcMaxChains) return set_err(c, ULG_ERR_ARG, who + ": searches must be 1..2^20");
    if (tenure < 0 || tenure > kSearchMaxTenure) return set_err(c, ULG_ERR_ARG, who + ": tenure must be 0..2^20");
    if (patience < 1 || patience > kSearchMaxPatience) return set_err(c, ULG_ERR_ARG, who + ": patience must be 1..2^31-1");
    return ULG_OK;
}

// The lists stand checked in c->mcmc: the searches' orders, terms and best-so-far.
int begin(ulg_ctx *c, const std::string &who, int64_t C, uint64_t seed, int64_t tenure, int64_t patience, const uint8_t *init_order) {
    const OrderMcmcState &l = *c->mcmc;
    const int n = l.n;
    for (int v = 0; v < n; ++v)
        if (l.offsets[v + 1] - l.offsets[v] > (int64_t)0xFFFFFFFFll)
            return set_err(c, ULG_ERR_UNSUPPORTED, who + ": variable " + std::to_string(v) + " lists more than 2^32 - 1 sets");
    if (init_order)
        for (int64_t k = 0; k < C; ++k)
            if (!is_permutation(init_order + k * n, n))
                return set_err(c, ULG_ERR_ARG, who + ": the initial order of search " + std::to_string(k) + " is not a permutation");
    if (!c->osearch) c->osearch = new OrderSearchState();
    OrderSearchState &s = *c->osearch;
    s.ready = false;
    s.tables = false;
    const bool tables = c->opt.search_tables != 0;
    double table_need = 0.0;  // option "search_tables": the candidate sets and the tables' sizes, before anything is allocated for them
    if (!tables) order_tables_drop(s);
    else if (int rc = order_tables_plan(c, who, s, l, &table_need)) return rc;
    const size_t cells = (size_t)C * (size_t)n;
    {
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        const double need = (double)C * (18.0 * n + 4.0 * n * n + 40.0) + 12 * 16.0 + 256.0 + table_need,
                     have = (double)free_b + (double)s.held_bytes();
        if (need > have && tables) {
            int big = 0;
            for (int v = 1; v < n; ++v)
                if (s.toff[v + 1] - s.toff[v] > s.toff[big + 1] - s.toff[big]) big = v;
            char buf[320];
            std::snprintf(buf, sizeof buf,
                          "%s: the tables of option \"search_tables\" need %.0f bytes of device memory (the largest, variable %d's, %.0f) "
                          "beside %.0f for %lld searches, %.0f are free",
                          who.c_str(), table_need, big, 8.0 * (double)(s.toff[big + 1] - s.toff[big]), need - table_need, (long long)C, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld searches of n = %d need %.0f bytes of device memory, %.0f are free", who.c_str(),
                          (long long)C, n, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    int rc;
    if ((rc = ensure(c, s.d_order, cells)) || (rc = ensure(c, s.d_best_order, cells)) || (rc = ensure(c, s.d_terms, cells)) ||
        (rc = ensure(c, s.d_ent, cells)) || (rc = ensure(c, s.d_best_ent, cells)) || (rc = ensure(c, s.d_stamp, cells * n)) ||
        (rc = ensure(c, s.d_score, (size_t)C)) || (rc = ensure(c, s.d_best_score, (size_t)C)) || (rc = ensure(c, s.d_idle, (size_t)C)) ||
        (rc = ensure(c, s.d_moves, (size_t)C)) || (rc = ensure(c, s.d_kicks, (size_t)C)) || (rc = ensure(c, s.d_err, 1)))
        return rc;
    ULG_HIP(c, hipMemsetAsync(s.d_err.p, 0xFF, sizeof(unsigned int), c->stream));
    ULG_HIP(c, hipMemsetAsync(s.d_stamp.p, 0, cells * n * 4, c->stream));
    if (init_order) {
        ULG_HIP(c, hipMemcpyAsync(s.d_order.p, init_order, cells, hipMemcpyHostToDevice, c->stream));
        ULG_HIP(c, hipStreamSynchronize(c->stream));  // init_order is the caller's again, whatever returns below
    } else {
        prof_begin(c, "osearch_shuffle");
        osearch_shuffle_kernel<<<flat_grid(((uint64_t)C + kB - 1) / kB), kB, 0, c->stream>>>(s.d_order.p, C, n, seed);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    if (tables && (rc = order_tables_build(c, s, l))) return rc;
    if ((rc = s.tables ? order_tables_best(c, s, l, s.d_order.p, C, s.d_terms.p, s.d_ent.p, nullptr)
                       : launch_best(c, l, s.d_order.p, C, s.d_terms.p, s.d_ent.p, nullptr)))
        return rc;
    prof_begin(c, "osearch_init");
    osearch_init_kernel<<<flat_grid(((uint64_t)C + kB - 1) / kB), kB, 0, c->stream>>>(
        s.d_terms.p, s.d_order.p, s.d_ent.p, C, n, s.d_best_order.p, s.d_best_ent.p, s.d_score.p, s.d_best_score.p, s.d_idle.p,
        s.d_moves.p, s.d_kicks.p, s.d_err.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    unsigned int least = 0;
    ULG_HIP(c, hipMemcpyAsync(&least, s.d_err.p, sizeof least, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (least != 0xFFFFFFFFu)
        return set_err(c, ULG_ERR_ARG,
                       who + ": the initial order of search " + std::to_string(least) +
                           " has a variable without a stored parent set among its predecessors (a term of -inf)");
    s.n = n;
    s.searches = C;
    s.seed = seed;
    s.tenure = tenure;
    s.patience = patience;
    s.step = 0;
    s.ready = true;
    return ULG_OK;
}

template <int W>
void launch_run(ulg_ctx *c, const SearchArgs &a) {
    osearch_run_kernel<W><<<dim3((unsigned)a.searches), kWave * W, 0, c->stream>>>(a);
}

}  // namespace

extern "C" {

int ulg_order_search_begin(ulg_ctx *c, int n, const int64_t *offsets, const uint64_t *sets, const float *scores, int device_ptrs,
                           int64_t searches, uint64_t seed, int64_t tenure, int64_t patience, const uint8_t *init_order) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_search_begin";
    order_search_end(c);  // a begin that is refused, for whatever reason, leaves no state of any family
    partition_mcmc_end(c);
    if (c->mcmc) c->mcmc->ready = false;
    if (int rc = check_args(c, who, searches, tenure, patience)) return rc;
    if (int rc = order_mcmc_take_lists(c, who, n, offsets, sets, scores, device_ptrs, searches)) return rc;
    return begin(c, who, searches, seed, tenure, patience, init_order);
}

int ulg_order_search_begin_from_scores(ulg_ctx *c, int64_t searches, uint64_t seed, int64_t tenure, int64_t patience,
                                       const uint8_t *init_order) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_search_begin_from_scores";
    order_search_end(c);
    partition_mcmc_end(c);
    if (c->mcmc) c->mcmc->ready = false;
    if (int rc = check_args(c, who, searches, tenure, patience)) return rc;
    if (int rc = order_mcmc_take_scored(c, who, searches)) return rc;
    return begin(c, who, searches, seed, tenure, patience, init_order);
}

int ulg_order_search_run(ulg_ctx *c, int64_t steps, double *best_score, uint8_t *best_order, uint64_t *best_parents, int64_t *moves,
                         int64_t *kicks, double *trace_gain, uint8_t *trace_pos) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_search_run";
    if (!live(c)) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_search_begin");
    OrderSearchState &s = *c->osearch;
    const OrderMcmcState &l = *c->mcmc;
    if (steps < 0) return set_err(c, ULG_ERR_ARG, who + ": steps must be >= 0");
    if (steps > kSearchMaxSteps - s.step) return set_err(c, ULG_ERR_ARG, who + ": the step count passes 2^32 - 1");
    const int n = s.n;
    const int64_t C = s.searches, t0 = s.step;
    ULG_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)C * (size_t)n, nmove = (size_t)steps * (size_t)C;
    {
        const double need = (double)steps * (double)C * ((trace_gain ? 8.0 : 0.0) + (trace_pos ? 1.0 : 0.0)) +
                            (best_parents ? 8.0 * (double)cells : 0.0) + 3 * 16.0 + 256.0;
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        const double have = (double)free_b + (double)s.run_bytes();
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld steps of %lld searches need %.0f bytes of device memory, %.0f are free", who.c_str(),
                          (long long)steps, (long long)C, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    int rc;
    if ((trace_gain && (rc = ensure(c, s.r_gain, nmove))) || (trace_pos && (rc = ensure(c, s.r_pos, nmove))) ||
        (best_parents && (rc = ensure(c, s.r_parents, cells))))
        return rc;
    SearchArgs a;
    a.sets = l.d_sets.p, a.scores = l.d_scores.p, a.offsets = l.d_offsets.p;
    a.order = s.d_order.p, a.best_order = s.d_best_order.p, a.terms = s.d_terms.p;
    a.ent = s.d_ent.p, a.best_ent = s.d_best_ent.p, a.stamp = s.d_stamp.p;
    a.score = s.d_score.p, a.best_score = s.d_best_score.p;
    a.idle = s.d_idle.p, a.moves = s.d_moves.p, a.kicks = s.d_kicks.p;
    a.n = n, a.searches = C, a.seed = s.seed, a.tenure = s.tenure, a.patience = s.patience;
    a.t_call = t0, a.nsteps = 0;
    a.t_gain = trace_gain ? s.r_gain.p : nullptr;
    a.t_pos = trace_pos ? s.r_pos.p : nullptr;
    const int64_t cap = c->opt.mcmc_launch_steps;
    for (int64_t done = 0; done < steps; done += a.nsteps) {
        a.t_begin = t0 + done;
        a.nsteps = std::min(cap, steps - done);
        prof_begin(c, s.tables ? "otab_run" : "osearch_run");
        if (s.tables) {
            order_tables_run(c, s, a);
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
    if (best_parents) {
        prof_begin(c, "osearch_parents");
        osearch_parents_kernel<<<flat_grid(((uint64_t)cells + kB - 1) / kB), kB, 0, c->stream>>>(
            l.d_sets.p, l.d_offsets.p, s.d_best_order.p, s.d_best_ent.p, C, n, s.r_parents.p);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    s.step = t0 + steps;  // the searches have moved, whatever becomes of the copies below
    static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as they are");
    if (best_score) ULG_HIP(c, hipMemcpyAsync(best_score, s.d_best_score.p, (size_t)C * 8, hipMemcpyDeviceToHost, c->stream));
    if (best_order) ULG_HIP(c, hipMemcpyAsync(best_order, s.d_best_order.p, cells, hipMemcpyDeviceToHost, c->stream));
    if (best_parents) ULG_HIP(c, hipMemcpyAsync(best_parents, s.r_parents.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (moves) ULG_HIP(c, hipMemcpyAsync(moves, s.d_moves.p, (size_t)C * 8, hipMemcpyDeviceToHost, c->stream));
    if (kicks) ULG_HIP(c, hipMemcpyAsync(kicks, s.d_kicks.p, (size_t)C * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace_gain && nmove) ULG_HIP(c, hipMemcpyAsync(trace_gain, s.r_gain.p, nmove * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace_pos && nmove) ULG_HIP(c, hipMemcpyAsync(trace_pos, s.r_pos.p, nmove, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    return ULG_OK;
}

int ulg_order_search_state(ulg_ctx *c, uint8_t *order, double *terms, double *score, int64_t *step) {
    if (!c) return ULG_ERR_ARG;
    if (!live(c)) return set_err(c, ULG_ERR_STATE, "ulg_order_search_state: no ulg_order_search_begin");
    OrderSearchState &s = *c->osearch;
    const size_t cells = (size_t)s.searches * (size_t)s.n;
    ULG_HIP(c, hipSetDevice(c->device));
    if (order) ULG_HIP(c, hipMemcpyAsync(order, s.d_order.p, cells, hipMemcpyDeviceToHost, c->stream));
    if (terms) ULG_HIP(c, hipMemcpyAsync(terms, s.d_terms.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (score) ULG_HIP(c, hipMemcpyAsync(score, s.d_score.p, (size_t)s.searches * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    if (step) *step = s.step;
    return ULG_OK;
}

int ulg_order_best(ulg_ctx *c, int64_t count, const uint8_t *orders, double *terms, uint64_t *parents) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_best";
    if (!live(c)) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_search_begin");
    OrderSearchState &s = *c->osearch;
    const int n = s.n;
    if (count < 0 || (count > 0 && !orders)) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
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
        const double need = 17.0 * (double)cells + 3 * 16.0 + 256.0, have = (double)free_b + (double)s.run_bytes();
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld orders of n = %d need %.0f bytes of device memory, %.0f are free", who.c_str(),
                          (long long)count, n, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    int rc;
    if ((rc = ensure(c, s.r_order, cells)) || (terms && (rc = ensure(c, s.r_terms, cells))) ||
        (parents && (rc = ensure(c, s.r_parents, cells))))
        return rc;
    ULG_HIP(c, hipMemcpyAsync(s.r_order.p, orders, cells, hipMemcpyHostToDevice, c->stream));
    double *const d_terms = terms ? s.r_terms.p : nullptr;
    uint64_t *const d_parents = parents ? s.r_parents.p : nullptr;
    if ((rc = s.tables ? order_tables_best(c, s, *c->mcmc, s.r_order.p, count, d_terms, nullptr, d_parents)
                       : launch_best(c, *c->mcmc, s.r_order.p, count, d_terms, nullptr, d_parents)))
        return rc;
    if (terms) ULG_HIP(c, hipMemcpyAsync(terms, s.r_terms.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (parents) ULG_HIP(c, hipMemcpyAsync(parents, s.r_parents.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ULG_OK;
}

int ulg_order_search_table(ulg_ctx *c, int v, uint64_t *candidates, int64_t *slots, uint64_t *keys, int64_t cap) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_search_table";
    if (!live(c)) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_search_begin");
    OrderSearchState &s = *c->osearch;
    if (!s.tables) return set_err(c, ULG_ERR_STATE, who + ": the searches were begun without option \"search_tables\"");
    if (v < 0 || v >= s.n) return set_err(c, ULG_ERR_ARG, who + ": v out of range");
    const int64_t count = s.toff[v + 1] - s.toff[v];
    if (candidates) *candidates = s.cand[v];
    if (slots) *slots = count;
    if (keys && cap >= count) {
        ULG_HIP(c, hipSetDevice(c->device));
        ULG_HIP(c, hipMemcpyAsync(keys, s.d_table.p + s.toff[v], (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
        ULG_HIP(c, hipStreamSynchronize(c->stream));
    }
    return ULG_OK;
}

}  // extern "C"
