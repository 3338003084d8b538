// order_tables.hip -- the order search over dense candidate-set tables (option
// "search_tables", ulg_order_search_table; contract: include/ulg.h, "Order
// search"; arithmetic: order_tables_dev.h).  For every variable v the table
// T_v over the subsets of its candidate parents C_v holds the maximum of
// os_entry_key over the stored sets inside the subset, so a term is one load
// at idx_v(U) and a neighbour swap moves an index by one bit.  A maximum of
// integers: the searches give the bits of the list-scanning path.
//
// Kernels:
//   otab_cand_kernel     one workgroup per variable: C_v, the OR of its sets
//   otab_small_kernel    K_v <= 13: one workgroup per variable builds the table
//                        in LDS (64 KB) -- slots cleared, every entry's key
//                        stored at the index of its own set, the butterfly,
//                        one coalesced write of the table
//   otab_scatter_kernel  K_v > 13: the keys into the cleared global table
//   otab_tile_kernel     ... rounds 0 .. 12 on tiles of 2^13 slots in LDS
//   otab_high_kernel     ... round j >= 13 as a strided pass over the pairs;
//                        each of the three serves every such variable at once
//     butterfly  (lds_butterfly) a lane owns slot 256 r + tid, so bits 0 .. 5
//              of a slot are the lane: rounds 0 .. 5 are cross-lane exchanges
//              of the slot's register inside a wave, rounds 6 .. through LDS,
//              one barrier each.
//   otab_best_kernel     one wave per order, lane p = position p: the
//                        predecessor masks by a prefix OR across the lanes,
//                        one load per term (ulg_order_best, the begin's terms)
//   otab_run_kernel      one wave per search, four searches to a workgroup,
//                        all steps of the launch and no barrier.  Lane p owns
//                        position p: its variable, C and table base, the table
//                        index of its predecessors, its term and entry, the
//                        best order's variable and entry.  The pair stamps
//                        [n][n] are the wave's slice of LDS.
//     select   lane p = swap p of x (its own) and y (lane p + 1's, by
//              shuffles): T_y[idx_y - bit_y(x)] and T_x[idx_x + bit_x(y)], two
//              gathers, os_gain, the stamp, os_admissible; a 64-bit wave
//              maximum of the gain's image, a ballot and a find-first.
//     move     lane p takes y's new state from its own registers, lane p + 1
//              x's by a shuffle from lane p; lane p stamps the pair.
//     kick     the best order through 64 bytes of LDS for os_kick on one
//              lane, then every lane's index and term again from the order.
// S, S_best and the counts are the same bits in every lane.  Plain vector
// stores only, no atomics, no communication between waves.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "order_search_state.h"
#include "order_tables_dev.h"

using namespace ulg;

namespace {

constexpr int kWave = kSearchWave;
constexpr int kB = 256;
constexpr int kRunWaves = 4;   // searches per workgroup of the run kernel
constexpr int kKickWords = 16;  // 64 bytes of LDS per search: the order os_kick permutes
constexpr int kLdsSlots = 1 << kTableLdsK;

constexpr uint64_t kGridX = 1ull << 20;
inline dim3 flat_grid(uint64_t blocks) {
    return dim3((unsigned)std::min<uint64_t>(blocks, kGridX), (unsigned)((blocks + kGridX - 1) / kGridX));
}
__device__ __forceinline__ uint64_t flat_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }
__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t x, int d) { return __shfl_xor((unsigned long long)x, d, kWave); }
__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, int d) { return __shfl_up((unsigned long long)x, d, kWave); }
__device__ __forceinline__ uint64_t shfl_down64(uint64_t x, int d) { return __shfl_down((unsigned long long)x, d, kWave); }
// what one lane of the wave wrote to LDS, the others may read
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t entry_key(const float *scores, int64_t i, int64_t b) {
    return os_entry_key(__float_as_uint(scores[i]), (uint32_t)(i - b));
}

__global__ void __launch_bounds__(kB) otab_cand_kernel(const uint64_t *sets, const int64_t *offsets, uint64_t *cand) {
    __shared__ uint64_t part[kB / kWave];
    const int v = blockIdx.x, tid = threadIdx.x;
    uint64_t C = 0;
    for (int64_t i = offsets[v] + tid, e = offsets[v + 1]; i < e; i += kB) C |= sets[i];
    for (int d = kWave / 2; d > 0; d >>= 1) C |= shfl_xor64(C, d);
    if ((tid & (kWave - 1)) == 0) part[tid >> 6] = C;
    __syncthreads();
    if (tid == 0) cand[v] = part[0] | part[1] | part[2] | part[3];
}

// Rounds 0 .. K-1 on T[0 .. 2^K) in LDS, K <= kTableLdsK, by the kB lanes of the
// workgroup, all of which call it.  Begins and ends on a barrier.
__device__ __forceinline__ void lds_butterfly(uint64_t *T, int K, int tid) {
    const int slots = 1 << K, lane = tid & (kWave - 1), low = K < 6 ? K : 6;
    __syncthreads();
    for (int base = 0; base < slots; base += kB) {
        const int x = base + tid;
        uint64_t val = x < slots ? T[x] : 0ull;
        for (int j = 0; j < low; ++j) {
            const uint64_t o = shfl_xor64(val, 1 << j);
            if (((lane >> j) & 1) && o > val) val = o;
        }
        if (x < slots) T[x] = val;
    }
    __syncthreads();
    for (int j = 6; j < K; ++j) {
        for (int q = tid; q < slots / 2; q += kB) {
            const int x = ((q >> j) << (j + 1)) | (1 << j) | (q & ((1 << j) - 1));
            const uint64_t o = T[x ^ (1 << j)];
            if (o > T[x]) T[x] = o;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kB) otab_small_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets,
                                                        const uint64_t *cand, const int64_t *toff, uint64_t *table) {
    __shared__ uint64_t T[kLdsSlots];
    const int v = blockIdx.x, tid = threadIdx.x;
    const uint64_t C = cand[v];
    const int K = ot_popcount(C);
    if (K > kTableLdsK) return;  // the whole workgroup
    const int slots = 1 << K;
    for (int x = tid; x < slots; x += kB) T[x] = 0ull;
    __syncthreads();
    const int64_t b = offsets[v], e = offsets[v + 1];
    for (int64_t i = b + tid; i < e; i += kB) T[ot_index(C, sets[i])] = entry_key(scores, i, b);
    lds_butterfly(T, K, tid);
    uint64_t *out = table + toff[v];
    for (int x = tid; x < slots; x += kB) out[x] = T[x];
}

// grid (any, n): the entries of every variable with K > kTableLdsK
__global__ void __launch_bounds__(kB) otab_scatter_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets,
                                                          const uint64_t *cand, const int64_t *toff, uint64_t *table) {
    const int v = blockIdx.y;
    const uint64_t C = cand[v];
    if (ot_popcount(C) <= kTableLdsK) return;
    uint64_t *out = table + toff[v];
    const int64_t b = offsets[v], e = offsets[v + 1];
    for (int64_t i = b + (int64_t)blockIdx.x * kB + threadIdx.x; i < e; i += (int64_t)gridDim.x * kB)
        out[ot_index(C, sets[i])] = entry_key(scores, i, b);
}

// grid (2^(Kmax - kTableLdsK), n): tile blockIdx.x of variable blockIdx.y
__global__ void __launch_bounds__(kB) otab_tile_kernel(const uint64_t *cand, const int64_t *toff, uint64_t *table) {
    __shared__ uint64_t T[kLdsSlots];
    const int v = blockIdx.y, tid = threadIdx.x;
    const int K = ot_popcount(cand[v]);
    if (K <= kTableLdsK || (int64_t)blockIdx.x >= ot_slots(K - kTableLdsK)) return;
    uint64_t *tile = table + toff[v] + (int64_t)blockIdx.x * kLdsSlots;
    for (int x = tid; x < kLdsSlots; x += kB) T[x] = tile[x];
    lds_butterfly(T, kTableLdsK, tid);
    for (int x = tid; x < kLdsSlots; x += kB) tile[x] = T[x];
}

// grid (2^(Kmax - 1) / kB, n): round j >= kTableLdsK, a lane per pair of slots
__global__ void __launch_bounds__(kB) otab_high_kernel(const uint64_t *cand, const int64_t *toff, uint64_t *table, int j) {
    const int v = blockIdx.y;
    const int K = ot_popcount(cand[v]);
    const int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (K <= j || q >= ot_slots(K - 1)) return;
    const int64_t bit = (int64_t)1 << j, x = ((q >> j) << (j + 1)) | bit | (q & (bit - 1));
    uint64_t *T = table + toff[v];
    const uint64_t o = T[x ^ bit];
    if (o > T[x]) T[x] = o;
}

// What lane p holds of the variable v at its position: C_v, the table's first
// slot, and the table index of the variables at the lanes below (on: lane < n).
struct Place {
    uint64_t C;
    int64_t base;
    uint32_t idx;
};
__device__ __forceinline__ Place place_of(const uint64_t *cand, const int64_t *toff, int v, bool on, int lane) {
    const uint64_t own = on ? 1ull << v : 0ull;
    uint64_t U = own;  // the prefix OR across the lanes, this one included
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t o = shfl_up64(U, d);
        if (lane >= d) U |= o;
    }
    Place r;
    r.C = on ? cand[v] : 0ull, r.base = on ? toff[v] : 0;
    r.idx = ot_index(r.C, U & ~own);
    return r;
}

// terms[k n + p], ent[k n + p] and parents[k n + v] of `count` orders: a wave per order; each output may be null
__global__ void __launch_bounds__(kB) otab_best_kernel(const uint64_t *sets, const int64_t *offsets, const uint64_t *cand,
                                                       const int64_t *toff, const uint64_t *table, int n, const uint8_t *orders,
                                                       int64_t count, double *terms, uint32_t *ent, uint64_t *parents) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t k = flat_block() * (kB / kWave) + (threadIdx.x >> 6);
    if (k >= (uint64_t)count) return;  // the whole wave
    const bool on = lane < n;
    const int v = on ? orders[k * n + lane] : 0;
    const Place pl = place_of(cand, toff, v, on, lane);
    if (!on) return;
    const OsBest r = os_decode(table[pl.base + pl.idx]);
    if (terms) terms[k * n + lane] = r.b;
    if (ent) ent[k * n + lane] = r.ent;
    if (parents) parents[k * n + v] = r.ent == kSearchNoEntry ? 0ull : sets[offsets[v] + r.ent];
}

__global__ void __launch_bounds__(kWave *kRunWaves) otab_run_kernel(const SearchArgs a, const uint64_t *cand, const int64_t *toff,
                                                                     const uint64_t *table) {
    extern __shared__ uint32_t lds[];  // per wave: the stamps by (lesser variable) n + (greater), then the kick's order
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int n = a.n;
    const int64_t c = (int64_t)blockIdx.x * kRunWaves + wave;
    if (c >= a.searches) return;  // the whole wave; the kernel has no barrier
    uint32_t *stamp = lds + wave * (n * n + kKickWords);
    uint8_t *kord = reinterpret_cast<uint8_t *>(stamp + n * n);
    const bool on = lane < n;
    const int64_t at = c * n + lane;
    int v = on ? a.order[at] : 0, bv = on ? a.best_order[at] : 0;
    double term = on ? a.terms[at] : 0.0;
    uint32_t ent = on ? a.ent[at] : 0u, bent = on ? a.best_ent[at] : 0u;
    for (int i = lane; i < n * n; i += kWave) stamp[i] = a.stamp[c * n * n + i];
    wave_sync();
    double S = a.score[c], S_best = a.best_score[c];
    long long idle = a.idle[c], moves = a.moves[c], kicks = a.kicks[c];
    Place pl = place_of(cand, toff, v, on, lane);  // the indices are not kept between launches

    // every lane's place, term and entry from the order in v
    auto recompute = [&]() {
        pl = place_of(cand, toff, v, on, lane);
        const OsBest r = os_decode(on ? table[pl.base + pl.idx] : 0ull);
        term = r.b, ent = r.ent;
    };

    for (int64_t s = 0; s < a.nsteps; ++s) {
        const int64_t t = a.t_begin + s + 1;
        double g = neg_inf();
        int p = -1;
        if (n > 1) {
            // select: lane p is swap p of x = v with y, the lane above's
            const int y = __shfl_down(v, 1, kWave);
            const uint32_t idy = __shfl_down(pl.idx, 1, kWave);
            const double ty = __shfl_down(term, 1, kWave);
            const uint64_t Cy = shfl_down64(pl.C, 1);
            const int64_t by = (int64_t)shfl_down64((uint64_t)pl.base, 1);
            double gain = neg_inf(), b0 = 0.0, b1 = 0.0;
            uint32_t i0 = 0, i1 = 0, e0 = 0, e1 = 0;
            uint64_t key = 0;
            const int pair = (v < y ? v : y) * n + (v < y ? y : v);
            if (lane < n - 1) {
                i0 = idy - ot_bit(Cy, v);    // y moved up: x leaves its predecessors
                i1 = pl.idx + ot_bit(pl.C, y);  // x behind it: y joins them
                const OsBest r0 = os_decode(table[by + i0]), r1 = os_decode(table[pl.base + i1]);
                b0 = r0.b, e0 = r0.ent, b1 = r1.b, e1 = r1.ent;
                gain = os_gain(b0, b1, term, ty);
                if (os_admissible(gain, os_tabu(stamp[pair], t, a.tenure), S, S_best)) key = os_double_image(gain);
            }
            uint64_t top = key;
            for (int d = kWave / 2; d > 0; d >>= 1) {
                const uint64_t o = shfl_xor64(top, d);
                top = o > top ? o : top;
            }
            const unsigned long long hit = __ballot(key == top && top != 0);
            p = hit ? __ffsll(hit) - 1 : -1;
            if (p >= 0) {  // the move
                g = __shfl(gain, p, kWave);
                const int ux = __shfl_up(v, 1, kWave);  // what lane p + 1 takes of x, from lane p
                const uint64_t uC = shfl_up64(pl.C, 1);
                const int64_t ub = (int64_t)shfl_up64((uint64_t)pl.base, 1);
                const uint32_t ui = __shfl_up(i1, 1, kWave), ue = __shfl_up(e1, 1, kWave);
                const double ut = __shfl_up(b1, 1, kWave);
                if (lane == p) {
                    stamp[pair] = (uint32_t)t;
                    v = y, pl.C = Cy, pl.base = by, pl.idx = i0, term = b0, ent = e0;
                } else if (lane == p + 1) {
                    v = ux, pl.C = uC, pl.base = ub, pl.idx = ui, term = ut, ent = ue;
                }
                wave_sync();
                S = S + g;
                ++moves;
            }
            if (S > S_best) S_best = S, idle = 0, bv = v, bent = ent;
            else ++idle;
            if (idle >= a.patience) {  // the kick
                if (on) kord[lane] = (uint8_t)bv;
                wave_sync();
                if (lane == 0) os_kick(a.seed, (uint64_t)t, (uint32_t)c, n, kord);  // one lane: the transpositions may share positions
                wave_sync();
                v = on ? kord[lane] : 0;
                recompute();
                const bool bad = __ballot(on && !(term > neg_inf())) != 0ull;
                if (bad) {  // undone: back on the best order
                    v = bv;
                    recompute();
                } else {
                    ++kicks;
                }
                for (int i = lane; i < n * n; i += kWave) stamp[i] = 0u;
                wave_sync();
                S = 0.0;
                for (int q = 0; q < n; ++q) S += __shfl(term, q, kWave);
                idle = 0;
                if (!bad) {
                    if (S > S_best) S_best = S, bv = v, bent = ent;
                    else idle = 1;
                }
            }
        }
        if (lane == 0) {
            const int64_t row = (t - a.t_call - 1) * a.searches + c;
            if (a.t_gain) a.t_gain[row] = g;
            if (a.t_pos) a.t_pos[row] = p >= 0 ? (uint8_t)p : kSearchNoMove;
        }
    }
    if (on) {
        a.order[at] = (uint8_t)v, a.best_order[at] = (uint8_t)bv;
        a.terms[at] = term;
        a.ent[at] = ent, a.best_ent[at] = bent;
    }
    for (int i = lane; i < n * n; i += kWave) a.stamp[c * n * n + i] = stamp[i];
    if (lane == 0) {
        a.score[c] = S, a.best_score[c] = S_best;
        a.idle[c] = idle, a.moves[c] = moves, a.kicks[c] = kicks;
    }
}

}  // namespace

namespace ulg {

void order_tables_drop(OrderSearchState &s) {
    s.tables = false;
    s.d_table.reset();
    s.d_cand.reset();
    s.d_toff.reset();
}

int order_tables_plan(ulg_ctx *c, const std::string &who, OrderSearchState &s, const OrderMcmcState &l, double *bytes) {
    const int n = l.n;
    int rc;
    if ((rc = ensure(c, s.d_cand, (size_t)n)) || (rc = ensure(c, s.d_toff, (size_t)n + 1))) return rc;
    prof_begin(c, "otab_cand");
    otab_cand_kernel<<<dim3((unsigned)n), kB, 0, c->stream>>>(l.d_sets.p, l.d_offsets.p, s.d_cand.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    s.cand.assign((size_t)n, 0);
    ULG_HIP(c, hipMemcpyAsync(s.cand.data(), s.d_cand.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    s.toff.assign((size_t)n + 1, 0);
    for (int v = 0; v < n; ++v) {
        const int K = ot_popcount(s.cand[v]);
        if (K > kTableMaxK) {
            char buf[256];
            std::snprintf(buf, sizeof buf,
                          "%s: option \"search_tables\": variable %d has %d candidate parents, its table would take %.0f bytes; at most %d "
                          "candidates are supported",
                          who.c_str(), v, K, 8.0 * std::ldexp(1.0, K), kTableMaxK);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
        s.toff[v + 1] = s.toff[v] + ot_slots(K);
    }
    ULG_HIP(c, hipMemcpyAsync(s.d_toff.p, s.toff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    *bytes = 8.0 * (double)s.toff[n] + 16.0 * n + 8.0 + 3 * 16.0;
    return ULG_OK;
}

int order_tables_build(ulg_ctx *c, OrderSearchState &s, const OrderMcmcState &l) {
    const int n = l.n;
    if (int rc = ensure(c, s.d_table, (size_t)s.toff[n])) return rc;
    int Kmax = 0;
    for (int v = 0; v < n; ++v) Kmax = std::max(Kmax, ot_popcount(s.cand[v]));
    const uint64_t *cand = s.d_cand.p;
    const int64_t *toff = s.d_toff.p;
    uint64_t *table = s.d_table.p;
    if (Kmax > kTableLdsK) {  // the large tables: cleared, the keys stored, then the low rounds by tiles
        ULG_HIP(c, hipMemsetAsync(table, 0, (size_t)s.toff[n] * 8, c->stream));
        prof_begin(c, "otab_scatter");
        otab_scatter_kernel<<<dim3(64, (unsigned)n), kB, 0, c->stream>>>(l.d_sets.p, l.d_scores.p, l.d_offsets.p, cand, toff, table);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    prof_begin(c, "otab_small");
    otab_small_kernel<<<dim3((unsigned)n), kB, 0, c->stream>>>(l.d_sets.p, l.d_scores.p, l.d_offsets.p, cand, toff, table);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    if (Kmax > kTableLdsK) {
        prof_begin(c, "otab_tile");
        otab_tile_kernel<<<dim3((unsigned)ot_slots(Kmax - kTableLdsK), (unsigned)n), kB, 0, c->stream>>>(cand, toff, table);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
        for (int j = kTableLdsK; j < Kmax; ++j) {  // ... and the high rounds, one pass each
            prof_begin(c, "otab_high");
            otab_high_kernel<<<dim3((unsigned)(ot_slots(Kmax - 1) / kB), (unsigned)n), kB, 0, c->stream>>>(cand, toff, table, j);
            prof_end(c);
            ULG_HIP(c, hipGetLastError());
        }
    }
    s.tables = true;
    return ULG_OK;
}

int order_tables_best(ulg_ctx *c, const OrderSearchState &s, const OrderMcmcState &l, const uint8_t *d_orders, int64_t count,
                      double *d_terms, uint32_t *d_ent, uint64_t *d_parents) {
    prof_begin(c, "otab_best");
    otab_best_kernel<<<flat_grid(((uint64_t)count + kB / kWave - 1) / (kB / kWave)), kB, 0, c->stream>>>(
        l.d_sets.p, l.d_offsets.p, s.d_cand.p, s.d_toff.p, s.d_table.p, l.n, d_orders, count, d_terms, d_ent, d_parents);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    return ULG_OK;
}

void order_tables_run(ulg_ctx *c, const OrderSearchState &s, const SearchArgs &a) {
    const size_t lds = (size_t)kRunWaves * (size_t)(a.n * a.n + kKickWords) * 4;  // 63,760 B at n = 63
    otab_run_kernel<<<dim3((unsigned)((a.searches + kRunWaves - 1) / kRunWaves)), kWave * kRunWaves, lds, c->stream>>>(
        a, s.d_cand.p, s.d_toff.p, s.d_table.p);
}

}  // namespace ulg
