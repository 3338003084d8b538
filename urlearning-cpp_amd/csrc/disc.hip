// disc.hip -- discrete scoring (ulg_disc_*): contingency counts of the
// records per (variable, parent set), then the score's reduction of those
// counts: n ln n terms and the penalty for BIC, lgamma terms for BDeu.
//
// Replaces, for `score -f BIC`, the reference's RecordFile / ADTree state
// (score/score_main.cpp:283-292), the AD-tree count queries
// (ad_tree/ad_tree.cpp:95-164), LogLikelihoodCalculator::calculate
// (scoring_function/log_likelihood_calculator.cpp:17-77) and
// BICScoringFunction::calculateScore (bic_scoring_function.cpp:20-76).
//
// One workgroup per (variable, parent set) work item, a grid-stride loop over
// the layer's items; an item is unranked from its colex rank within its
// variable's layer.  Two counting paths:
//   dense   q r_v <= disc_dense_cells: an int32 LDS histogram, one LDS atomic
//           per record, then one thread per parent configuration;
//   sparse  above: a hash table of the non-empty cells and parent
//           configurations (at most 2N keys in >= 4N slots), in LDS when it
//           fits, else in the workgroup's HBM slab.
// Either way the value is the sum of the terms +fix(n_jk ln n_jk) and
// -fix(n_j ln n_j) over the non-empty cells and parent configurations, where
// fix() rounds one FP64 term to a 2^-shift fixed-point integer: the terms are
// a function of the counts alone and integer adds commute, so the sum -- and
// the float it is rounded to once -- does not depend on the path, the hash
// placement or the scheduling.
//
// The reduction is a compile-time policy (BicReduce, BdeuReduce, FnmlReduce below) of
// decode_item, sparse_count, item_value and the two scoring kernels: what
// thread 0 prepares per item, the term of a cell, the term of a parent
// configuration and the float made of the integer sum.  BDeu (ULG_SCORE_BDEU,
// csrc/disc_bdeu.h) replaces BDeuScoringFunction::calculateScore and calculate
// (bdeu_scoring_function.cpp:21-35, 69-79, 117-166) with the same counting and
// its own terms [lgamma(a_jk + n_jk) - lgamma(a_jk)] and
// [lgamma(a_j) - lgamma(a_j + n_j)].  fNML (ULG_SCORE_FNML, csrc/disc_fnml.h)
// replaces fNMLScoringFunction::calculateScore and its regret table
// (fnml_scoring_function.cpp:17-74, fnml_scoring_function.h:300-340): BIC's
// n ln n terms, and per non-empty parent configuration the regret
// ln C(r_v, n_j) read from a device table that fnml_regret_kernel fills once
// per load.
//
// Option disc_prune adds the reference's prune() (score_calculator.cpp:
// 137-197, disabled in its score_main.cpp:166-171) between the last layer and
// the compaction: disc_prune_kernel below.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "disc_bdeu.h"  // BdeuItem, bdeu_cell_term, bdeu_cfg_term, bdeu_fix, bdeu_shift
#include "disc_dev.h"  // DiscData, fix_nlogn, disc_ready, disc_data
#include "disc_fnml.h"  // fnml_c2_table, fnml_c2_szpankowski, fnml_next_ratio, fnml_fix, fnml_shift, fnml_table_fits
#include "disc_prune.h"  // for_each_subset_rank, kPruneTwoEps
#include "slot_table.h"  // SlotTable, slot_table_begin / time_up / prune / compact
#include "ulg_internal.h"

using namespace ulg;

namespace {

constexpr int kDiscBlock = 256;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr unsigned long long kCfgTag = 1ull << 63;  // hash keys of parent configurations
constexpr int kHashLdsSlots = 8192;                 // 8192 x 12 B = 96 KB of the 160 KB LDS
constexpr int kScanPerThread = 8;
constexpr int kScanPerBlock = kDiscBlock * kScanPerThread;
constexpr unsigned long long kErrCode = 1ull;       // a value code >= its column's arity
constexpr int kDiscWords = kSlotWords;              // the call's words: [error word, dense sets, sparse sets, stored, pruned]

struct DiscWork {
    unsigned long long *slab;  // sparse path in HBM: hslots keys, then hslots uint32 counts, per workgroup
    uint64_t hslots;           // power of two >= 4N
    int hash_lds;              // the hash table fits LDS
    int64_t dense_cells;
    unsigned long long *word;  // [error word, dense sets, sparse sets, stored, pruned]
};

// One work item, decoded by thread 0.
struct Item {
    int v, k, rv, skip;        // skip: 1 = value known without counting
    float value;
    uint64_t q, cells, mask;
    int col[ULG_MAX_PARENTS_GPU];
    uint64_t base[ULG_MAX_PARENTS_GPU];
    BdeuItem bdeu;             // BdeuReduce only
    const long long *row;      // FnmlReduce only: the fixed regrets of arity rv, by n_j
};

// ---- the reductions ----------------------------------------------------------
// prepare(): thread 0, once per decoded item that is counted.  cell() / config():
// the fixed-point term of a count (0 for an empty one).  finish(): the value
// from the integer sum.
struct BicReduce {
    __device__ __forceinline__ void prepare(Item &) const {}
    __device__ __forceinline__ long long cell(const DiscData &D, const Item &, unsigned int c) const {
        return fix_nlogn(c, D.shift);
    }
    __device__ __forceinline__ long long config(const DiscData &D, const Item &, unsigned int nj) const {
        return -fix_nlogn(nj, D.shift);
    }
    // R4: the log-likelihood from the exact counts, the penalty, one rounding
    __device__ __forceinline__ float finish(const DiscData &D, const Item &it, long long sum) const {
        const double ll = ldexp((double)sum, -D.shift);
        const double pen = (double)(it.rv - 1) * (double)it.q * D.half_ln_N;
        return (float)(ll - pen);
    }
};

struct BdeuReduce {
    double ess;
    int shift;  // bdeu_shift(N, ess)
    __device__ __forceinline__ void prepare(Item &it) const { it.bdeu = bdeu_item(ess, it.q, it.cells); }
    __device__ __forceinline__ long long cell(const DiscData &, const Item &it, unsigned int c) const {
        return c ? bdeu_fix(bdeu_cell_term(it.bdeu, c), shift) : 0;
    }
    __device__ __forceinline__ long long config(const DiscData &, const Item &it, unsigned int nj) const {
        return nj ? bdeu_fix(bdeu_cfg_term(it.bdeu, nj), shift) : 0;
    }
    __device__ __forceinline__ float finish(const DiscData &, const Item &, long long sum) const {
        return (float)bdeu_unfix(sum, shift);
    }
};

// arity -> row of the regret table (kFnmlNoRow: no loaded column has it)
constexpr uint8_t kFnmlNoRow = 0xFF;
struct FnmlRows {
    uint8_t of[256];
};

struct FnmlReduce {
    const long long *table;  // rows ascending by arity, stride entries each: fix(ln C(r, n)), n = 0 .. N
    int64_t stride;          // N + 1
    int shift;               // fnml_shift(N, rmax)
    FnmlRows rows;
    // it.rv >= 2 here (decode_item), and every loaded arity >= 2 has a row
    __device__ __forceinline__ void prepare(Item &it) const { it.row = table + (int64_t)rows.of[it.rv] * stride; }
    __device__ __forceinline__ long long cell(const DiscData &, const Item &, unsigned int c) const {
        return fix_nlogn(c, shift);
    }
    // nj <= N: inside the row
    __device__ __forceinline__ long long config(const DiscData &, const Item &it, unsigned int nj) const {
        return nj ? -fix_nlogn(nj, shift) - it.row[nj] : 0;
    }
    __device__ __forceinline__ float finish(const DiscData &, const Item &, long long sum) const {
        return (float)fnml_unfix(sum, shift);
    }
};

__device__ __forceinline__ bool disc_violates(const uint64_t *ct, int n, int v, uint64_t set) {
    const uint64_t b = ct[v], e = ct[v + 1];
    if (b == e) return false;
    const uint64_t *p = ct + n + 1 + 2 * b;
    for (uint64_t i = 0; i < e - b; ++i)
        if ((p[2 * i] & ~set) == 0 && (p[2 * i + 1] & set) == 0) return false;
    return true;
}

// Thread 0: the item's parents (ascending variable order), bases and table
// size; R5 (arity 1) and R6 (constraints) settle the value without counting.
// The host has checked that q r_v < 2^63 for every set of the call.
template <class R>
__device__ void decode_item(const DiscData &D, const R &red, int v, uint64_t pmask, const uint64_t *cons, Item &it) {
    it.v = v;
    it.mask = pmask;
    it.rv = D.arity[v];
    int k = 0;
    uint64_t q = 1;
    for (uint64_t m = pmask; m; m &= m - 1) {
        const int p = __builtin_ctzll(m);
        it.col[k] = p;
        it.base[k] = q;
        q *= (uint64_t)D.arity[p];
        ++k;
    }
    it.k = k;
    it.q = q;
    it.cells = q * (uint64_t)it.rv;
    it.skip = 0;
    if (cons && disc_violates(cons, D.n, v, pmask)) {
        it.skip = 1;
        it.value = 1.0f;  // bic_scoring_function.cpp:34-37
    } else if (it.rv == 1) {
        it.skip = 1;
        it.value = 0.0f;  // penalty 0, log-likelihood 0; BDeu: every cell term cancels its configuration's
    } else {
        red.prepare(it);
    }
}

__device__ __forceinline__ uint64_t cell_of(const DiscData &D, const Item &it, int64_t r, uint64_t &cfg) {
    uint64_t j = 0;
    for (int a = 0; a < it.k; ++a) j += (uint64_t)D.codes[(int64_t)it.col[a] * D.N + r] * it.base[a];
    cfg = j;
    return j + (uint64_t)D.codes[(int64_t)it.v * D.N + r] * it.q;
}

// Counts the item's records in the hash table (keys / cnt, hslots entries) and
// adds the fixed-point terms to *acc; counts_out (optional) receives the
// non-empty cells of the dense table.
template <class R, class KP, class CP>
__device__ __forceinline__ void sparse_count(const DiscData &D, const R &red, const Item &it, KP keys, CP cnt,
                                             uint64_t hslots, unsigned long long *acc, int32_t *counts_out) {
    const int tid = threadIdx.x;
    for (uint64_t h = tid; h < hslots; h += kDiscBlock) {
        keys[h] = kEmptyKey;
        cnt[h] = 0u;
    }
    __syncthreads();
    const uint64_t hm = hslots - 1;
    for (int64_t r = tid; r < D.N; r += kDiscBlock) {
        uint64_t cfg;
        const uint64_t cell = cell_of(D, it, r, cfg);
        const unsigned long long two[2] = {cell, cfg | kCfgTag};
        for (int t = 0; t < 2; ++t) {
            const unsigned long long key = two[t];
            uint64_t h = (key * 0x9E3779B97F4A7C15ull >> 20) & hm;
            // at most 2N distinct keys in >= 4N slots: a free slot is always reached
            for (;;) {
                const unsigned long long prev = atomicCAS(&keys[h], kEmptyKey, key);
                if (prev == kEmptyKey || prev == key) break;
                h = (h + 1) & hm;
            }
            atomicAdd(&cnt[h], 1u);
        }
    }
    __syncthreads();
    long long a = 0;
    for (uint64_t h = tid; h < hslots; h += kDiscBlock) {
        const unsigned long long key = keys[h];
        if (key == kEmptyKey) continue;
        const unsigned int c = cnt[h];
        if (key & kCfgTag) {
            a += red.config(D, it, c);
        } else {
            a += red.cell(D, it, c);
            if (counts_out) counts_out[key] = (int32_t)c;
        }
    }
    if (a) atomicAdd(acc, (unsigned long long)a);
    __syncthreads();
}

// The whole workgroup: the value of the decoded item `it` (in LDS).  smem:
// the dynamic LDS behind the item (histogram or hash table).  counts_out
// (optional, zeroed by the caller, it.cells entries): the dense table.
template <class R>
__device__ float item_value(const DiscData &D, const DiscWork &W, const R &red, const Item &it,
                            unsigned long long *acc, unsigned char *smem, int32_t *counts_out, bool count_path) {
    const int tid = threadIdx.x;
    if (it.skip && !counts_out) return it.value;
    if (tid == 0) *acc = 0ull;
    __syncthreads();
    if (it.cells <= (uint64_t)W.dense_cells) {
        int *hist = reinterpret_cast<int *>(smem);
        const int cells = (int)it.cells;
        for (int i = tid; i < cells; i += kDiscBlock) hist[i] = 0;
        __syncthreads();
        for (int64_t r = tid; r < D.N; r += kDiscBlock) {
            uint64_t cfg;
            const uint64_t cell = cell_of(D, it, r, cfg);
            atomicAdd(&hist[(int)cell], 1);  // cell < cells: every code is below its arity (checked at load)
        }
        __syncthreads();
        long long a = 0;
        const int q = (int)it.q;
        for (int j = tid; j < q; j += kDiscBlock) {
            unsigned int nj = 0;
            for (int kk = 0; kk < it.rv; ++kk) {
                const unsigned int c = (unsigned int)hist[j + kk * q];
                nj += c;
                a += red.cell(D, it, c);
            }
            a += red.config(D, it, nj);
        }
        if (a) atomicAdd(acc, (unsigned long long)a);
        if (counts_out)
            for (int i = tid; i < cells; i += kDiscBlock) counts_out[i] = hist[i];
        if (count_path && tid == 0) atomicAdd(&W.word[1], 1ull);
        __syncthreads();
    } else {
        if (W.hash_lds) {
            unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);
            unsigned int *cnt = reinterpret_cast<unsigned int *>(keys + W.hslots);
            sparse_count(D, red, it, keys, cnt, W.hslots, acc, counts_out);
        } else {
            unsigned long long *keys = W.slab + (uint64_t)blockIdx.x * (W.hslots + W.hslots / 2);
            unsigned int *cnt = reinterpret_cast<unsigned int *>(keys + W.hslots);
            sparse_count(D, red, it, keys, cnt, W.hslots, acc, counts_out);
        }
        if (count_path && tid == 0) atomicAdd(&W.word[2], 1ull);
    }
    if (it.skip) return it.value;
    return red.finish(D, it, (long long)*acc);
}

// ---- upload check ------------------------------------------------------------
__global__ void __launch_bounds__(kDiscBlock) disc_check_kernel(DiscData D, unsigned long long *word) {
    const int64_t total = D.N * (int64_t)D.n;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kDiscBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kDiscBlock)
        bad |= D.codes[i] >= D.arity[(int)(i / D.N)];
    if (bad) atomicOr(word, kErrCode);
}

// ---- the regret table of fNML ----------------------------------------------------
// One lane per n = 0 .. N: the ratio recurrence of disc_fnml.h from rho_2 =
// C(2, n) (c2[n] for n <= kFnmlExact, Szpankowski's form above) up to arity
// rmax, storing fix(ln C(k, n)) at every k that has a row.  Row `of[k]` is
// N + 1 contiguous entries, so the lanes of a wave store side by side.
__global__ void __launch_bounds__(kDiscBlock)
fnml_regret_kernel(const double *c2, int64_t N, int rmax, int shift, FnmlRows rows, long long *table) {
    const int64_t n = (int64_t)blockIdx.x * kDiscBlock + threadIdx.x;
    if (n > N) return;
    const int64_t stride = N + 1;
    double rho = n <= kFnmlExact ? c2[n] : fnml_c2_szpankowski((double)n);
    double lc = log(rho);  // n = 0: C(k, 0) = 1 for every k, every ratio is 1
    if (rows.of[2] != kFnmlNoRow) table[(int64_t)rows.of[2] * stride + n] = fnml_fix(lc, shift);
    for (int k = 3; k <= rmax; ++k) {
        rho = fnml_next_ratio(rho, (double)n, k);
        lc += log(rho);
        if (rows.of[k] != kFnmlNoRow) table[(int64_t)rows.of[k] * stride + n] = fnml_fix(lc, shift);
    }
}

// ---- one layer ---------------------------------------------------------------
struct LayerArgs {
    const uint8_t *cand;     // [nv][64] compact index -> variable
    const int *vm;           // [nv][2]: variable, candidate count
    const uint64_t *toff;    // [nv * S + 1] slot prefixes
    const uint64_t *work;    // [nv + 1] this layer's item prefixes
    const uint64_t *binom64; // [64][64]
    const uint64_t *cons;    // by variable, or null
    float *table;            // per slot: the stored value, or absent
    uint64_t *sets;          // per slot: the set's variable mask
    int nv, S, L;
};

template <class R>
__global__ void __launch_bounds__(kDiscBlock) disc_layer_kernel(DiscData D, DiscWork W, LayerArgs A, R red) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ Item it;
    __shared__ unsigned long long acc;
    __shared__ uint64_t slot;
    const uint64_t total = A.work[A.nv];
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        __syncthreads();  // the previous item's LDS is done with
        if (threadIdx.x == 0) {
            int i = 0;
            while (i + 1 < A.nv && A.work[i + 1] <= w) ++i;
            uint64_t r = w - A.work[i];
            // colex unrank over the variable's compact candidate indices
            const int m = A.vm[2 * i + 1];
            uint64_t pmask = 0;
            int c = m - 1;
            for (int e = A.L; e >= 1; --e) {
                while (c > e - 1 && A.binom64[c * 64 + e] > r) --c;
                r -= A.binom64[c * 64 + e];
                pmask |= 1ull << A.cand[i * 64 + c];
                --c;
            }
            slot = A.toff[(uint64_t)i * A.S + A.L] + (w - A.work[i]);
            decode_item(D, red, A.vm[2 * i], pmask, A.cons, it);
        }
        __syncthreads();
        const float val = item_value(D, W, red, it, &acc, smem, nullptr, true);
        if (threadIdx.x == 0) {
            // R3: the empty set is stored iff < 1, every other set iff < 0
            const bool keep = A.L == 0 ? val < 1.0f : val < 0.0f;
            A.table[slot] = keep ? val : __uint_as_float(kAbsentBits);
            A.sets[slot] = it.mask;
        }
    }
}

// ---- prune pass (option disc_prune) ------------------------------------------
// R8, the reference's prune() (score_calculator.cpp:137-197) per variable: a
// stored set P goes iff a kept proper subset Q has (float)(s(Q) - s(P)) >=
// -2 FLT_EPSILON.  best[slot] = the largest kept score among the slot's set
// and all its subsets (-inf: none); a hole (violating or arity-1 set) stores
// nothing of its own but passes its subsets' maximum on, so every kept proper
// subset of P is seen through P's L immediate subsets.  One launch per layer
// (layer L reads best of layer L - 1), one slot per thread: it alone reads and
// writes table[slot] and best[slot] in this launch.
struct PruneArgs {
    const int *vm;           // [nv][2]: variable, candidate count
    const uint64_t *toff;    // [nv * S + 1] slot prefixes
    const uint64_t *work;    // [nv + 1] this layer's item prefixes
    const uint64_t *binom64; // [64][64]
    float *table;            // per slot: the stored value, or absent
    float *best;             // per slot: B
    unsigned long long *pruned;
    int nv, S, L;
};

__global__ void __launch_bounds__(kDiscBlock) disc_prune_kernel(PruneArgs A) {
    const uint64_t total = A.work[A.nv];
    unsigned int gone = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * kDiscBlock + threadIdx.x; w < total; w += (uint64_t)gridDim.x * kDiscBlock) {
        // the variable: the last i with work[i] <= w (w < work[nv], so i < nv)
        int lo = 0, hi = A.nv;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (A.work[mid] <= w) lo = mid; else hi = mid;
        }
        const int i = lo;
        const uint64_t r = w - A.work[i];
        const uint64_t slot = A.toff[(uint64_t)i * A.S + A.L] + r;
        float M = -INFINITY;
        if (A.L > 0) {
            const float *below = A.best + A.toff[(uint64_t)i * A.S + A.L - 1];  // slab (i, L - 1): C(m, L - 1) slots
            for_each_subset_rank(A.binom64, A.vm[2 * i + 1], A.L, r,
                                 [&](int, int, uint64_t sub) { M = fmaxf(M, below[sub]); });
        }
        const float own = A.table[slot];
        float B = M;
        if (__float_as_uint(own) != kAbsentBits) {
            if (__fsub_rn(M, own) < -kPruneTwoEps) {  // M = -inf: no kept subset
                B = fmaxf(M, own);
            } else {
                A.table[slot] = __uint_as_float(kAbsentBits);
                ++gone;
            }
        }
        A.best[slot] = B;
    }
    // every lane is here: one add per wave
    for (int d = 32; d >= 1; d >>= 1) gone += __shfl_down(gone, d, 64);
    if ((threadIdx.x & 63) == 0 && gone) atomicAdd(A.pruned, (unsigned long long)gone);
}

// ---- arbitrary pairs / one table ---------------------------------------------
template <class R>
__global__ void __launch_bounds__(kDiscBlock)
disc_sets_kernel(DiscData D, DiscWork W, const uint64_t *pairs, int64_t count, const uint64_t *cons, float *out,
                 int32_t *counts_out, R red) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ Item it;
    __shared__ unsigned long long acc;
    for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
        __syncthreads();
        if (threadIdx.x == 0) decode_item(D, red, (int)pairs[2 * w], pairs[2 * w + 1], cons, it);
        __syncthreads();
        const float val = item_value(D, W, red, it, &acc, smem, counts_out, false);
        if (threadIdx.x == 0 && out) out[w] = val;
    }
}

// ---- compaction in slot (= rank) order -----------------------------------------
__global__ void __launch_bounds__(kDiscBlock)
disc_count_kernel(const float *table, uint64_t total, unsigned long long *blk) {
    __shared__ unsigned int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    const uint64_t b0 = (uint64_t)blockIdx.x * kScanPerBlock + (uint64_t)threadIdx.x * kScanPerThread;
    unsigned int cnt = 0;
    for (int j = 0; j < kScanPerThread; ++j)
        if (b0 + j < total && __float_as_uint(table[b0 + j]) != kAbsentBits) ++cnt;
    if (cnt) atomicAdd(&s, cnt);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s;
}

// one workgroup: exclusive scan of the block counts, total into blk[nb] and word[3]
__global__ void __launch_bounds__(kDiscBlock)
disc_scan_kernel(unsigned long long *blk, int64_t nb, unsigned long long *word) {
    __shared__ unsigned long long part[kDiscBlock];
    const int tid = threadIdx.x;
    const int64_t per = (nb + kDiscBlock - 1) / kDiscBlock;
    const int64_t b = std::min<int64_t>(nb, (int64_t)tid * per), e = std::min<int64_t>(nb, b + per);
    unsigned long long s = 0;
    for (int64_t i = b; i < e; ++i) s += blk[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < kDiscBlock; ++i) {
            const unsigned long long t = part[i];
            part[i] = run;
            run += t;
        }
        blk[nb] = run;
        word[3] = run;
    }
    __syncthreads();
    unsigned long long run = part[tid];
    for (int64_t i = b; i < e; ++i) {
        const unsigned long long t = blk[i];
        blk[i] = run;
        run += t;
    }
}

__global__ void __launch_bounds__(kDiscBlock)
disc_write_kernel(const float *table, const uint64_t *sets, uint64_t total, const unsigned long long *blk,
                  uint64_t *out_sets, float *out_scores) {
    __shared__ unsigned int pre[kDiscBlock];
    const int tid = threadIdx.x;
    const uint64_t b0 = (uint64_t)blockIdx.x * kScanPerBlock + (uint64_t)tid * kScanPerThread;
    unsigned int cnt = 0;
    for (int j = 0; j < kScanPerThread; ++j)
        if (b0 + j < total && __float_as_uint(table[b0 + j]) != kAbsentBits) ++cnt;
    pre[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned int run = 0;
        for (int i = 0; i < kDiscBlock; ++i) {
            const unsigned int t = pre[i];
            pre[i] = run;
            run += t;
        }
    }
    __syncthreads();
    unsigned long long o = blk[blockIdx.x] + pre[tid];
    for (int j = 0; j < kScanPerThread; ++j)
        if (b0 + j < total && __float_as_uint(table[b0 + j]) != kAbsentBits) {
            out_sets[o] = sets[b0 + j];
            out_scores[o] = table[b0 + j];
            ++o;
        }
}

// offsets[i] = stored sets below slot toff[i * S] (i = nv: all of them)
__global__ void disc_offsets_kernel(const float *table, const uint64_t *toff, int nv, int S,
                                    const unsigned long long *blk, int64_t *offsets) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nv) return;
    const uint64_t s = toff[(uint64_t)i * S];
    const uint64_t b = s / kScanPerBlock;
    unsigned long long o = blk[b];  // slot == total: b may be nb, the total
    for (uint64_t j = b * kScanPerBlock; j < s; ++j)
        if (__float_as_uint(table[j]) != kAbsentBits) ++o;
    offsets[i] = (int64_t)o;
}

// ---- host ----------------------------------------------------------------------
// q r_v of (v, parents), or 2^63 where it does not fit
uint64_t table_cells(const ulg_ctx *c, int v, uint64_t parents) {
    unsigned __int128 cells = (unsigned)c->disc_arity[v];
    for (uint64_t m = parents; m; m &= m - 1) {
        cells *= (unsigned)c->disc_arity[__builtin_ctzll(m)];
        if (cells >> 63) return 1ull << 63;
    }
    return (uint64_t)cells;
}

// The counting resources of a launch whose largest table has max_cells cells:
// the dynamic LDS, and the HBM slabs when the hash table does not fit LDS
// (which bounds the grid).
int disc_work(ulg_ctx *c, uint64_t max_cells, uint64_t items, DiscWork &W, size_t &lds, unsigned &grid) {
    W = DiscWork{};
    W.dense_cells = c->opt.disc_dense_cells;
    W.word = c->d_disc_word.p;
    uint64_t hs = 64;
    while (hs < 4ull * (uint64_t)c->N) hs <<= 1;
    W.hslots = hs;
    W.hash_lds = hs <= (uint64_t)kHashLdsSlots;
    const bool sparse = max_cells > (uint64_t)W.dense_cells;
    lds = (size_t)std::min<uint64_t>(max_cells, (uint64_t)W.dense_cells) * 4;
    if (sparse && W.hash_lds) lds = std::max(lds, (size_t)hs * 12);
    lds = std::max<size_t>(lds, 16);
    uint64_t g = std::min<uint64_t>(std::max<uint64_t>(items, 1), 2048);
    if (sparse && !W.hash_lds) {
        const uint64_t per = hs + hs / 2;  // words per workgroup
        g = std::min<uint64_t>(g, std::max<uint64_t>(1, (1ull << 28) / per));  // at most 2 GiB of slabs
        if (int rc = ensure(c, c->d_disc_slab, (size_t)(g * per))) return rc;
        W.slab = c->d_disc_slab.p;
    }
    grid = (unsigned)g;
    return ULG_OK;
}

bool kind_ok(int kind) { return kind == ULG_SCORE_BIC || kind == ULG_SCORE_BDEU || kind == ULG_SCORE_FNML; }

BdeuReduce bdeu_reduce(const ulg_ctx *c) { return BdeuReduce{c->disc_ess, bdeu_shift(c->N, c->disc_ess)}; }

// The rows of the loaded columns: one per distinct arity >= 2, ascending.
int fnml_rows(const ulg_ctx *c, FnmlRows &R, int &rmax) {
    std::memset(R.of, kFnmlNoRow, sizeof R.of);
    bool has[256] = {};
    for (int a : c->disc_arity) has[a] = true;
    int rows = 0;
    rmax = 1;
    for (int a = 2; a < 256; ++a)
        if (has[a]) {
            R.of[a] = (uint8_t)rows++;
            rmax = a;
        }
    return rows;
}

// The regret table of the loaded data, built at the first fNML call after a
// ulg_disc_load and kept until the next load of either kind (fnml_drop).
int fnml_ensure_table(ulg_ctx *c, const char *who) {
    if (c->fnml_built) return ULG_OK;
    FnmlRows R;
    int rmax = 1;
    const int rows = fnml_rows(c, R, rmax);
    if (!fnml_table_fits(rows, c->N))
        return set_err(c, ULG_ERR_UNSUPPORTED, std::string(who) + ": the fNML regret table would hold more than 2^28 entries");
    const size_t entries = (size_t)rows * (size_t)(c->N + 1);
    if (rows) {
        const std::vector<double> &c2 = fnml_c2_table();
        int rc;
        if ((rc = ensure(c, c->d_fnml_c2, c2.size())) || (rc = ensure(c, c->d_fnml, entries))) return rc;
        // a static source: it outlives the copy
        ULG_HIP(c, hipMemcpyAsync(c->d_fnml_c2.p, c2.data(), c2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        prof_begin(c, "fnml_regret");
        fnml_regret_kernel<<<(unsigned)((c->N + 1 + kDiscBlock - 1) / kDiscBlock), kDiscBlock, 0, c->stream>>>(
            c->d_fnml_c2.p, c->N, rmax, fnml_shift(c->N, rmax), R, c->d_fnml.p);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    c->fnml_built = true;
    c->fnml_bytes = (int64_t)(entries * sizeof(long long));
    return ULG_OK;
}

FnmlReduce fnml_reduce(const ulg_ctx *c) {
    FnmlReduce red{};
    int rmax = 1;
    (void)fnml_rows(c, red.rows, rmax);
    red.table = c->d_fnml.p;
    red.stride = c->N + 1;
    red.shift = fnml_shift(c->N, rmax);
    return red;
}

}  // namespace

// ---- the score-agnostic steps (slot_table.h) -------------------------------------
namespace ulg {

void SlotTable::build(const ScoreLists &ls) {
    nv = ls.nv;
    S = ls.S;
    total_slots = ls.total_slots;
    nb = (int64_t)((total_slots + kScanPerBlock - 1) / kScanPerBlock);
    vm.assign((size_t)nv * 2, 0);
    for (int i = 0; i < nv; ++i) {
        vm[2 * i] = ls.vars[i];
        vm[2 * i + 1] = ls.mv[i];
    }
    // [toff: nv * S + 1][work: S x (nv + 1)]
    meta.assign((size_t)nv * S + 1 + (size_t)S * (nv + 1), 0);
    std::copy(ls.toff.begin(), ls.toff.end(), meta.begin());
    uint64_t *work = meta.data() + (size_t)nv * S + 1;
    for (int L = 0; L < S; ++L) {
        uint64_t s = 0;
        for (int i = 0; i < nv; ++i) {
            work[(size_t)L * (nv + 1) + i] = s;
            s += ls.slab_count(i, L);
        }
        work[(size_t)L * (nv + 1) + nv] = s;
    }
}

int slot_table_begin(ulg_ctx *c, const ScoreLists &ls, const SlotTable &st) {
    const std::vector<uint8_t> &cand = ls.cand;
    const uint64_t total_slots = st.total_slots;
    int rc;
    // the slot table and the block counts live in buffers of the scorers; the
    // context's lists are replaced only once every layer has been launched
    if ((rc = ensure(c, c->d_disc_meta, st.meta.size())) || (rc = ensure(c, c->d_disc_cand, cand.size())) ||
        (rc = ensure(c, c->d_disc_vm, st.vm.size())) || (rc = ensure(c, c->d_disc_table, total_slots)) ||
        (rc = ensure(c, c->d_disc_sets, total_slots)) || (rc = ensure(c, c->d_disc_blk, (size_t)st.nb + 1)) ||
        (rc = ensure(c, c->d_disc_word, kDiscWords)))
        return rc;
    ULG_HIP(c, hipMemcpyAsync(c->d_disc_meta.p, st.meta.data(), st.meta.size() * 8, hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemcpyAsync(c->d_disc_cand.p, cand.data(), cand.size(), hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemcpyAsync(c->d_disc_vm.p, st.vm.data(), st.vm.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemsetAsync(c->d_disc_table.p, 0xFF, total_slots * sizeof(float), c->stream));  // absent
    ULG_HIP(c, hipMemsetAsync(c->d_disc_word.p, 0, kDiscWords * sizeof(unsigned long long), c->stream));
    // pageable sources: the copies above must be done before `st` goes away
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    return ULG_OK;
}

int slot_table_time_up(ulg_ctx *c, std::chrono::steady_clock::time_point t_call, bool *up) {
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    *up = ms > (double)c->opt.time_limit_ms;
    return ULG_OK;
}

int slot_table_prune(ulg_ctx *c, const SlotTable &st, int done_L) {
    // the completed layers only: nothing above done_L was stored
    int rc;
    if ((rc = ensure(c, c->d_disc_best, st.total_slots))) return rc;
    PruneArgs P{};
    P.vm = c->d_disc_vm.p;
    P.toff = c->d_disc_meta.p;
    P.binom64 = c->d_binom64.p;
    P.table = c->d_disc_table.p;
    P.best = c->d_disc_best.p;
    P.pruned = c->d_disc_word.p + 4;
    P.nv = st.nv;
    P.S = st.S;
    for (int L = 0; L <= done_L; ++L) {
        const uint64_t items = st.items(L);
        if (!items) continue;
        P.L = L;
        P.work = c->d_disc_meta.p + st.work_at(L);
        prof_begin(c, "disc_prune");
        disc_prune_kernel<<<(unsigned)std::min<uint64_t>((items + kDiscBlock - 1) / kDiscBlock, 2048), kDiscBlock, 0,
                            c->stream>>>(P);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    return ULG_OK;
}

int slot_table_compact(ulg_ctx *c, const SlotTable &st, unsigned long long (&word)[kSlotWords]) {
    const uint64_t total_slots = st.total_slots;
    const int64_t nb = st.nb;
    const int nv = st.nv, S = st.S;
    int rc;
    if ((rc = ensure(c, c->out_sets, total_slots)) || (rc = ensure(c, c->out_scores, total_slots)) ||
        (rc = ensure(c, c->out_offsets, (size_t)nv + 1)))
        return rc;
    prof_begin(c, "disc_compact");
    disc_count_kernel<<<(unsigned)nb, kDiscBlock, 0, c->stream>>>(c->d_disc_table.p, total_slots, c->d_disc_blk.p);
    disc_scan_kernel<<<1, kDiscBlock, 0, c->stream>>>(c->d_disc_blk.p, nb, c->d_disc_word.p);
    disc_write_kernel<<<(unsigned)nb, kDiscBlock, 0, c->stream>>>(c->d_disc_table.p, c->d_disc_sets.p, total_slots,
                                                                 c->d_disc_blk.p, c->out_sets.p, c->out_scores.p);
    disc_offsets_kernel<<<(nv + 1 + 63) / 64, 64, 0, c->stream>>>(c->d_disc_table.p, c->d_disc_meta.p, nv, S,
                                                                 c->d_disc_blk.p, c->out_offsets.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    for (unsigned long long &w : word) w = 0;
    ULG_HIP(c, hipMemcpyAsync(word, c->d_disc_word.p, sizeof word, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ULG_OK;
}

}  // namespace ulg

extern "C" {

int ulg_disc_load(ulg_ctx *c, const uint8_t *codes, int64_t N, int n, const int *arity) {
    if (!c) return ULG_ERR_ARG;
    if (!codes || !arity || N < 2 || N >= (1ll << 31) || n < 1 || n > kMaxVars)
        return set_err(c, ULG_ERR_ARG, "ulg_disc_load: bad arguments");
    for (int j = 0; j < n; ++j)
        if (arity[j] < 1 || arity[j] > 255) return set_err(c, ULG_ERR_ARG, "ulg_disc_load: arity must be 1..255");
    if (int rc0 = finish_pending(c)) return rc0;
    ULG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->d_codes, (size_t)(N * n))) || (rc = ensure(c, c->d_disc_word, kDiscWords))) return rc;
    c->disc_loaded = false;  // the previous codes are gone
    fnml_drop(c);            // ... and the regret table made for them
    ULG_HIP(c, hipMemcpyAsync(c->d_codes.p, codes, (size_t)(N * n), hipMemcpyHostToDevice, c->stream));
    ULG_HIP(c, hipMemsetAsync(c->d_disc_word.p, 0, kDiscWords * sizeof(unsigned long long), c->stream));
    DiscData D{};
    D.codes = c->d_codes.p;
    D.N = N;
    D.n = n;
    for (int j = 0; j < n; ++j) D.arity[j] = (uint8_t)arity[j];
    const int64_t total = N * n;
    prof_begin(c, "disc_check");
    disc_check_kernel<<<(unsigned)std::min<int64_t>((total + kDiscBlock - 1) / kDiscBlock, 4096), kDiscBlock, 0,
                        c->stream>>>(D, c->d_disc_word.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    unsigned long long word = 0;
    ULG_HIP(c, hipMemcpyAsync(&word, c->d_disc_word.p, sizeof word, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (word & kErrCode) return set_err(c, ULG_ERR_ARG, "ulg_disc_load: a value code is not below its column's arity");
    // the context now holds these records: the continuous data, the lists
    // scored from the previous data and its constraints are gone
    c->loaded = false;
    c->scored = false;
    if (!c->cons_var.empty()) {
        graph_reset(c);
        c->cons_var.clear();
        c->cons_req.clear();
        c->cons_forb.clear();
    }
    c->n = n;
    c->N = N;
    c->disc_arity.assign(arity, arity + n);
    c->disc_loaded = true;
    return ULG_OK;
}

int ulg_disc_score(ulg_ctx *c, int kind, const int *vars, int nv, const uint64_t *candidates, int max_parents,
                   int64_t *total_stored, int64_t *total_scored) {
    if (!c) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!disc_ready(c)) return set_err(c, ULG_ERR_STATE, "ulg_disc_score: call ulg_disc_load first");
    if (!kind_ok(kind)) return set_err(c, ULG_ERR_ARG, "ulg_disc_score: kind must be ULG_SCORE_BIC, ULG_SCORE_BDEU or ULG_SCORE_FNML");
    ScoreLists &ls = c->lists;
    const ScoreLists::Status st = ls.build(c->n, vars, nv, candidates, max_parents);
    if (st != ScoreLists::kOk && st != ScoreLists::kTooWide) return lists_error(c, "ulg_disc_score", st);
    uint64_t max_cells = 0;
    for (int i = 0; i < nv; ++i) {
        const int m = ls.mv[i];
        std::vector<int> ar(m);
        for (int j = 0; j < m; ++j) ar[j] = c->disc_arity[ls.cand[(size_t)i * 64 + j]];
        const int k = std::min(m, ls.max_parents);
        // the variable's largest table: its k candidates of largest arity
        std::sort(ar.begin(), ar.end(), std::greater<int>());
        unsigned __int128 cells = (unsigned)c->disc_arity[vars[i]];
        for (int j = 0; j < k && !(cells >> 63); ++j) cells *= (unsigned)ar[j];
        if ((cells >> 63) && c->disc_arity[vars[i]] > 1)
            return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_disc_score: a contingency table of 2^63 cells or more");
        if (c->disc_arity[vars[i]] > 1) max_cells = std::max(max_cells, (uint64_t)cells);
    }
    if (st != ScoreLists::kOk) return lists_error(c, "ulg_disc_score", st);
    const int kmax = ls.kmax, S = ls.S;
    SlotTable tb;
    tb.build(ls);
    ULG_HIP(c, hipSetDevice(c->device));
    int rc;
    const bool bdeu = kind == ULG_SCORE_BDEU, fnml = kind == ULG_SCORE_FNML;
    if (fnml && (rc = fnml_ensure_table(c, "ulg_disc_score"))) return rc;
    if ((rc = slot_table_begin(c, ls, tb))) return rc;
    DiscWork W;
    size_t lds = 0;
    unsigned grid_cap = 1;
    if ((rc = disc_work(c, max_cells, tb.total_slots, W, lds, grid_cap))) return rc;
    // each instantiation is a kernel of its own, with its own attribute
    const void *layer_fn = bdeu   ? (const void *)disc_layer_kernel<BdeuReduce>
                           : fnml ? (const void *)disc_layer_kernel<FnmlReduce>
                                  : (const void *)disc_layer_kernel<BicReduce>;
    ULG_HIP(c, hipFuncSetAttribute(layer_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    const DiscData D = disc_data(c);
    LayerArgs A{};
    A.cand = c->d_disc_cand.p;
    A.vm = c->d_disc_vm.p;
    A.toff = c->d_disc_meta.p;
    A.binom64 = c->d_binom64.p;
    A.cons = c->cons_var.empty() ? nullptr : c->d_cons_var.p;
    A.table = c->d_disc_table.p;
    A.sets = c->d_disc_sets.p;
    A.nv = nv;
    A.S = S;
    // -r (score_calculator.cpp:33-52,78): checked after every complete layer
    const auto t_call = std::chrono::steady_clock::now();
    c->out_of_time = 0;
    int done_L = kmax;
    for (int L = 0; L <= kmax; ++L) {
        const uint64_t items = tb.items(L);
        if (items) {
            A.L = L;
            A.work = c->d_disc_meta.p + tb.work_at(L);
            prof_begin(c, "disc_layer");
            const unsigned grid = (unsigned)std::min<uint64_t>(items, grid_cap);
            if (bdeu)
                disc_layer_kernel<BdeuReduce><<<grid, kDiscBlock, lds, c->stream>>>(D, W, A, bdeu_reduce(c));
            else if (fnml)
                disc_layer_kernel<FnmlReduce><<<grid, kDiscBlock, lds, c->stream>>>(D, W, A, fnml_reduce(c));
            else
                disc_layer_kernel<BicReduce><<<grid, kDiscBlock, lds, c->stream>>>(D, W, A, BicReduce{});
            prof_end(c);
            ULG_HIP(c, hipGetLastError());
        }
        if (c->opt.time_limit_ms > 0 && L < kmax) {
            bool up = false;
            if ((rc = slot_table_time_up(c, t_call, &up))) return rc;
            if (up) {
                done_L = L;
                c->out_of_time = 1;
                break;
            }
        }
    }
    c->completed_layer = done_L;
    if (c->opt.disc_prune && (rc = slot_table_prune(c, tb, done_L))) return rc;
    unsigned long long word[kDiscWords];
    if ((rc = slot_table_compact(c, tb, word))) return rc;
    c->last_err_word = 0;
    c->disc_path_sets[0] = (int64_t)word[1];
    c->disc_path_sets[1] = (int64_t)word[2];
    c->disc_pruned = (int64_t)word[4];
    publish(c, ls, (int64_t)word[3], false);
    if (total_stored) *total_stored = c->total_stored;
    if (total_scored) *total_scored = c->total_scored;
    return ULG_OK;
}

// the pairs on the device, the counting resources and one launch of disc_sets_kernel
static int disc_sets_launch(ulg_ctx *c, const char *what, int kind, int64_t count, const int *vars,
                            const uint64_t *parents, float *out_dev, int32_t *counts_dev) {
    const int n = c->n;
    const uint64_t allmask = (1ull << n) - 1ull;
    std::vector<uint64_t> pairs((size_t)count * 2);
    uint64_t max_cells = 0;
    for (int64_t i = 0; i < count; ++i) {
        if (vars[i] < 0 || vars[i] >= n) return set_err(c, ULG_ERR_ARG, std::string(what) + ": variable out of range");
        if (parents[i] & ~allmask) return set_err(c, ULG_ERR_ARG, std::string(what) + ": parent bit >= n");
        const uint64_t P = parents[i] & ~(1ull << vars[i]);
        if (__builtin_popcountll(P) > kWideMax)
            return set_err(c, ULG_ERR_UNSUPPORTED, std::string(what) + ": more than ULG_MAX_PARENTS_GPU (31) parents");
        const uint64_t cells = table_cells(c, vars[i], P);
        if (cells >> 63) {
            if (c->disc_arity[vars[i]] > 1 || counts_dev)
                return set_err(c, ULG_ERR_UNSUPPORTED, std::string(what) + ": a contingency table of 2^63 cells or more");
        } else if (c->disc_arity[vars[i]] > 1 || counts_dev) {
            max_cells = std::max(max_cells, cells);
        }
        pairs[2 * i] = (uint64_t)vars[i];
        pairs[2 * i + 1] = P;
    }
    ULG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->d_sets_in, (size_t)count * 2)) || (rc = ensure(c, c->d_disc_word, kDiscWords))) return rc;
    DiscWork W;
    size_t lds = 0;
    unsigned grid = 1;
    if ((rc = disc_work(c, max_cells, (uint64_t)count, W, lds, grid))) return rc;
    const bool bdeu = kind == ULG_SCORE_BDEU, fnml = kind == ULG_SCORE_FNML;
    if (fnml && (rc = fnml_ensure_table(c, what))) return rc;
    const void *sets_fn = bdeu   ? (const void *)disc_sets_kernel<BdeuReduce>
                          : fnml ? (const void *)disc_sets_kernel<FnmlReduce>
                                 : (const void *)disc_sets_kernel<BicReduce>;
    ULG_HIP(c, hipFuncSetAttribute(sets_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ULG_HIP(c, hipMemcpyAsync(c->d_sets_in.p, pairs.data(), (size_t)count * 16, hipMemcpyHostToDevice, c->stream));
    prof_begin(c, "disc_sets");
    const uint64_t *cons = c->cons_var.empty() || counts_dev ? nullptr : c->d_cons_var.p;
    if (bdeu)
        disc_sets_kernel<BdeuReduce><<<grid, kDiscBlock, lds, c->stream>>>(disc_data(c), W, c->d_sets_in.p, count, cons,
                                                                           out_dev, counts_dev, bdeu_reduce(c));
    else if (fnml)
        disc_sets_kernel<FnmlReduce><<<grid, kDiscBlock, lds, c->stream>>>(disc_data(c), W, c->d_sets_in.p, count, cons,
                                                                           out_dev, counts_dev, fnml_reduce(c));
    else
        disc_sets_kernel<BicReduce><<<grid, kDiscBlock, lds, c->stream>>>(disc_data(c), W, c->d_sets_in.p, count, cons,
                                                                          out_dev, counts_dev, BicReduce{});
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    ULG_HIP(c, hipStreamSynchronize(c->stream));  // `pairs` is a pageable source
    prof_collect(c);
    return ULG_OK;
}

int ulg_disc_score_sets(ulg_ctx *c, int kind, int64_t count, const int *vars, const uint64_t *parents,
                        float *scores) {
    if (!c || count < 0 || (count > 0 && (!vars || !parents || !scores))) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!disc_ready(c)) return set_err(c, ULG_ERR_STATE, "ulg_disc_score_sets: call ulg_disc_load first");
    if (!kind_ok(kind))
        return set_err(c, ULG_ERR_ARG, "ulg_disc_score_sets: kind must be ULG_SCORE_BIC, ULG_SCORE_BDEU or ULG_SCORE_FNML");
    if (count == 0) return ULG_OK;
    int rc;
    if ((rc = ensure(c, c->qbuf_out, (size_t)count))) return rc;
    if ((rc = disc_sets_launch(c, "ulg_disc_score_sets", kind, count, vars, parents, c->qbuf_out.p, nullptr))) return rc;
    ULG_HIP(c, hipMemcpy(scores, c->qbuf_out.p, (size_t)count * 4, hipMemcpyDeviceToHost));
    return ULG_OK;
}

int ulg_disc_regret(ulg_ctx *c, int arity, int64_t first, int64_t count, double *out) {
    if (!c || count < 0 || (count > 0 && !out)) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!disc_ready(c)) return set_err(c, ULG_ERR_STATE, "ulg_disc_regret: call ulg_disc_load first");
    if (arity < 1 || arity > 255 || std::find(c->disc_arity.begin(), c->disc_arity.end(), arity) == c->disc_arity.end())
        return set_err(c, ULG_ERR_ARG, "ulg_disc_regret: no loaded column has this arity");
    if (first < 0 || first > c->N || count > c->N + 1 - first)
        return set_err(c, ULG_ERR_ARG, "ulg_disc_regret: the range leaves 0 .. N");
    ULG_HIP(c, hipSetDevice(c->device));
    if (int rc = fnml_ensure_table(c, "ulg_disc_regret")) return rc;
    if (count == 0) return ULG_OK;
    if (arity == 1) {  // ln C(1, n) = 0: no row
        std::fill(out, out + count, 0.0);
        return ULG_OK;
    }
    const FnmlReduce red = fnml_reduce(c);
    std::vector<long long> fixed((size_t)count);
    ULG_HIP(c, hipMemcpyAsync(fixed.data(), red.table + (int64_t)red.rows.of[arity] * red.stride + first,
                              (size_t)count * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (int64_t i = 0; i < count; ++i) out[i] = fnml_unfix(fixed[(size_t)i], red.shift);
    return ULG_OK;
}

int ulg_disc_counts(ulg_ctx *c, int var, uint64_t parents, int32_t *counts, int64_t cap, int64_t *ncells) {
    if (!c || !counts || !ncells) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!disc_ready(c)) return set_err(c, ULG_ERR_STATE, "ulg_disc_counts: call ulg_disc_load first");
    if (var < 0 || var >= c->n || (parents >> c->n)) return set_err(c, ULG_ERR_ARG, "ulg_disc_counts: bad variable or parents");
    const uint64_t P = parents & ~(1ull << var);
    const uint64_t cells = table_cells(c, var, P);
    if (cells >> 63) return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_disc_counts: a contingency table of 2^63 cells or more");
    *ncells = (int64_t)cells;
    if (cap < (int64_t)cells) return set_err(c, ULG_ERR_ARG, "ulg_disc_counts: cap is below q * r_v");
    if (cells > (1ull << 28)) return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_disc_counts: more than 2^28 cells");
    ULG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->d_disc_counts, (size_t)cells))) return rc;
    ULG_HIP(c, hipMemsetAsync(c->d_disc_counts.p, 0, (size_t)cells * 4, c->stream));
    if ((rc = disc_sets_launch(c, "ulg_disc_counts", ULG_SCORE_BIC, 1, &var, &P, nullptr, c->d_disc_counts.p))) return rc;
    ULG_HIP(c, hipMemcpy(counts, c->d_disc_counts.p, (size_t)cells * 4, hipMemcpyDeviceToHost));
    return ULG_OK;
}

}  // extern "C"
