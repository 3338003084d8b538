// cbic.hip -- continuous-BIC parent-set scoring on MI355X (gfx950).
//
// Reference path (ninalu/urlearning-cpp, urlearning/):
//   BIC_OLS_Function ctor          scoring_function/BIC_OLS.cpp:30-123
//   calculateScoreAndBeta          BIC_OLS.cpp:277-389 (mlpack OLS, no intercept)
//   calculateScore                 BIC_OLS.cpp:174-276 (store / prune rule)
//   find_best_subset_score         BIC_OLS.cpp:125-172 (dominance recursion)
//   calculateScores_internal       score_calculator.cpp:54-135 (layers, Gosper)
//
// Design (MI355X-first):
//   * the data is normalised once and the FP64 Gram matrix G = Z'Z is built
//     with v_mfma_f64_16x16x4_f64 (the only dense contraction on the path);
//   * every parent set is then one lane: gather G[P,P], G[P,v] from LDS,
//     k x k Cholesky in registers, RSS = G[v,v] - |L^-1 b|^2;
//   * the dominance recursion (whose result depends on the reference's
//     zero-padded parent vector and XOR-toggle) is replayed
//     exactly on per-lane bitsets over subsets of P u {variable 0};
//   * a layer is two launches -- sets that contain variable 0, then the rest
//      -- which reproduces the sequential Gosper order;
//   * every (variable, layer) owns a dense float slab indexed by the colex
//     rank of the set inside the variable's candidate list (= the Gosper
//     enumeration index), holding the stored score or an absent sentinel.
#include <cstdio>
#include <atomic>
#include <thread>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "search_internal.h"
#include "host_walk.h"
#include "cbic_dev.h"

using namespace ulg;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kGramRows = 1024;  // rows of Z per Gram wave (split-K chunk)


// ------------------------------------------------------------------------
// Normalisation (BIC_OLS.cpp:66-97): x - mean, divided by the sample std
// (N-1) of the centred column.  Deterministic tree reductions.
// ------------------------------------------------------------------------
__device__ double block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kBlock) colstats_kernel(const double *raw, int64_t N, double *stat) {
    __shared__ double red[kBlock];
    const double *x = raw + (int64_t)blockIdx.x * N;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += kBlock) s += x[i];
    const double mean = block_sum(s, red) / (double)N;
    // arma::var(x - mean): two-pass with the compensation term
    double s2 = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += kBlock) s2 += x[i] - mean;
    const double m2 = block_sum(s2, red) / (double)N;
    double a2 = 0.0, a3 = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += kBlock) {
        const double t = m2 - (x[i] - mean);
        a2 += t * t;
        a3 += t;
    }
    a2 = block_sum(a2, red);
    a3 = block_sum(a3, red);
    if (threadIdx.x == 0) {
        const double var = N > 1 ? (a2 - a3 * a3 / (double)N) / (double)(N - 1) : 0.0;
        stat[2 * blockIdx.x] = mean;
        stat[2 * blockIdx.x + 1] = sqrt(var);
    }
}

// Z row-major N x npad (padded columns zero): lanes of a wave read one row.
__global__ void __launch_bounds__(kBlock) normalise_kernel(const double *raw, int64_t N, int n, int npad,
                                                           const double *stat, double *z) {
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= N * npad) return;
    const int64_t r = idx / npad;
    const int c = (int)(idx % npad);
    double v = 0.0;
    if (c < n) v = (raw[(int64_t)c * N + r] - stat[2 * c]) / stat[2 * c + 1];
    z[idx] = v;
}

// G = Z'Z on v_mfma_f64_16x16x4_f64.  One wave per (16x16 tile, row chunk).
// A[i][k] = Z[r0+k][I0+i], B[k][j] = Z[r0+k][J0+j]; lane l holds
// i = j = l & 15, k = l >> 4.  D: col = l & 15, row = (l >> 4) + 4 * reg.
__global__ void __launch_bounds__(64) gram_mfma_kernel(const double *z, int64_t N, int npad, int tiles,
                                                       double *partials) {
    const int chunk = blockIdx.x;
    const int tile = blockIdx.y;
    const int I0 = (tile / tiles) * 16, J0 = (tile % tiles) * 16;
    const int lane = threadIdx.x;
    const int i = lane & 15, k = lane >> 4;
    const int64_t rb = (int64_t)chunk * kGramRows;
    const int64_t re = rb + kGramRows < N ? rb + kGramRows : N;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r0 = rb; r0 < re; r0 += 4) {
        const int64_t r = r0 + k;
        double a = 0.0, b = 0.0;
        if (r < re) {
            a = z[r * npad + I0 + i];
            b = z[r * npad + J0 + i];
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    double *out = partials + ((int64_t)chunk * tiles * tiles + tile) * 256;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = (lane >> 4) + 4 * reg;
        out[row * 16 + (lane & 15)] = acc[reg];
    }
}

__global__ void __launch_bounds__(kBlock) gram_reduce_kernel(const double *partials, int chunks, int tiles, int n,
                                                             double *gram) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n * n) return;
    const int r = idx / n, c = idx % n;
    const int tile = (r / 16) * tiles + (c / 16);
    const int e = (r % 16) * 16 + (c % 16);
    double s = 0.0;
    for (int ch = 0; ch < chunks; ++ch) s += partials[((int64_t)ch * tiles * tiles + tile) * 256 + e];
    gram[idx] = s;
}


struct ScoreArgs {
    const double *gram;      // n x n row-major
    const uint32_t *binom;   // [64][kBinomK]
    const uint8_t *cand;     // [nv][64] compact index -> variable
    const int *meta;         // [nv][4]: variable, m, var0in, -
    const uint64_t *tbl_off; // [nv*S + 1] start of (vi, layer) slab
    const uint64_t *work;    // [nv + 1] prefix of this launch's sets
    uint64_t total;          // work[nv], for the layer kernels' scalar search (wave_variable)
    float *table;
    float *hsub;                // variant bit 6: per slot, the maximum stored value over the set's
                                // nonempty subsets (the set included; NaN = none), table layout
    uint64_t *queue;            // variant bit 4: lanes left for the walk launch
    unsigned long long *qcount;
    unsigned long long *err;    // the call's error word (kErrQueue: a walk-queue segment overflowed)
    uint8_t *qkey;              // bucketed walk launches: per queue entry, its walk key
    double N;
    double pen;                 // lambda ln(N), the device's product (ulg_ctx::pen, penalty_kernel)
    int n, nv, S;
    int xcd;                    // remap blocks so each XCD takes a contiguous run of sets
    int hsub_out;               // write the subset maxima (0: the top layer's phase 1, never read)
    // Unrank tables (option score_unrank_lut; CbicPlan::build_luts): lut[off + r]
    // = unrank_colex(r, l, U) as 32 bits, for the (U, l) this launch unranks
    // variable vi's sets with; lut_off[vi] = its offset, -1 = none (the lane
    // computes).  Both null: no table in this launch.
    const uint32_t *lut;
    const int32_t *lut_off;     // [nv], this launch's (layer, phase)
    // The launch image (option score_lds_image; CbicPlan::build_images): the
    // bytes of LDS [0, lay.stack) as 16-byte pieces, image16 of them.  Null:
    // the layer kernels fill LDS from the arrays above.
    const uint4 *image;
    int image16;
};

// Blocks are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8),
// and each XCD has its own L2.  With xcd set, XCD x takes the x-th contiguous
// eighth of the launch's blocks -- the sets of a few variables, whose slabs
// then stay in that XCD's L2 -- through a bijection of [0, nb).
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb, int on) {
    if (!on) return b;
    const uint32_t x = b & 7u, k = b >> 3, q = nb >> 3, r = nb & 7u;
    return x * q + (x < r ? x : r) + k;
}

// Parent-set constraints (scoring::Constraints, constraints.h:123-139) as the
// kernels read them: words [0, nv] are the prefix of the variables'
// alternatives, then one (required, forbidden) pair of masks per alternative.
// A scoring call's table is indexed by the call's variable index and holds
// compact candidate masks (the lanes' cm); ulg_cbic_score_sets' table is
// indexed by variable and holds variable masks.  A set satisfies a variable
// without alternatives, or one alternative with required within the set and
// forbidden disjoint from it; a variable whose alternatives all require a
// non-candidate carries one alternative requiring bit 63, which no set holds.
// Only the constrained kernels read it (*_cons_kernel: the texts of
// cbic_score_{layer,small,wide,sets}.inc included a second time with
// ULG_CONS 1, so the unconstrained kernels stay the code they were); tables
// of at most kConsLdsWords words (score_plan.h) are copied into LDS behind
// the block's layout.
__host__ __device__ inline bool cons_violates(const uint64_t *ct, int nv, int vi, uint64_t set) {
    const uint64_t b = ct[vi], e = ct[vi + 1];
    if (b == e) return false;
    const uint64_t *p = ct + nv + 1 + 2 * b;
    for (uint64_t i = 0; i < e - b; ++i)
        if ((p[2 * i] & ~set) == 0 && (p[2 * i + 1] & set) == 0) return false;
    return true;
}
// the block's copy of the call's table (CONS kernels; before the first barrier)
template <int THREADS>
__device__ __forceinline__ const uint64_t *cons_stage(unsigned char *smem, int lds_end, const uint64_t *cons,
                                                      int cons_words) {
    if (cons_words > kConsLdsWords) return cons;
    uint64_t *sc = reinterpret_cast<uint64_t *>(smem + ((lds_end + 15) & ~15));
    for (int i = threadIdx.x; i < cons_words; i += THREADS) sc[i] = cons[i];
    return sc;
}


// The blocks' LDS carve (LdsLayout, lds_layout): score_plan.h.

// The walk queue's segments and their counters (kSegBlocks, kSegEntries,
// kSegStride, kBucketHdrWords, seg_count): score_plan.h.
// Bits of the call's error word (d_qcount[nqc - 1], zeroed by the prologue,
// copied beside the stored count by scan_kernel): a wide walk over its cap;
// a queue position past its segment (nothing is written there); a walk entry
// whose table slot lies past the call's slots (its decision is not written).
constexpr unsigned long long kErrWide = 1ull, kErrQueue = 2ull, kErrSlot = 4ull;
__device__ __forceinline__ uint64_t walk_segment() { return blockIdx.x % seg_count(gridDim.x); }

// Append a set to the walk queue (wave-aggregated: one atomic per wave on the
// segment's counter): table slot | ts bits << 32, the hi words, then the open
// words (open = absent & cover(T without var 0) & not checked; checked =
// {empty}).  queue / qcount: the segment's entries and counter.
// The walk key of a queued set (walk_bucket): which of the walk's first-level
// nodes (P minus one member, the top call's tests) it may expand, one bit per
// member -- sets with the same key start the same union walk, so a launch
// sorted by key walks ~3x fewer union points (scripts/walk_sched_study.cpp).
// When every first-level node is open (the longest, least alike walks), the
// key is 64 + the open bits of six second-level nodes (P minus two members,
// the first six pairs in order): those sets then split further (C3 layer 6
// with variable 0: the longest wave 432 -> 294 union points).
template <int L, int PHASE, int W>
__device__ __forceinline__ uint32_t walk_key(const uint64_t (&ow)[W]) {
    constexpr uint32_t root = PHASE == 0 ? ((1u << L) - 1u) : (((1u << L) - 1u) << 1);
    constexpr int off = PHASE == 0 ? 0 : 1;
    uint32_t key = 0;
#pragma unroll
    for (int a = 0; a < L; ++a) {
        const uint32_t t = root ^ (1u << (a + off));
        key |= (uint32_t)((ow[t >> 6] >> (t & 63u)) & 1ull) << a;
    }
    if (key == (1u << L) - 1u) {
        uint32_t sec = 0;
        int nb = 0;
#pragma unroll
        for (int a = 0; a < L; ++a)
#pragma unroll
            for (int b = a + 1; b < L; ++b) {
                if (nb < 6) {
                    const uint32_t t = root ^ (1u << (a + off)) ^ (1u << (b + off));
                    sec |= (uint32_t)((ow[t >> 6] >> (t & 63u)) & 1ull) << nb;
                }
                ++nb;
            }
        key = 64u + sec;
    }
    return key;
}

// MBCNT (the narrow layer kernels): the lane's place among the active lanes
// from the hardware's masked bit count, the same number as the popcount of
// the active lanes below it, without the lane index held in a register from
// the top of the kernel (it was spilled there).
template <int L, int PHASE, class BS, bool MBCNT = false>
__device__ __forceinline__ void queue_walk(const BS &present, const BS &hi, uint64_t *queue,
                                           unsigned long long *qcount, unsigned long long *err, uint64_t slot,
                                           float ts, uint8_t *qkey = nullptr) {
    constexpr int W = BS::kWords;
    const unsigned long long act = __ballot(1);
    const int leader = __ffsll((long long)act) - 1;
    unsigned long long base = 0;
    uint32_t below;  // active lanes below this one
    if constexpr (MBCNT) {
        below = __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
        if (below == 0u) base = atomicAdd(qcount, (unsigned long long)__popcll(act));
    } else {
        const int lane = threadIdx.x & 63;
        if (lane == leader) base = atomicAdd(qcount, (unsigned long long)__popcll(act));
        below = (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
    }
    base = __shfl(base, leader);
    const uint64_t pos = base + (uint64_t)below;
    // a segment holds at most kSegBlocks blocks' lanes by construction
    // (seg_count); a sizing mistake becomes an error status, not a stray write
    if (pos >= kSegEntries) {
        if (err) atomicOr(err, kErrQueue);
        return;
    }
    uint64_t ow[W];
#pragma unroll
    for (int wj = 0; wj < W; ++wj) ow[wj] = hi.word(wj);
    cover_words<W>(ow);
#pragma unroll
    for (int wj = 0; wj < W; ++wj) {
        const uint64_t ce = ow[wj] & 0x5555555555555555ull;
        ow[wj] = (ce | (ce << 1)) & ~present.word(wj) & (wj == 0 ? ~1ull : ~0ull);
    }
    if constexpr (W < 4)
        if (qkey) qkey[pos] = (uint8_t)walk_key<L, PHASE, W>(ow);
    uint64_t *e = queue + pos * (uint64_t)(1 + 2 * W);
    e[0] = slot | ((uint64_t)fbits(ts) << 32);
#pragma unroll
    for (int wj = 0; wj < W; ++wj) e[1 + wj] = hi.word(wj);
#pragma unroll
    for (int wj = 0; wj < W; ++wj) e[1 + W + wj] = ow[wj];
}



#ifdef ULG_GATHER_STATS
// Diagnostic build only (scripts/gather_stats.py): per (layer, phase) counts of
// what the presence gathers of the compacted sets find.
__device__ unsigned long long g_gstats[2 * (kMaxL + 1) * 16];

// Compile-time masks over the local subsets t of a layer-L set: the keys the
// full gather reads, the keys without child i's removed member (child i =
// P minus its i-th member in compact order), the keys holding variable 0.
template <int L, int PHASE>
struct KeyMasks {
    static constexpr int Q = PHASE == 0 ? L : L + 1;
    static constexpr int W = bits_words(L);
    uint64_t key[W], miss[L][W], v0[W];
    constexpr KeyMasks() : key{}, miss{}, v0{} {
        constexpr PresList<L, PHASE, Q, 0> PL{};
        for (int i = 0; i < PL.n; ++i) key[PL.t[i] >> 6] |= 1ull << (PL.t[i] & 63);
        for (uint32_t t = 0; t < (1u << Q); ++t) {
            if (t & 1u) v0[t >> 6] |= 1ull << (t & 63);
            for (int i = 0; i < L; ++i) {
                const int b = PHASE == 1 ? i + 1 : i;
                if (!((t >> b) & 1u)) miss[i][t >> 6] |= 1ull << (t & 63);
            }
        }
    }
};

template <int L, int PHASE, class BS>
__device__ void gather_stats(const BS &present, const BS &hi, uint32_t hotA, uint32_t hotZ, bool z, bool queued) {
    constexpr int W = BS::kWords;
    constexpr KeyMasks<L, PHASE> KM{};
    uint64_t cov[W];
#pragma unroll
    for (int j = 0; j < W; ++j) cov[j] = hi.word(j);
    cover_words<W>(cov);
    unsigned long long c[16] = {};
    c[0] = 1;
    c[1] = __builtin_popcount(hotA);
    c[2] = __builtin_popcount(hotZ);
    const uint32_t sel = (PHASE == 1 && z) ? hotZ : hotA;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        uint64_t need = 0, hrel = 0;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            if ((sel >> i) & 1u) need |= KM.miss[i][j];
            if ((hotA >> i) & 1u) hrel |= KM.miss[i][j] & ~KM.v0[j];
            if (PHASE == 1 && z && ((hotZ >> i) & 1u)) hrel |= KM.miss[i][j] & KM.v0[j];
        }
        need &= KM.key[j];
        hrel &= KM.key[j];
        const uint64_t pr = present.word(j) & KM.key[j], hw = hi.word(j) & KM.key[j], cv = cov[j] & KM.key[j];
        c[3] += __builtin_popcountll(pr);
        c[4] += __builtin_popcountll(hw);
        c[5] += __builtin_popcountll(need);
        c[6] += __builtin_popcountll(hrel);
        c[7] += __builtin_popcountll(cv);
        c[8] += __builtin_popcountll(pr & need);
        c[9] += __builtin_popcountll(hw & ~hrel);
        c[10] += __builtin_popcountll(cv & ~need);
        c[11] += __builtin_popcountll(KM.key[j]);
        c[13] += __builtin_popcountll((hrel | cv) & KM.key[j]);
        c[14] += __builtin_popcountll(pr & ~need);
    }
    c[12] = queued;
    unsigned long long *g = g_gstats + (L * 2 + PHASE) * 16;
#pragma unroll
    for (int i = 0; i < 15; ++i) atomicAdd(g + i, c[i]);
}
#endif

// Set r of variable vi's (layer L, phase) launch: its compact mask over the
// candidate list, colex rank, and parent variables in ascending order (==
// BIC_OLS parent_vec order).  smeta / scand / binom: the LDS copies.
// M: uint64_t, or uint32_t in the narrow form of the layer kernels
template <int L, class M = uint64_t>
struct SetHead {
    int v;
    bool z;
    M cm, rankP;
    int gv[L];
};
// out[r] = unrank_colex(r, l, U) for r < count = C(U, l): a context's unrank
// table (score_plan.h LutCache), equal to the computed mapping by construction.
__global__ void __launch_bounds__(kBlock) unrank_lut_fill_kernel(uint32_t *out, uint32_t count, int l, int U,
                                                                 const uint32_t *binom) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r < count) out[r] = (uint32_t)unrank_colex(r, l, U, binom);
}

// *out = lambda ln(N) with the device's logarithm and one rounded product:
// the value every lane used to compute inside the score's last expression.
__global__ void penalty_kernel(double N, double lambda, double *out) { *out = lambda * log(N); }

// The variable of a whole wave of a layer launch, found on the scalar unit
// before the block fills its LDS: the wave's first and last set (lane 0's gid
// and 63 further, clamped to the launch's last set like the lanes' own) are
// wave-uniform, so the search of the launch's prefixes runs in SGPRs on scalar
// loads of a.work.  vi >= 0: every lane's set belongs to variable vi, whose
// sets start at `base`; -1: the wave straddles a boundary and each lane
// searches the LDS copy as before.  With vi known this early the lane's read
// of the unrank table is in flight while the block fills its LDS, instead of a
// dependent round trip behind the barrier.
struct WaveVar {
    int vi;
    int32_t loff;  // the variable's unrank table in this launch, -1 = none
    uint64_t base, total;
};
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
    return (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)x) |
           ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(x >> 32)) << 32);
}
// total = work[nv], the launch's sets (ScoreArgs::total): every scalar load
// here is a dependent round trip at the start of the wave, so the search keeps
// the prefixes it has read -- work[0] = 0 and work[nv] = total bound it, and
// when it ends the last two probes are work[lo] and work[lo + 1].
// The same for the variable's unrank-table offset (lut_off, may be null): each
// probe reads it beside the prefix, in the same round trip, so loff is
// lut_off[lo] when the search ends.
__device__ __forceinline__ WaveVar wave_variable(const uint64_t *work, const int32_t *lut_off, int nv, uint64_t total,
                                                 uint64_t gid_lane0) {
    WaveVar w;
    w.total = total;
    const uint64_t first = uniform64(gid_lane0), last = total - 1;
    const uint64_t gl = first < last ? first : last, gh = first + 63 < last ? first + 63 : last;
    int lo = 0, hi = nv;
    uint64_t wlo = 0, whi = total;
    int32_t llo = lut_off ? lut_off[0] : -1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const uint64_t wm = work[mid];
        const int32_t lm = lut_off ? lut_off[mid] : -1;
        if (wm <= gl) {
            lo = mid;
            wlo = wm;
            llo = lm;
        } else {
            hi = mid;
            whi = wm;
        }
    }
    w.base = wlo;
    w.vi = gh < whi ? lo : -1;
    w.loff = llo;
    return w;
}

// have_um: um is the set's unranked mask read from the launch's unrank table
// (UnrankPick below); otherwise the lane computes it.  RANK false: the caller
// takes the set's rank from child_ranks and rankP stays 0.
// M = uint32_t (narrow launches: m <= 32): the shift by one for variable 0
// moves a mask over U = m - 1 <= 31 candidates, so bit 31 is the last one used.
template <int L, int PHASE, bool RANK = true, class M = uint64_t>
__device__ __forceinline__ SetHead<L, M> set_head(const int *smeta, const uint8_t *scand, const uint32_t *binom, int vi,
                                                  M r, bool have_um = false, uint32_t um32 = 0u) {
    SetHead<L, M> h;
    h.v = smeta[vi * 4 + 0];
    const int m = smeta[vi * 4 + 1];
    h.z = smeta[vi * 4 + 2] != 0;
    M um = um32;
    if (!have_um) um = unrank_colex<M>(r, (PHASE == 0) ? L - 1 : L, (PHASE == 0 || h.z) ? m - 1 : m, binom);
    if (PHASE == 0) h.cm = (um << 1) | (M)1;
    else if (h.z) h.cm = um << 1;
    else h.cm = um;
    h.rankP = RANK ? rank_colex(h.cm, binom) : (M)0;
    const uint8_t *cl = scand + vi * 64;
    int el[L];
    mask_elements<L>(h.cm, el);
#pragma unroll
    for (int i = 0; i < L; ++i) h.gv[i] = cl[el[i]];
    return h;
}

// The one-pass form of one set (variant bit 4 clear): presence gathers, the
// walk in registers (or LDS bitsets from 4 words), the store rule, and under
// bit 6 the subset maxima.  Shared by score_layer_kernel and the fused small
// layers (score_small_kernel).
template <int L, int PHASE, int V>
__device__ __forceinline__ void one_pass_set(const ScoreArgs &a, unsigned char *smem, const LdsLayout &lay,
                                             const uint32_t *binom, const uint64_t *toff, int vi, bool z, uint64_t cm,
                                             uint64_t rankP, float ts) {
    constexpr bool HM = (V & 64) != 0;
    // the children's subset maxima (bit 6), loaded before the gathers so both
    // share one memory round trip
    float hch = absent_f();
    if constexpr (HM && L > 1) {
        const uint64_t vbase = (uint64_t)vi * a.S;
        uint64_t rc[L], rz[L];
        child_ranks<L, false>(cm, binom, rc, rz);
        float ch[L];
#pragma unroll
        for (int i = 0; i < L; ++i) ch[i] = a.hsub[toff[vbase + L - 1] + rc[i]];
#pragma unroll
        for (int i = 0; i < L; ++i) hch = fmaxf(hch, ch[i]);
    }
    // small layers (one bitset word, unrolled gathers): the gathered values
    // stay in registers, so the walk's best needs no second round trip
    constexpr int QV = PHASE == 0 ? L : L + 1;
    constexpr bool KEEPV = bits_words(L) == 1 && (V & 1) && !(V & 16) && QV <= 5;
    float out;
    bool queued = false;  // variant bit 4: left for the walk launch
    if (ts >= 0.0f) {
        // returned -ts; the caller stores it iff it is < 0 (score_calculator.cpp:111)
        const float s = -ts;
        out = (s < 0.0f) ? s : absent_f();
    } else {
        constexpr int W = bits_words(L);
        using BS = std::conditional_t<(W >= 4), BitsLds<W>, Bits<W>>;
        uint64_t *lds_bits = reinterpret_cast<uint64_t *>(smem + lay.bits) + threadIdx.x;
        const LocalSet<L> ls = local_set<L, PHASE>(cm, z);
        const uint64_t cpack = ls.cpack;
        const uint32_t Plocal = ls.Plocal;
        const uint32_t pvtop = ls.pvtop;
        const uint64_t vbase = (uint64_t)vi * a.S;

        // presence of every candidate key in the cache as it stands now
        // the first LDS bitset is `present`; `hi` and `checked` share the
        // second (only the decision-only walk uses `hi`); `visited` the third
        BS present = make_bits<BS>(lds_bits);
        BS hi = make_bits<BS>(lds_bits + (size_t)W * kBlock);
        present.clear();
        if constexpr ((V & 16) != 0) hi.clear();
        const float thr = -ts;
        float vals[KEEPV ? (1 << QV) : 1];
        if constexpr (KEEPV) {
#pragma unroll
            for (int t = 0; t < (1 << QV); ++t) vals[t] = 0.0f;
            presence_unrolled<L, PHASE, QV, W, LdPlain, 8, (V != 1), 0>(present, hi, thr, binom, ls.cpack, z, a.table,
                                                                        toff + vbase, vals);
        } else {
            gather_keys<L, PHASE, V>(present, hi, ls, thr, binom, z, a.table, toff + vbase);
        }

        if constexpr ((V & 16) != 0) {
            // decide what needs no walk; queue the rest for the walk kernel
            const bool dom = settle_rules<L, PHASE>(present, hi, ls, queued);
            if (queued) {
                const uint64_t seg = walk_segment();
                constexpr int QW = bits_words(L);
                queue_walk<L, PHASE>(present, hi, a.queue + seg * kSegEntries * (uint64_t)(1 + 2 * QW),
                                     a.qcount + seg * kSegStride, a.err, toff[vbase + L] + rankP, ts);
            }
            out = dom ? absent_f() : -ts;
        } else {
        BS checked = make_bits<BS>(lds_bits + (size_t)W * kBlock);
        BS visited = make_bits<BS>(lds_bits + (size_t)2 * W * kBlock);
        checked.clear();
        visited.clear();
        checked.set(0u);  // checked.insert(empty_set)
        best_subset<L, BS>(Plocal, pvtop, present, checked, visited);

        float best = 0.0f;
        if constexpr (KEEPV) {
            // every visited node is a present key, gathered above
            const uint64_t x = visited.word(0);
#pragma unroll
            for (int t = 0; t < (1 << QV); ++t)
                if (((x >> t) & 1ull) && vals[t] > best) best = vals[t];
        } else {
#pragma unroll
        for (int wj = 0; wj < W; ++wj) {
            uint64_t x = visited.word(wj);
            while (x) {
                const uint32_t t = (uint32_t)(wj * 64 + __builtin_ctzll(x));
                x &= x - 1;
                uint64_t rk = 0;
                uint32_t rem = t;
                int j = 0;
                while (rem) {
                    const int lb = __builtin_ctz(rem);
                    rem &= rem - 1;
                    ++j;
                    rk += B(binom, (int)((cpack >> (6 * lb)) & 63ull), j);
                }
                const float val = a.table[toff[vbase + __builtin_popcount(t)] + rk];
                if (val > best) best = val;
            }
        }
        }
        // BIC_OLS.cpp:234: best_subset_score + bic_threshold >= -the_score
        out = ((double)best + 0.0 >= (double)(-ts)) ? absent_f() : -ts;
        }
    }
    if (!queued) a.table[toff[(uint64_t)vi * a.S + L] + rankP] = out;
    // the one-pass form keeps the subset maxima for the layers above it
    if constexpr (HM)
        if (a.hsub_out) a.hsub[toff[(uint64_t)vi * a.S + L] + rankP] = fmaxf(out, hch);
}

// The rest of a queued set's gathers (the keys the rules did not read), then
// either the walk queue or, when the walk closure shows the walk cannot reach
// a key >= -ts, the store it would make.  toffv: this variable's slab offsets.
// (TO, M: the offsets' and the slot's 64-bit or narrow types, cbic_dev.h)
template <int L, int PHASE, int V, class BS, class TO, class M>
__device__ __forceinline__ void walk_or_store(const ScoreArgs &a, BS &present, BS &hib, const LocalSet<L> &ls,
                                              float tk, const uint32_t *binom, bool zk, TO toffv, uint64_t seg, M sk,
                                              float hch) {
    constexpr int W = BS::kWords;
#ifndef ULG_PROBE_NOPART2
    gather_keys<L, PHASE, V, BS, LdPlain, 2, TO>(present, hib, ls, -tk, binom, zk, a.table, toffv);
#endif
    // no key >= -ts among the nodes the walk can test: it would store P
    // (80 % of the walked sets at C3's layer 6 end stored)
    bool may_hit = true;
    if constexpr (W < 4) {
        uint64_t pw[W], hw[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            pw[j] = present.word(j);
            hw[j] = hib.word(j);
        }
        may_hit = walk_may_hit<L, PHASE, W>(pw, hw);
    }
    if (may_hit) {
#ifndef ULG_PROBE_NOQUEUE
        queue_walk<L, PHASE, BS, sizeof(M) == 4>(present, hib, a.queue + seg * kSegEntries * (uint64_t)(1 + 2 * W),
                                                 a.qcount + seg * kSegStride, a.err, sk, tk,
                             a.qkey ? a.qkey + seg * kSegEntries : nullptr);
#endif
        if (a.hsub_out) *slot_ptr(a.hsub, sk) = hch;  // the walk raises it to -ts if it stores P
    } else {
        *slot_ptr(a.table, sk) = -tk;
        if (a.hsub_out) *slot_ptr(a.hsub, sk) = fmaxf(-tk, hch);
    }
}

// Minimum waves per SIMD for the register allocator (the second argument of
// __launch_bounds__): the layer-6 two-pass launch without variable 0, the
// largest, at 7 (72 VGPRs; 82 had left 5 waves per SIMD): C3 188 -> 175 us,
// C5 1,405 -> 1,293 us (6: 178 / 1,302 us).  8 for every kernel (64 VGPRs)
// spilled more and slowed the phase-0 launch 210 -> 269 us.  The phase-0
// launch at 7 (72 VGPRs): 215 -> 208 us at C5; the layer-4 one-pass kernels
// at 8 (60 VGPRs, no spills): C5 81 -> 79 us.  The others keep their
// allocation.
#ifndef ULG_L6_REST_WAVES
#define ULG_L6_REST_WAVES 7
#endif
#ifndef ULG_L6_VAR0_WAVES
#define ULG_L6_VAR0_WAVES 7
#endif
#ifndef ULG_L4_WAVES
#define ULG_L4_WAVES 8
#endif
template <int L, int PHASE, int V>
constexpr int score_min_waves() {
    return (L == 6 && (V & 16) != 0) ? (PHASE == 1 ? ULG_L6_REST_WAVES : ULG_L6_VAR0_WAVES)
                                     : (L == 4 ? ULG_L4_WAVES : 1);
}
// PHASE 0: sets containing variable 0; 1: the rest.  V = variant bits (see
// ulg_set_option "score_variant"), compile-time so each form gets its own
// register allocation.
#define ULG_CONS 0
#include "cbic_score_layer.inc"
#undef ULG_CONS
#define ULG_CONS 1
#include "cbic_score_layer.inc"
#undef ULG_CONS

// Layers 1..LF of every variable in ONE launch (option score_fused; the
// small layers' one-pass form, V = variant & 65).  Workgroup b takes variable
// b and runs (L, phase) in order, its kFusedThreads lanes taking the phase's
// sets kFusedThreads at a time, with a barrier between phases: a phase reads
// only its own variable's lower layers and, in phase 1, the same layer's
// var-0 sets, all written by this workgroup before the barrier
// (its waves share one CU, so the workgroup-scope fences of __syncthreads
// order the stores before the loads).  Replaces 2 LF dependent launches of
// a few waves each (layers 1-4 at C3: ~117 us whatever the variable count).
constexpr int kFusedThreads = 1024;
#define ULG_CONS 0
#include "cbic_score_small.inc"
#undef ULG_CONS
#define ULG_CONS 1
#include "cbic_score_small.inc"
#undef ULG_CONS

// Second half of a queued layer (variant bit 4): one wave (64 threads) per
// 64*K queued sets.  Entry: table slot (low 32 bits) | ts bits (high 32), W
// `hi` words, W open words (queue_walk).  walk_load gathers this lane's K
// entries into the bit-sliced hi / open vectors (register r, field f <-
// subset r*E + f, bit k of a field <- set k) and returns the alive mask.
template <int L, int K>
__device__ __forceinline__ uint32_t walk_load(const uint64_t *queue, uint64_t qn, uint64_t mine,
                                              typename Sliced<L, K>::Vec &hiV, typename Sliced<L, K>::Vec &openV) {
    using S = Sliced<L, K>;
    constexpr int W = bits_words(L);
#pragma unroll
    for (int r = 0; r < S::NV; ++r) {
        hiV[r] = 0u;
        openV[r] = 0u;
    }
    uint32_t alive = 0u;
#pragma nounroll
    for (int k = 0; k < S::K; ++k) {
        if (mine + k >= qn) break;
        alive |= 1u << k;
        const uint64_t *e = queue + (mine + k) * (uint64_t)(1 + 2 * W);
        uint64_t hw[W], ow[W];
#pragma unroll
        for (int wj = 0; wj < W; ++wj) {
            hw[wj] = e[1 + wj];
            ow[wj] = e[1 + W + wj];
        }
        // transpose: register r, field f <- subset r*E + f of set k
#pragma unroll
        for (int r = 0; r < S::NV0; ++r) {
            const int t0 = r * S::E;
            constexpr uint32_t EM = (uint32_t)((1ull << S::E) - 1ull);
            const uint32_t hb = (uint32_t)(hw[t0 >> 6] >> (t0 & 63)) & EM;
            const uint32_t ob = (uint32_t)(ow[t0 >> 6] >> (t0 & 63)) & EM;
            uint32_t hs, os;
            if constexpr (S::K == 8) {
                // 4 bits -> bytes 0..3 (non-overlapping partial products)
                hs = (hb * 0x00204081u) & 0x01010101u;
                os = (ob * 0x00204081u) & 0x01010101u;
            } else {
                hs = os = 0u;
#pragma unroll
                for (int f = 0; f < S::E; ++f) {
                    hs |= ((hb >> f) & 1u) << (S::K * f);
                    os |= ((ob >> f) & 1u) << (S::K * f);
                }
            }
            hiV[r] |= hs << k;
            openV[r] |= os << k;
        }
    }
    return alive;
}

// The decisions of this lane's sets: pruned (absent) or stored (-ts), and the
// subset maxima raised to -ts when stored (variant bit 6).
template <int K>
__device__ __forceinline__ void walk_store(const uint64_t *queue, uint64_t qn, uint64_t mine, int W, uint32_t dom,
                                           float *table, float *hsub, uint64_t nslots, unsigned long long *err) {
#pragma nounroll
    for (int k = 0; k < K; ++k) {
        if (mine + k >= qn) break;
        const uint64_t e0 = queue[(mine + k) * (uint64_t)(1 + 2 * W)];
        const float ts = __uint_as_float((uint32_t)(e0 >> 32));
        const bool d = (dom >> k) & 1u;
        if ((uint32_t)e0 >= nslots) {  // an entry no scoring lane wrote
            atomicOr(err, kErrSlot);
            continue;
        }
        table[(uint32_t)e0] = d ? absent_f() : -ts;
        if (hsub && !d) hsub[(uint32_t)e0] = fmaxf(hsub[(uint32_t)e0], -ts);
    }
}

// One wave per (queue segment, chunk of 64 * K entries), chunk-major:
// blockIdx.x = chunk * nseg + segment, so the few chunks that hold sets come
// first in dispatch order and the empty ones (a segment can hold up to
// kSegEntries sets) form the tail -- interleaved, the empty workgroups' own
// dispatch delayed the last busy waves (the layer-6 walk's span 220 -> 427 us).
template <int L, int PHASE, int K>
__global__ void __launch_bounds__(64) walk_sliced_kernel(const uint64_t *queue, const unsigned long long *qcount,
                                                         float *table, float *hsub, uint64_t *wclock, uint64_t nslots,
                                                         unsigned long long *err) {
    using S = Sliced<L, K>;
    const uint64_t t_start = wclock ? wall_clock64() : 0;
    constexpr int W = bits_words(L);
    constexpr uint32_t kChunks = (uint32_t)((kSegEntries + 64 * K - 1) / (64 * K));
    const uint32_t nseg = gridDim.x / kChunks;
    const uint32_t seg = blockIdx.x % nseg;
    const uint64_t qc = qcount[(uint64_t)seg * kSegStride];
    const uint64_t qn = qc < kSegEntries ? qc : kSegEntries;  // past it: kErrQueue is set
    const uint64_t first = (uint64_t)(blockIdx.x / nseg) * 64 * S::K;
    if (first >= qn) return;
    queue += (uint64_t)seg * kSegEntries * (uint64_t)(1 + 2 * W);
    const uint64_t mine = first + (uint64_t)threadIdx.x * S::K;
    typename S::Vec hiV, openV;
    uint32_t alive = walk_load<L, K>(queue, qn, mine, hiV, openV);
    constexpr bool v0inP = PHASE == 0;
    constexpr uint32_t Plocal = v0inP ? ((1u << L) - 1u) : (((1u << L) - 1u) << 1);
    uint32_t pvtop = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) pvtop |= (uint32_t)(i + (v0inP ? 0 : 1)) << (4 * i);
    uint32_t dom = 0u, pts = 0u;
    // the open bits in LDS (OpenLds): no vector copies per recursion level
    __shared__ uint32_t open_lds[2 * S::NV * 64];
    OpenLds<L, K> ol{open_lds + threadIdx.x};
#pragma unroll
    for (int r = 0; r < S::NV; ++r) {
        ol.base[r * 64] = openV[r];
        ol.base[r * 64 + S::NV * 64] = hiV[r];
    }
    if (wclock) walk_sliced<L, K, L, true, OpenLds<L, K>, PHASE>(Plocal, pvtop, alive, hiV, ol, alive, dom, pts);
    else walk_sliced<L, K, L, false, OpenLds<L, K>, PHASE>(Plocal, pvtop, alive, hiV, ol, alive, dom, pts);
#ifdef ULG_GATHER_STATS
    if (alive) atomicAdd(&g_wstats[(L * 2 + PHASE) * 16 + 15], (unsigned long long)__builtin_popcount(alive));
#endif
    if (wclock && threadIdx.x == 0) {
        // diagnostics (ULG_WALK_CLOCK): start, end, union points of this wave
        wclock[3 * blockIdx.x] = t_start;
        wclock[3 * blockIdx.x + 1] = wall_clock64();
        wclock[3 * blockIdx.x + 2] = pts;
    }
    walk_store<S::K>(queue, qn, mine, W, dom, table, hsub, nslots, err);
}

// ---- bucketed walk launches (round 6, option walk_bucket) --------------------
// A layer-5/6 launch's queued sets walked in the order of their walk key
// (walk_key): a counting sort over (key, segment) -- the scoring kernel
// writes each set's key, walk_bucket_count_kernel ranks the sets of each
// segment by key and, in its last block, lays out the keys and a table of walk
// waves, walk_bucket_scatter_kernel writes each set's queue index at its place -- and
// walk_bucket_kernel walks the table.  The sets whose every first-level node
// is open hold the longest, least alike walks: split 64 ways by six
// second-level nodes (keys 64..127), they come first in the table, 64 sets per
// wave (one per lane); every other key 64 x K per wave.  At C3's layer 6
// without variable 0 the longest wave's union walk drops from 811 to ~465
// points and the launch's union points from 311 K to ~100 K
// (scripts/walk_sched_study.cpp on the dumped queues).  Same walks, same
// decisions: only which sets share a wave changes.  kBucketMax keys
// (score_plan.h): 64 first-level patterns, the all-open one split 64 ways.


// One block per kBucketSegs segments: the segments' key histogram in LDS
// (16 keys per 16-byte load), each entry's rank among the block's sets of its
// key (qaux = key << 24 | rank), and one global atomic per key for the
// block's base within the key (kbase; few blocks, so few atomics per address
// -- one block per segment serialised ~300-2300 atomics on each key's total).
// The key totals then give every key's sorted start and the list of walk
// waves (bucket_lanes), recomputed by each later kernel instead of a table.
#ifndef ULG_BUCKET_SEGS
#define ULG_BUCKET_SEGS 8
#endif
constexpr int kBucketSegs = ULG_BUCKET_SEGS;
__global__ void __launch_bounds__(256) walk_bucket_count_kernel(const unsigned long long *qseg, uint32_t nseg,
                                                                int L, const uint8_t *qkey, uint32_t *qaux,
                                                                uint32_t *kbase) {
    __shared__ unsigned int lh[kBucketMax];
    __shared__ unsigned int cst[kBucketSegs + 1];
    __shared__ unsigned int qnl[kBucketSegs];
    const uint32_t seg0 = blockIdx.x * kBucketSegs;
    const uint32_t nsb = nseg - seg0 < (uint32_t)kBucketSegs ? nseg - seg0 : (uint32_t)kBucketSegs;
    unsigned int *hdr = reinterpret_cast<unsigned int *>(const_cast<unsigned long long *>(qseg) + (uint64_t)nseg * kSegStride);
    if (threadIdx.x < kBucketMax) lh[threadIdx.x] = 0u;
    if (threadIdx.x < 64) {
        // the block's segments: their set counts and 16-entry chunk offsets
        const int lane = threadIdx.x;
        unsigned int qn = 0;
        if ((uint32_t)lane < nsb) {
            const uint64_t qc = qseg[(uint64_t)(seg0 + lane) * kSegStride];
            qn = (unsigned int)(qc < kSegEntries ? qc : kSegEntries);
            qnl[lane] = qn;
        }
        const unsigned int ch = (qn + 15u) >> 4;
        unsigned int incl = ch;
#pragma unroll
        for (int o = 1; o < kBucketSegs; o <<= 1) {
            const unsigned int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane < kBucketSegs) cst[lane + 1] = incl;
        if (lane == 0) cst[0] = 0u;
    }
    __syncthreads();
    const unsigned int items = cst[nsb];
    for (unsigned int it = threadIdx.x; it < items; it += 256) {
        uint32_t s = 0;
        while (s + 1 < nsb && cst[s + 1] <= it) ++s;
        const uint32_t c = it - cst[s];
        const uint64_t base = (uint64_t)(seg0 + s) * kSegEntries + (uint64_t)c * 16;
        const unsigned int n = qnl[s] - c * 16 < 16u ? qnl[s] - c * 16 : 16u;
        const uint4 k4 = *reinterpret_cast<const uint4 *>(qkey + base);
        const uint32_t kw[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
        for (unsigned int j = 0; j < 16; ++j) {
            if (j >= n) break;
            const uint32_t key = (kw[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            const uint32_t r = atomicAdd(&lh[key], 1u);
            qaux[base + j] = (key << 24) | r;
        }
    }
    __syncthreads();
    if (threadIdx.x < kBucketMax) {
        const unsigned int c = lh[threadIdx.x];
        kbase[(uint64_t)blockIdx.x * kBucketMax + threadIdx.x] = c ? atomicAdd(hdr + 64 + threadIdx.x, c) : 0u;
    }
    (void)L;
}

// The keys in walk order as one wave's lanes, two per lane: order kk = 2 lane
// + h (h = 0, 1); orders 0..63 are the all-open sub-keys 64..127 (64 sets
// per wave, one per lane), orders 64..127 the other first-level patterns
// 0..63 (per_light sets per wave).  Per half: the key's set count, its first
// sorted position and its wave range [wbeg, wend) in the launch's wave list.
struct BucketLanes {
    unsigned int tot[2], st[2], wbeg[2], wend[2], pk[2];
};
__device__ __forceinline__ uint32_t bucket_key(uint32_t kk) { return kk < 64 ? 64u + kk : kk - 64u; }
__device__ __forceinline__ BucketLanes bucket_lanes(const unsigned int *hdr, uint32_t per_light) {
    const int lane = threadIdx.x & 63;
    BucketLanes b;
    unsigned int nw[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t kk = 2u * (uint32_t)lane + (uint32_t)h;
        b.tot[h] = hdr[64 + bucket_key(kk)];
        b.pk[h] = kk < 64 ? 64u : per_light;
        nw[h] = (b.tot[h] + b.pk[h] - 1) / b.pk[h];
    }
    const unsigned int t2 = b.tot[0] + b.tot[1], w2 = nw[0] + nw[1];
    unsigned int st = t2, wi = w2;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int t = __shfl_up(st, o), u = __shfl_up(wi, o);
        if (lane >= o) {
            st += t;
            wi += u;
        }
    }
    b.st[0] = st - t2;
    b.st[1] = b.st[0] + b.tot[0];
    b.wbeg[0] = wi - w2;
    b.wend[0] = b.wbeg[0] + nw[0];
    b.wbeg[1] = b.wend[0];
    b.wend[1] = wi;
    return b;
}

// Every queued set's queue index at its sorted position: key start + the
// segment's base in the key + the set's rank (256-entry chunks of each
// segment, chunk-major, grid-stride).
__global__ void __launch_bounds__(256) walk_bucket_scatter_kernel(const unsigned long long *qseg,
                                                                  const uint32_t *qaux, const uint32_t *kbase,
                                                                  uint32_t nseg, int L, uint32_t *sidx) {
    const unsigned int *hdr =
        reinterpret_cast<const unsigned int *>(qseg + (uint64_t)nseg * kSegStride);
    __shared__ unsigned int kst[kBucketMax];
    if (threadIdx.x < 64) {
        const BucketLanes b = bucket_lanes(hdr, 64u);
        kst[bucket_key(2 * threadIdx.x)] = b.st[0];
        kst[bucket_key(2 * threadIdx.x + 1)] = b.st[1];
    }
    __syncthreads();
    (void)L;
    const uint64_t items = (uint64_t)nseg * (kSegEntries / 256);
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t seg = (uint32_t)(item % nseg);
        const uint64_t e = (item / nseg) * 256 + threadIdx.x;
        const uint64_t qc = qseg[(uint64_t)seg * kSegStride];
        const uint64_t qn = qc < kSegEntries ? qc : kSegEntries;
        if ((item / nseg) * 256 >= qn) continue;
        if (e >= qn) continue;
        const uint32_t ax = qaux[(uint64_t)seg * kSegEntries + e];
        const uint32_t key = ax >> 24, r = ax & 0xFFFFFFu;
        const uint32_t pos = kst[key] + kbase[(uint64_t)(seg / kBucketSegs) * kBucketMax + key] + r;
        sidx[pos] = (uint32_t)((uint64_t)seg * kSegEntries + e);
    }
}

// walk_load / walk_sliced / walk_store over the sorted index: wave w of the
// table walks its sets K per lane.
template <int L, int PHASE, int K, int NVMAX>
__device__ __forceinline__ void walk_group(const uint64_t *queue, const uint32_t *sidx, uint32_t st, uint32_t cnt,
                                           uint32_t *open_lds, float *table, float *hsub, uint64_t nslots,
                                           unsigned long long *err) {
    using S = Sliced<L, K>;
    static_assert(S::NV <= NVMAX, "open bits LDS");
    constexpr int W = bits_words(L);
    const uint32_t lane = threadIdx.x;
    typename S::Vec hiV, openV;
#pragma unroll
    for (int r = 0; r < S::NV; ++r) {
        hiV[r] = 0u;
        openV[r] = 0u;
    }
    uint32_t alive = 0u;
    uint32_t ent[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t p = lane * K + k;
        ent[k] = p < cnt ? sidx[st + p] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (ent[k] == 0xFFFFFFFFu) continue;
        alive |= 1u << k;
        const uint64_t *e = queue + (uint64_t)ent[k] * (1 + 2 * W);
        uint64_t hw[W], ow[W];
#pragma unroll
        for (int wj = 0; wj < W; ++wj) {
            hw[wj] = e[1 + wj];
            ow[wj] = e[1 + W + wj];
        }
#pragma unroll
        for (int r = 0; r < S::NV0; ++r) {
            const int t0 = r * S::E;
            constexpr uint32_t EM = (uint32_t)((1ull << S::E) - 1ull);
            const uint32_t hb = (uint32_t)(hw[t0 >> 6] >> (t0 & 63)) & EM;
            const uint32_t ob = (uint32_t)(ow[t0 >> 6] >> (t0 & 63)) & EM;
            uint32_t hs = 0u, os = 0u;
            if constexpr (S::K == 8) {
                hs = (hb * 0x00204081u) & 0x01010101u;
                os = (ob * 0x00204081u) & 0x01010101u;
            } else if constexpr (S::K == 1) {
                hs = hb;
                os = ob;
            } else {
#pragma unroll
                for (int f = 0; f < S::E; ++f) {
                    hs |= ((hb >> f) & 1u) << (S::K * f);
                    os |= ((ob >> f) & 1u) << (S::K * f);
                }
            }
            hiV[r] |= hs << k;
            openV[r] |= os << k;
        }
    }
    constexpr bool v0inP = PHASE == 0;
    constexpr uint32_t Plocal = v0inP ? ((1u << L) - 1u) : (((1u << L) - 1u) << 1);
    uint32_t pvtop = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) pvtop |= (uint32_t)(i + (v0inP ? 0 : 1)) << (4 * i);
    uint32_t dom = 0u, pts = 0u;
    OpenLds<L, K, NVMAX * 64> ol{open_lds + lane};
#pragma unroll
    for (int r = 0; r < S::NV; ++r) {
        ol.base[r * 64] = openV[r];
        ol.base[r * 64 + NVMAX * 64] = hiV[r];
    }
    walk_sliced<L, K, L, false, OpenLds<L, K, NVMAX * 64>, PHASE>(Plocal, pvtop, alive, hiV, ol, alive, dom, pts);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (ent[k] == 0xFFFFFFFFu) continue;
        const uint64_t e0 = queue[(uint64_t)ent[k] * (1 + 2 * W)];
        const float ts = __uint_as_float((uint32_t)(e0 >> 32));
        const bool d = (dom >> k) & 1u;
        const uint32_t slot = (uint32_t)e0;
        if (slot >= nslots) {
            atomicOr(err, kErrSlot);
            continue;
        }
        table[slot] = d ? absent_f() : -ts;
        if (hsub && !d) hsub[slot] = fmaxf(hsub[slot], -ts);
    }
}

// hdr: the launch's bucket header (key totals); waves in key order, the
// all-open key's first (bucket_lanes), a grid-stride loop over them.
template <int L, int PHASE, int KL>
__global__ void __launch_bounds__(64) walk_bucket_kernel(const uint64_t *queue, const uint32_t *sidx,
                                                         const unsigned int *hdr, float *table, float *hsub,
                                                         uint64_t nslots, unsigned long long *err) {
    constexpr int NVMAX = Sliced<L, KL>::NV > Sliced<L, 1>::NV ? Sliced<L, KL>::NV : Sliced<L, 1>::NV;
    __shared__ uint32_t open_lds[2 * NVMAX * 64];  // open bits, then the hi copy
    const BucketLanes b = bucket_lanes(hdr, 64u * KL);
    const uint32_t nw = __shfl(b.wend[1], 63);
    for (uint32_t w = blockIdx.x; w < nw; w += gridDim.x) {
        // the lane holding wave w: the first whose range ends past w; then its half
        const unsigned long long past = __ballot(b.wend[1] > w);
        const int ln = __ffsll((long long)past) - 1;
        const bool h1 = __shfl(b.wend[0], ln) <= w;
        const uint32_t wbeg = h1 ? __shfl(b.wbeg[1], ln) : __shfl(b.wbeg[0], ln);
        const uint32_t st = h1 ? __shfl(b.st[1], ln) : __shfl(b.st[0], ln);
        const uint32_t tot = h1 ? __shfl(b.tot[1], ln) : __shfl(b.tot[0], ln);
        const uint32_t pk = h1 ? __shfl(b.pk[1], ln) : __shfl(b.pk[0], ln);
        const uint32_t kk = 2u * (uint32_t)ln + (h1 ? 1u : 0u);
        const uint32_t off = (w - wbeg) * pk;
        const uint32_t cw = tot - off < pk ? tot - off : pk;
        if (kk < 64)
            walk_group<L, PHASE, 1, NVMAX>(queue, sidx, st + off, cw, open_lds, table, hsub, nslots, err);
        else
            walk_group<L, PHASE, KL, NVMAX>(queue, sidx, st + off, cw, open_lds, table, hsub, nslots, err);
    }
}

// ---- wide layers (kMaxL < L <= kWideMax) ------------------------------------
// The reference's default parent limit is n - 1 (score_main.cpp:296-298), so on
// small n (data/hepatitis.clean.csv: n = 20) the layers run to 19 parents.
// Those layers use runtime-L kernels: the same Cholesky-of-the-Gram score per
// lane (the triangle in private memory), the direct-children decision in the
// scoring kernel (a present child P\{a} >= -ts is always visited at the top
// level: present keys never enter `checked`), and, for the rest, an explicit
// stack replay of find_best_subset_score (BIC_OLS.cpp:125-172)
// whose `checked` set is a 2^q-bit bitset per walking set in HBM (q local
// bits: P, plus variable 0 when P lacks it).
constexpr uint64_t kWideStepCap = 1ull << 30;  // per-set walk steps before the call fails loudly

__device__ __forceinline__ uint64_t B64(const uint64_t *b, int a, int k) { return b[a * 64 + k]; }

__device__ __forceinline__ uint64_t unrank_colex64(uint64_t r, int l, int U, const uint64_t *b) {
    uint64_t mask = 0;
    int c = U - 1;
    for (int i = l; i >= 1; --i) {
        while (c >= 0 && B64(b, c, i) > r) --c;
        mask |= 1ull << c;
        r -= B64(b, c, i);
        --c;
    }
    return mask;
}

__device__ __forceinline__ uint64_t rank_colex64(uint64_t mask, const uint64_t *b) {
    uint64_t r = 0;
    int j = 0;
    while (mask) {
        const int x = __builtin_ctzll(mask);
        mask &= mask - 1;
        ++j;
        r += B64(b, x, j);
    }
    return r;
}

struct WideArgs {
    const double *gram;       // n x n row-major
    const uint64_t *binom;    // [64][64]
    const uint8_t *cand;      // [nv][64]
    const int *meta;          // [nv][4]
    const uint64_t *tbl_off;  // [nv*S + 1]
    const uint64_t *work;     // [nv + 1] prefix of this launch's sets
    float *table;
    uint64_t *queue;          // 3 words per undecided set: slot, compact mask, vi | ts bits << 32
    unsigned long long *qcount;
    const float *hmax;        // hi-cover tables (hikey_*_kernel) or null
    const float *pval;        // the same variables' present keys by compact mask (absent bits otherwise)
    const uint64_t *hoff;     // [nv] offset of a variable's tables in hmax / pval, ~0 = none
    int reduced;              // walk_wide_kernel: skip the reference's no-op re-tests
    double N;
    double pen;               // lambda ln(N), the device's product (ulg_ctx::pen)
    int n, nv, S, L;
};

// A wide layer's scoring launch: the regression, the ts >= 0 exit, the direct
// children's test; the undecided sets go to the walk queue.
#define ULG_CONS 0
#include "cbic_score_wide.inc"
#undef ULG_CONS
#define ULG_CONS 1
#include "cbic_score_wide.inc"
#undef ULG_CONS

// One lane per queued set: find_best_subset_score replayed step by step.  A
// frame at depth d holds T, the parent vector (L - d entries; entries past the
// filled ones are 0 = variable 0), the outer index idx, and while a
// child list is being built the inner position i, the fill j and u.  The walk
// stops at the first visited key >= -ts: that alone decides the store rule
// (BIC_OLS.cpp:234 with best starting at 0 < -ts).
template <int LMAX, int PHASE>
__global__ void __launch_bounds__(64) walk_wide_kernel(WideArgs a, uint64_t qbase, uint64_t qn, uint64_t *bits,
                                                       uint64_t wpl, unsigned long long *err,
                                                       unsigned long long *wstats, uint64_t budget,
                                                       uint64_t *squeue, unsigned long long *scount) {
    const uint64_t lid = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t qi = qbase + lid;
    if (qi >= qn) return;
    const uint64_t *e = a.queue + 3 * qi;
    const uint64_t slot = e[0], cm = e[1];
    const int vi = (int)(uint32_t)e[2];
    const float ts = __uint_as_float((uint32_t)(e[2] >> 32));
    const int L = a.L;
    const bool z = a.meta[vi * 4 + 2] != 0;
    uint8_t lc[LMAX + 1];  // local bit -> compact index
    uint64_t Plocal;
    {
        uint64_t rem = cm;
        const int first = PHASE == 0 ? 0 : 1;
        lc[0] = 0;
        for (int i = first; i < L + first; ++i) {
            lc[i] = (uint8_t)__builtin_ctzll(rem);
            rem &= rem - 1;
        }
        Plocal = PHASE == 0 ? ((1ull << L) - 1ull) : (((1ull << L) - 1ull) << 1);
    }
    const uint64_t *toffv = a.tbl_off + (uint64_t)vi * a.S;
    const float thr = -ts;
    // Hi-cover prune: the walk's answer is only whether it visits a present key
    // >= -ts (a "hi" key).  From a node T it can only visit subsets of T and
    // variable 0 (U(T)), so an absent T whose U(T) holds no hi key is not
    // expanded (marked checked, as its call would have been).  Expanding it
    // could only change `checked` inside U(T), and every later difference
    // stays inside U(T) (U is monotone), so the first hi key visited -- the
    // decision -- is unchanged.  hmax[X] = max over the keys present when
    // this phase runs of the subsets of the compact mask X.
    // With the tables, a node also carries its compact mask Tc (variable 0 is
    // compact bit 0 when it is a candidate), and the presence test is one read
    // of pval[Tc] instead of a colex rank over the node's bits.
    const uint64_t ho = a.hoff ? a.hoff[vi] : ~0ull;
    const bool dense = ho != ~0ull;
    const uint64_t zb = z ? 1ull : 0ull;
    auto cbit = [&](int u) -> uint64_t { return u == 0 ? zb : (1ull << lc[u]); };
    auto hi_in_cover = [&](uint64_t Tc) -> bool { return !dense || a.hmax[ho + (Tc | zb)] >= thr; };
    if (!hi_in_cover(cm)) {  // no hi key below P at all: stored
        a.table[slot] = -ts;
        return;
    }
    uint64_t *chk = bits + lid * wpl;
    chk[0] |= 1ull;  // checked.insert(empty_set)

    // Re-test skipping (a.reduced): the inner loop calls fb(T2, npv) once per
    // appended entry, with npv = the first j appended entries + zero padding.
    // In call j >= 2 the positions below j-1 were tested by the earlier calls
    // (each is now checked, or a present key below -ts: testing it again
    // changes nothing) and the positions from j on are zeros, whose child
    // T2 ^ {0} call 1 already tested at its position 1.  So call 1 tests
    // positions 0 and 1 and call j >= 2 only position j-1: the same tests in
    // the same order, minus the no-ops (O(m) instead of O(m^2) per expanded
    // node).  ends[d] is where the current call at depth d stops.
    uint64_t Ts[LMAX + 1], Tcs[LMAX + 1];
    uint8_t idxs[LMAX + 1], is[LMAX + 1], js[LMAX + 1], us[LMAX + 1], inner[LMAX + 1], ends[LMAX + 1];
    uint8_t pvs[LMAX * (LMAX + 1) / 2 + 1];
    for (int i = 0; i < L; ++i) pvs[i] = (uint8_t)(i + (PHASE == 0 ? 0 : 1));
    int d = 0;
    Ts[0] = Plocal;
    Tcs[0] = cm;
    idxs[0] = 0;
    ends[0] = (uint8_t)L;
    inner[0] = 0;
    bool dom = false;
    uint64_t steps = 0;
    while (true) {
        if (++steps > kWideStepCap) {
            atomicOr(err, 1ull);
            break;
        }
        if (budget && steps > budget && dense) {
            // a long walk: hand it to walk_wide_lds_kernel, which replays it
            // from the start with every bitset in LDS (same walk)
            const unsigned long long pos = atomicAdd(scount, 1ull);
            squeue[3 * pos] = e[0];
            squeue[3 * pos + 1] = e[1];
            squeue[3 * pos + 2] = e[2];
            return;
        }
        const int mm = L - d;
        const int po = d * L - d * (d - 1) / 2;  // pvs offset of depth d
        if (!inner[d]) {
            if (idxs[d] == ends[d]) {  // fb returns
                if (d == 0) break;
                --d;
                const uint64_t c = Ts[d + 1];
                chk[c >> 6] |= 1ull << (c & 63);  // checked.insert(thin_parents) after the call
                continue;
            }
            const uint8_t u = pvs[po + idxs[d]];
            const uint64_t T2 = Ts[d] ^ (1ull << u);
            if ((chk[T2 >> 6] >> (T2 & 63)) & 1ull) {
                ++idxs[d];
                continue;
            }
            const uint64_t T2c = Tcs[d] ^ cbit(u);
            // is T2 in the cache as it stood when P was scored?
            bool present = false;
            const int pc = __popcll(T2);
            if (dense) {
                // pval holds exactly the keys of that cache (hikey_tile_kernel);
                // variable 0 outside the candidates is never a key's member
                if (!(PHASE == 1 && (T2 & 1ull) && !z)) {
                    const float val = a.pval[ho + T2c];
                    if (fbits(val) != kAbsentBits) {
                        present = true;
                        if (val >= thr) {
                            dom = true;
                            break;
                        }
                    }
                }
            } else if (pc < L || (PHASE == 1 && pc == L && (T2 & 1ull))) {
                if (!(PHASE == 1 && (T2 & 1ull) && !z)) {
                    uint64_t rk = 0, rem = T2;
                    int j = 0;
                    while (rem) {
                        const int lb = __builtin_ctzll(rem);
                        rem &= rem - 1;
                        ++j;
                        rk += B64(a.binom, lc[lb], j);
                    }
                    const float val = a.table[toffv[pc] + rk];
                    if (fbits(val) != kAbsentBits) {
                        present = true;
                        if (val >= thr) {
                            dom = true;
                            break;
                        }
                    }
                }
            }
            if (present) {
                ++idxs[d];
                continue;
            }
            if (!hi_in_cover(T2c)) {
                chk[T2 >> 6] |= 1ull << (T2 & 63);
                ++idxs[d];
                continue;
            }
            inner[d] = 1;
            is[d] = 0;
            js[d] = 0;
            us[d] = u;
            for (int k = 0; k < mm - 1; ++k) pvs[po + mm + k] = 0;
            continue;
        }
        if (is[d] == mm) {
            inner[d] = 0;
            ++idxs[d];
            continue;
        }
        const uint8_t pi = pvs[po + is[d]];
        ++is[d];
        if (pi == us[d]) continue;
        pvs[po + mm + js[d]] = pi;
        ++js[d];
        Ts[d + 1] = Ts[d] ^ (1ull << us[d]);
        Tcs[d + 1] = Tcs[d] ^ cbit(us[d]);
        if (a.reduced) {
            const int j = js[d];  // this is call j of fb(T2, npv)
            idxs[d + 1] = (uint8_t)(j == 1 ? 0 : j - 1);
            ends[d + 1] = (uint8_t)(j == 1 ? (mm - 1 < 2 ? mm - 1 : 2) : j);
        } else {
            idxs[d + 1] = 0;
            ends[d + 1] = (uint8_t)(mm - 1);
        }
        inner[d + 1] = 0;
        ++d;
    }
    a.table[slot] = dom ? absent_f() : -ts;
    if (wstats) {  // ULG_WALK_STATS: walks, steps, max steps, walks over 2^20 steps
        atomicAdd(&wstats[0], 1ull);
        atomicAdd(&wstats[1], (unsigned long long)steps);
        atomicMax(&wstats[2], (unsigned long long)steps);
        if (steps > (1ull << 20)) atomicAdd(&wstats[3], 1ull);
    }
}

using WideFn = void (*)(WideArgs);
using WideWalkFn = void (*)(WideArgs, uint64_t, uint64_t, uint64_t *, uint64_t, unsigned long long *,
                           unsigned long long *, uint64_t, uint64_t *, unsigned long long *);
WideFn wide_fn(int L, int phase) {
    if (L <= 16) return phase == 0 ? score_wide_kernel<16, 0> : score_wide_kernel<16, 1>;
    return phase == 0 ? score_wide_kernel<kWideMax, 0> : score_wide_kernel<kWideMax, 1>;
}
// the constrained twin (launch_twin)
using WideConsFn = void (*)(WideArgs, const uint64_t *, int);
WideConsFn wide_cons_fn(int L, int phase) {
    if (L <= 16) return phase == 0 ? score_wide_cons_kernel<16, 0> : score_wide_cons_kernel<16, 1>;
    return phase == 0 ? score_wide_cons_kernel<kWideMax, 0> : score_wide_cons_kernel<kWideMax, 1>;
}
WideWalkFn wide_walk_fn(int L, int phase) {
    if (L <= 16) return phase == 0 ? walk_wide_kernel<16, 0> : walk_wide_kernel<16, 1>;
    return phase == 0 ? walk_wide_kernel<kWideMax, 0> : walk_wide_kernel<kWideMax, 1>;
}

// ---- long wide walks in LDS -----------------------------------------------
// A wide walk is one lane's sequential DFS; the few long ones set a layer's
// time (C1 at the reference's default lambda 0.5: single walks of 5-19 M
// steps at L = 18, 19), and in walk_wide_kernel every step waits on scratch
// memory and global bitsets (~1 us).  Walks over kStragBudget steps (only
// where q = |local bits| <= kStragQMax and the hi-cover tables exist) are
// re-queued and replayed here from the start, one workgroup per set.
//
// Fill: the workgroup lays out, over the 2^q local subsets, two bitsets from
// pval / hmax: `skip` (present below -ts, or absent with no key >= -ts among
// its subsets and variable 0: a test of it changes nothing but `checked`,
// which it would never consult again) and `hi` (present and >= -ts: the walk
// stops there).  A test is then: skip bit set (or checked) -> next; hi bit set
// -> dominated; otherwise expand.  `checked` merges into `skip`: checked nodes
// are expanded ones, never hi, and the empty set starts checked.
//
// Walk (lane 0): the reduced walk of walk_wide_kernel with every parent-vector
// list held as a bit mask.  A list is its real entries in increasing local-bit
// order followed by zero padding (the root list is P's bits; an expansion of
// T2 = T ^ {x} appends the caller's entries != x in order, so order is kept,
// and zeros appended from the padding read like padding), so a frame is: node
// N, removed entry x, the caller's list (remaining mask `rem`, remaining zeros
// `zr`), the appended mask B, the call count js, and whether the current call
// still owes its position-1 test (call 1 tests positions 0 and 1, call j >= 2
// position j - 1 = the entry it appended).  N is checked after each call of
// its expansion returns (BIC_OLS.cpp:234 recursion).  Wave 0 runs
// the walk with its lanes reading a node's q neighbour bits at once, so a
// test is a register bit test; frames are 32 B in LDS, pushed per expansion.
constexpr int kStragQMax = 20;                 // skip bitset 2^20 bits = 128 KiB of LDS
constexpr int kStragHiLdsQ = 19;               // hi bitset in LDS up to here, else in global scratch
constexpr uint64_t kStragBudget = 1ull << 6;  // steps in walk_wide_kernel before a walk moves here (2^13 -> 2^6: C4 0.82 -> 0.24 s, C1 10.0 -> 9.4 s)
// ULG_STRAG_BUDGET=<log2 steps> overrides it (A/B timing only: results are the same)
inline uint64_t strag_budget() {
    static const uint64_t b = std::getenv("ULG_STRAG_BUDGET") ? 1ull << std::atoi(std::getenv("ULG_STRAG_BUDGET"))
                                                              : kStragBudget;
    return b;
}
constexpr int kStragThreads = 256;             // fill threads (64 when many walks share the GPU); wave 0 walks
constexpr uint64_t kStragWide = 4096;          // replays per launch from which blocks are one wave

// The fill of one replay (entry e of the straggler queue) into skip / hib
// (word w at skip[w * stride], hib[w * stride]): lc (>= 32 bytes) and xlow
// (64 words), shared by the block, receive the local-bit -> compact index
// map and the compact masks of the 64 low-bit patterns.  Every thread of the
// block takes words w = tid, tid + nthreads, ...
template <int PHASE>
__device__ __forceinline__ void strag_fill(const WideArgs &a, const uint64_t *e, uint64_t *skip, uint64_t *hib,
                                           uint32_t stride, uint8_t *lc, uint64_t *xlow, uint32_t tid,
                                           uint32_t nthreads) {
    const int L = a.L;
    const int q = PHASE == 0 ? L : L + 1;
    const uint32_t nw = (1u << q) >> 6;
    const uint64_t cm = e[1];
    const int vi = (int)(uint32_t)e[2];
    const float thr = -__uint_as_float((uint32_t)(e[2] >> 32));
    const bool z = a.meta[vi * 4 + 2] != 0;
    const uint64_t zb = z ? 1ull : 0ull;
    const uint64_t ho = a.hoff[vi];
    if (tid == 0) {
        uint64_t rem = cm;
        const int first = PHASE == 0 ? 0 : 1;
        lc[0] = 0;
        for (int i = first; i < L + first; ++i) {
            lc[i] = (uint8_t)__builtin_ctzll(rem);
            rem &= rem - 1;
        }
    }
    __syncthreads();
    if (tid < 64) {  // compact mask of local bits 1..5 of pattern tid (bit 0 = variable 0: zb)
        uint64_t X = 0;
        for (uint32_t y = tid & ~1u; y; y &= y - 1) X |= 1ull << lc[__builtin_ctz(y)];
        xlow[tid] = X | ((tid & 1u) ? zb : 0ull);
    }
    __syncthreads();
    for (uint32_t w = tid; w < nw; w += nthreads) {
        uint64_t sw = 0, hw = 0;
        uint64_t Xw = 0;  // compact mask of the word's high local bits
        for (uint32_t y = (w << 6); y; y &= y - 1) Xw |= 1ull << lc[__builtin_ctz(y)];
#pragma unroll 8
        for (int b = 0; b < 64; ++b) {
            const uint32_t t = (w << 6) | (uint32_t)b;
            const uint64_t X = Xw | xlow[b];
            bool pres = false, hi = false;
            if (!(PHASE == 1 && (t & 1u) && !z)) {
                const float val = a.pval[ho + X];
                if (fbits(val) != kAbsentBits) {
                    pres = true;
                    hi = val >= thr;
                }
            }
            const bool sk = t == 0 || (pres ? !hi : !(a.hmax[ho + (X | zb)] >= thr));
            if (sk) sw |= 1ull << b;
            if (hi && t != 0) hw |= 1ull << b;
        }
        skip[(uint64_t)w * stride] = sw;
        hib[(uint64_t)w * stride] = hw;
    }
    __syncthreads();
}

// The fills of the replays handed to the host (one block each, entries
// sq[3 * idx[b]]), written to out: [b][skip nw words][hi nw words].
template <int PHASE>
__global__ void __launch_bounds__(256) strag_fill_global_kernel(WideArgs a, const uint64_t *sq, const uint32_t *idx,
                                                                uint64_t *out) {
    __shared__ uint8_t lc[64];
    __shared__ uint64_t xlow[64];
    const int q = PHASE == 0 ? a.L : a.L + 1;
    const uint64_t nw = ((uint64_t)1 << q) >> 6;
    uint64_t *o = out + (uint64_t)blockIdx.x * 2 * nw;
    strag_fill<PHASE>(a, sq + 3 * (uint64_t)idx[blockIdx.x], o, o + nw, 1, lc, xlow, threadIdx.x, blockDim.x);
}

// host_budget > 0: a walk still running after that many iterations stops,
// and its queue index goes to hq (count *hqc) for the host (host_walk):
// one wave issues at most one instruction every 4 cycles, so a long
// sequential walk runs far faster on a host core.
template <int PHASE, bool HI_LDS>
__global__ void __launch_bounds__(kStragThreads) walk_wide_lds_kernel(WideArgs a, const uint64_t *sq,
                                                                      uint64_t *hig, unsigned long long *err,
                                                                      unsigned long long *wstats, uint64_t host_budget,
                                                                      uint32_t *hq, unsigned int *hqc, uint32_t qbase) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int L = a.L;
    const int q = PHASE == 0 ? L : L + 1;
    const uint32_t nw = (1u << q) >> 6;
    // HI_LDS: skip and hi words interleaved (one 16-B read per neighbour);
    // else skip in LDS and hi in this block's global scratch
    constexpr uint32_t kS = HI_LDS ? 2u : 1u;
    uint64_t *skip = reinterpret_cast<uint64_t *>(smem);
    uint64_t *hib = HI_LDS ? skip + 1 : hig + (uint64_t)blockIdx.x * nw;
    uint64_t *xlow = skip + (HI_LDS ? 2 * nw : nw);
    uint8_t *lc = reinterpret_cast<uint8_t *>(xlow + 64);
    const uint64_t *e = sq + 3 * (uint64_t)blockIdx.x;
    const uint64_t slot = e[0];
    const float ts = __uint_as_float((uint32_t)(e[2] >> 32));
    const uint64_t tk0 = wstats ? wall_clock64() : 0;
    strag_fill<PHASE>(a, e, skip, hib, kS, lc, xlow, threadIdx.x, blockDim.x);
    if (threadIdx.x >= 64) return;
    // wave 0 walks, every lane in step (the walk state is wave-uniform); the
    // lanes only split up to read a node's neighbour bits: bit l of sm / hm is
    // the skip / hi bit of N ^ {l}.  Within one expansion only its children's
    // subtrees change `skip` (N's own mark is not a neighbour of N), so sm is
    // re-read after each child returns and every test is a register bit test.
    const int lane = threadIdx.x;
    const uint64_t tk1 = wstats ? wall_clock64() : 0;
    // lanes >= q read a valid word too, so both loads issue back to back
    const uint32_t lbit = 1u << (lane < q ? lane : 0);
    auto nbr = [&](uint32_t Nn, uint32_t &sm_, uint32_t &hm_) {
        const uint32_t t = Nn ^ lbit;
        uint64_t sw, hw;
        if constexpr (HI_LDS) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(skip + 2 * (t >> 6));
            sw = v.x;
            hw = v.y;
        } else {
            sw = skip[t >> 6];
            hw = hib[t >> 6];
        }
        sm_ = (uint32_t)__ballot((int)(((sw >> (t & 63)) & 1ull) | (lane >= q)));
        hm_ = (uint32_t)__ballot((int)(((hw >> (t & 63)) & 1ull) & (lane < q)));
    };
    // frames in VGPR lanes: lane d of fN .. fSm holds frame d (kStragDepth <= 64)
    uint32_t fN = 0, fRem = 0, fB = 0, fW = 0, fHm = 0, fSm = 0;
    auto wl = [&](uint32_t v, int l, uint32_t old) -> uint32_t { return lane == l ? v : old; };
    auto rl = [](uint32_t v, int l) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); };
    const uint32_t P = PHASE == 0 ? ((1u << L) - 1u) : (((1u << L) - 1u) << 1);
    uint32_t N = P, rem = P, B = 0, sm, hm;
    nbr(N, sm, hm);
    int x = 31, zr = 0, js = 0, d = 0, mS = L;
    bool pend = false, incall = false, dom = false;
    uint64_t it = 0;
    while (true) {
        if (++it > kStragIterCap) {
            if (lane == 0) atomicOr(err, 1ull);
            break;
        }
        if (host_budget && it > host_budget) {  // to the host, from the start
            if (lane == 0) hq[atomicAdd(hqc, 1u)] = qbase + blockIdx.x;
            return;
        }
        int y;
        if (pend) {  // call 1's position-1 test: the zero padding, variable 0
            pend = false;
            y = 0;
        } else {
            if (incall) {  // the call returned: checked.insert(N)
                if (lane == 0) atomicOr(&skip[(N >> 6) * kS], 1ull << (N & 63));
                incall = false;
            }
            // Next test that is not a no-op.  A test whose node has its skip
            // bit set changes nothing, so after call 1 (N is checked from then
            // on) a run of such calls only appends its entries to B.
            const uint32_t xb = x < 32 ? 1u << x : 0u;
            const uint32_t cand = rem & ~xb;  // real entries that make calls
            bool found = false;
            if (d == 0) {  // the root call: P's entries, no appends
                const uint32_t ev = rem & ~sm;
                if (ev) {
                    y = __builtin_ctz(ev);
                    rem &= ~((2u << y) - 1u);
                    found = true;
                }
            } else if (js == 0) {  // call 1, with its position-1 test
                if (cand) {
                    y = __builtin_ctz(cand);
                    rem &= ~((2u << y) - 1u);
                    B |= 1u << y;
                    found = true;
                } else if (zr && x != 0) {  // the first entry is padding
                    --zr;
                    y = 0;
                    found = true;
                }
                if (found) {
                    js = 1;
                    incall = true;
                    pend = mS - 1 >= 2;
                }
            } else {
                const uint32_t ev = cand & ~sm;
                if (ev) {
                    y = __builtin_ctz(ev);
                    const uint32_t run = cand & ((2u << y) - 1u);  // skipped calls + this one
                    B |= run;
                    js += __popc(run);
                    rem &= ~((2u << y) - 1u);
                    incall = true;
                    found = true;
                } else {
                    B |= cand;  // the rest of the real entries: no-op calls
                    js += __popc(cand);
                    rem = 0;
                    if (zr && x != 0) {  // padding entries: each a call testing N ^ {0}
                        if (sm & 1u) {
                            js += zr;
                            zr = 0;
                        } else {
                            --zr;
                            ++js;
                            y = 0;
                            incall = true;
                            found = true;
                        }
                    }
                }
            }
            if (!found) {  // the expansion (or the root call) is done
                if (d == 0) break;
                // Back in the caller's frame, whose neighbour bits the subtree of
                // N = caller ^ {x} changed only at N itself (marked iff it made
                // a call) when x != 0: x never re-enters a list below it, so
                // every node of the subtree differs from the caller in bit x.
                // Variable 0 re-enters as padding: then read them again.
                const int cx = x;
                const bool cmarked = js > 0;
                --d;
                N = rl(fN, d);
                rem = rl(fRem, d);
                B = rl(fB, d);
                const uint32_t w = rl(fW, d);
                hm = rl(fHm, d);
                sm = rl(fSm, d);
                x = (int)(w & 31u);
                zr = (int)((w >> 5) & 31u);
                js = (int)((w >> 10) & 31u);
                pend = (w >> 15) & 1u;
                incall = (w >> 16) & 1u;
                mS = d == 0 ? L : L - d + 1;
                if (cx != 0) {
                    if (cmarked) sm |= 1u << cx;
                } else {
                    uint32_t h2;
                    nbr(N, sm, h2);
                }
                continue;
            }
        }
        if ((sm >> y) & 1u) continue;
        if ((hm >> y) & 1u) {
            dom = true;
            break;
        }
        // expand N ^ {y} with the current call's list (root: P's bits; else B_j)
        const uint32_t Sc = d == 0 ? P : B;
        const int mc = d == 0 ? L : mS - 1;
        if (d + 1 >= kStragDepth || mc < __popc(Sc)) {  // cannot happen: the list holds its entries
            if (lane == 0) atomicOr(err, 1ull);
            break;
        }
        fN = wl(N, d, fN);
        fRem = wl(rem, d, fRem);
        fB = wl(B, d, fB);
        fW = wl((uint32_t)x | ((uint32_t)zr << 5) | ((uint32_t)js << 10) | ((uint32_t)pend << 15) |
                    ((uint32_t)incall << 16),
                d, fW);
        fHm = wl(hm, d, fHm);
        fSm = wl(sm, d, fSm);
        ++d;
        N ^= 1u << y;
        x = y;
        rem = Sc;
        zr = mc - __popc(Sc);
        B = 0;
        js = 0;
        pend = false;
        incall = false;
        mS = mc;
        nbr(N, sm, hm);
    }
    if (lane != 0) return;
    a.table[slot] = dom ? absent_f() : -ts;
    if (wstats) {  // ULG_WALK_STATS: replays, iterations, max iterations, max fill / walk ticks
        const uint64_t tk2 = wall_clock64();
        atomicAdd(&wstats[4], 1ull);
        atomicAdd(&wstats[5], (unsigned long long)it);
        atomicMax(&wstats[6], (unsigned long long)it);
        atomicMax(&wstats[7], (unsigned long long)(tk1 - tk0));
        atomicMax(&wstats[8], (unsigned long long)(tk2 - tk1));
    }
}

// ---- hi-cover tables for the wide walks ---------------------------------
// Per walking variable (m <= kHiMaxBits candidates), before each wide walk
// launch: hmax[X] = max over the keys present in the cache when this phase
// runs (layers < L, and in phase 1 the layer-L sets holding variable 0,
// SURVEY N4) of their stored value, over every subset of the compact mask X;
// absent keys count as -inf.  A subset-max (zeta) transform: the low
// kHiTileBits bits per LDS tile, the rest kHiGroup bits per strided pass.
constexpr int kHiTileBits = 12;  // tables of up to kHiMaxBits bits (score_plan.h)
constexpr int kHiGroup = 4;

struct HiArgs {
    const int *lvars;     // walking variables of this launch (batch index)
    const int *prefix;    // [nl + 1]: tiles (tile pass) or blocks (strided pass) per variable
    int nl;
    const int *meta;
    const uint64_t *tbl_off;
    const float *table;
    const uint64_t *binom;  // [64][64]
    float *hmax;
    float *pval;
    const uint64_t *hoff;
    int S, L, kmax, bit_lo;
};

__device__ __forceinline__ int hi_find(const int *prefix, int nl, int x) {
    int lo = 0, hi = nl;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

template <int PHASE>
__global__ void __launch_bounds__(1024) hikey_tile_kernel(HiArgs a) {
    __shared__ float t[1 << kHiTileBits];
    const int li = hi_find(a.prefix, a.nl, blockIdx.x);
    const int vi = a.lvars[li];
    const int m = a.meta[vi * 4 + 1];
    const bool z = a.meta[vi * 4 + 2] != 0;
    const int tb = m < kHiTileBits ? m : kHiTileBits;
    const int cnt = 1 << tb;
    const uint64_t base = (uint64_t)(blockIdx.x - a.prefix[li]) << kHiTileBits;
    const uint64_t *toff = a.tbl_off + (uint64_t)vi * a.S;
    for (int i = threadIdx.x; i < cnt; i += 1024) {
        const uint64_t X = base + (uint64_t)i;
        const int l = __popcll(X);
        float val = -INFINITY, pv = absent_f();
        if (l <= a.kmax && (l < a.L || (PHASE == 1 && l == a.L && (X & 1ull) && z))) {
            const float f = a.table[toff[l] + rank_colex64(X, a.binom)];
            pv = f;
            if (fbits(f) != kAbsentBits && f == f) val = f;  // absent or NaN: never >= -ts
        }
        a.pval[a.hoff[vi] + X] = pv;
        t[i] = val;
    }
    __syncthreads();
    for (int b = 0; b < tb; ++b) {
        for (int i = threadIdx.x; i < cnt; i += 1024)
            if (!((i >> b) & 1)) t[i | (1 << b)] = fmaxf(t[i | (1 << b)], t[i]);
        __syncthreads();
    }
    float *h = a.hmax + a.hoff[vi] + base;
    for (int i = threadIdx.x; i < cnt; i += 1024) h[i] = t[i];
}

__global__ void __launch_bounds__(256) hikey_strided_kernel(HiArgs a) {
    const int li = hi_find(a.prefix, a.nl, blockIdx.x);
    const int vi = a.lvars[li];
    const int m = a.meta[vi * 4 + 1];
    const int G = m - a.bit_lo < kHiGroup ? m - a.bit_lo : kHiGroup;
    const uint64_t tid = (uint64_t)(blockIdx.x - a.prefix[li]) * 256 + threadIdx.x;
    if (G <= 0 || tid >= (1ull << (m - G))) return;
    const uint64_t lowm = (1ull << a.bit_lo) - 1ull;
    const uint64_t base = ((tid & ~lowm) << G) | (tid & lowm);
    float *h = a.hmax + a.hoff[vi];
    float r[1 << kHiGroup];
    for (int k = 0; k < (1 << G); ++k) r[k] = h[base + ((uint64_t)k << a.bit_lo)];
    for (int b = 0; b < G; ++b)
        for (int k = 0; k < (1 << G); ++k)
            if (!((k >> b) & 1)) r[k | (1 << b)] = fmaxf(r[k | (1 << b)], r[k]);
    for (int k = 0; k < (1 << G); ++k) h[base + ((uint64_t)k << a.bit_lo)] = r[k];
}

// The call's first launch: cache[empty] = -0.0f per variable (BIC_OLS.cpp:249)
// and the walk-queue counters zeroed.  It sits inside the call's hipGraph;
// as three eager launches before the replay (a kernel and two memsets) they
// left ~40 us of submission gaps ahead of the first layer.
__global__ void call_prologue_kernel(const uint64_t *tbl_off, int nv, int S, float *table,
                                     unsigned long long *qcount, uint64_t nqc, unsigned long long *qseg,
                                     uint64_t nseg) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (uint64_t)nv) table[tbl_off[i * (uint64_t)S]] = -0.0f;
    if (qcount && i < nqc) qcount[i] = 0ull;
    if (qseg && i < nseg) qseg[i] = 0ull;
}
// ... under constraints: a variable whose every alternative requires a parent
// has cache[empty] = -float(n) (the violator's value falls through to
// BIC_OLS.cpp:249 and score_calculator.cpp:59 keeps it)
__global__ void call_prologue_cons_kernel(const uint64_t *tbl_off, int nv, int S, float *table,
                                          unsigned long long *qcount, uint64_t nqc, unsigned long long *qseg,
                                          uint64_t nseg, const uint64_t *cons, int n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (uint64_t)nv) table[tbl_off[i * (uint64_t)S]] = cons_violates(cons, nv, (int)i, 0ull) ? -(float)n : -0.0f;
    if (qcount && i < nqc) qcount[i] = 0ull;
    if (qseg && i < nseg) qseg[i] = 0ull;
}

// ---- compaction of the slabs into (set, score) lists ------------------------
// kSlotsPerThread contiguous slots per thread, kSlotsPerBlock per block (score_plan.h)

// the thread's kSlotsPerThread slots from `base` (absent past the end)
__device__ __forceinline__ void load_slots(const float *table, uint64_t total, uint64_t base,
                                           float (&v)[kSlotsPerThread]) {
    if (base + kSlotsPerThread <= total) {
        const float4 *p = reinterpret_cast<const float4 *>(table + base);
#pragma unroll
        for (int q = 0; q < kSlotsPerThread / 4; ++q) {
            const float4 f = p[q];
            v[4 * q] = f.x;
            v[4 * q + 1] = f.y;
            v[4 * q + 2] = f.z;
            v[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kSlotsPerThread; ++j) v[j] = base + j < total ? table[base + j] : absent_f();
    }
}

__global__ void __launch_bounds__(kBlock) count_kernel(const float *table, uint64_t total, uint64_t *blk) {
    __shared__ uint32_t red[kBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kSlotsPerBlock + threadIdx.x * kSlotsPerThread;
    float v[kSlotsPerThread];
    load_slots(table, total, base, v);
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kSlotsPerThread; ++j) c += fbits(v[j]) != kAbsentBits;
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += red[w];
        blk[blockIdx.x] = t;
    }
}

// exclusive scan of nb block counts in place, total in blk[nb] and in
// *total (the lists' end offset, offsets[nv]); one block: each thread sums
// its run of counts, a shuffle scan per wave and one over the 16 wave
// totals (two barriers; the Hillis-Steele form took 20, 10.6 us at C3)
// blk[nb + 1]: a copy of the call's error word (0 without one), so one copy
// brings the stored count and the error bits to the host
__global__ void __launch_bounds__(1024) scan_kernel(uint64_t *blk, int64_t nb, int64_t *total,
                                                    const unsigned long long *err) {
    __shared__ unsigned long long wsum[16];
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b0 = threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    unsigned long long s = 0;
    for (int64_t i = b0; i < b1; ++i) s += blk[i];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    if (wv == 0) {
        const unsigned long long w = lane < 16 ? wsum[lane] : 0ull;
        unsigned long long wi = w;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const unsigned long long t = __shfl_up(wi, o);
            if (lane >= o) wi += t;
        }
        if (lane < 16) wsum[lane] = wi - w;
        if (lane == 15) {
            blk[nb] = wi;
            blk[nb + 1] = err ? *err : 0ull;
            *total = (int64_t)wi;
        }
    }
    __syncthreads();
    uint64_t acc = wsum[wv] + incl - s;
    for (int64_t i = b0; i < b1; ++i) {
        const uint64_t t = blk[i];
        blk[i] = acc;
        acc += t;
    }
}

struct WriteArgs {
    const float *table;
    const uint64_t *blk;
    const uint64_t *tbl_off;
    const int *meta;
    const uint8_t *cand;
    const uint32_t *binom;
    const uint64_t *binom64;  // wide layers (L > kMaxL)
    uint64_t total;
    int nv, S;
    uint64_t *sets;
    float *scores;
    int64_t *offsets;
};

constexpr int kWriteLdsSegs = 2048;  // slab offsets staged in LDS up to this many (vi, L) segments

// Stored slots -> (set, score) lists.  A thread's slots are contiguous, so it
// locates its first slot's (variable, layer) segment and unranks it once;
// every later slot is the colex successor (Gosper's hack, typedefs.h:692-697)
// inside the segment, or the first set (1 << L) - 1 of the next one.
// 8 waves per SIMD (<= 64 VGPRs) and the slab offsets in dynamic LDS sized
// to the call ((nv * S + 1) * 8 bytes, 1.6 KB at C3, instead of a fixed 16 KB):
// the kernel waits on its loads, so resident waves are what it needs.
__global__ void __launch_bounds__(kBlock, 8) write_kernel(WriteArgs a) {
    __shared__ uint32_t pre[kBlock / 64];
    __shared__ uint32_t binom[64 * kBinomK];
    extern __shared__ uint64_t toff_s[];  // (nv * S + 1) entries when nv * S <= kWriteLdsSegs
    __shared__ uint32_t cand_s[64 * 16];  // the candidate lists (64 bytes per variable, nv <= 64)
    const int nseg = a.nv * a.S;
    const bool lds_off = nseg <= kWriteLdsSegs;
    for (int i = threadIdx.x; i < 64 * kBinomK; i += kBlock) binom[i] = a.binom[i];
    for (int i = threadIdx.x; i < a.nv * 16; i += kBlock) cand_s[i] = reinterpret_cast<const uint32_t *>(a.cand)[i];
    const uint8_t *cand = reinterpret_cast<const uint8_t *>(cand_s);
    if (lds_off)
        for (int i = threadIdx.x; i <= nseg; i += kBlock) toff_s[i] = a.tbl_off[i];
    const uint64_t *toff = lds_off ? toff_s : a.tbl_off;
    const uint64_t base = (uint64_t)blockIdx.x * kSlotsPerBlock + threadIdx.x * kSlotsPerThread;
    float vals[kSlotsPerThread];
    load_slots(a.table, a.total, base, vals);
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kSlotsPerThread; ++j) c += fbits(vals[j]) != kAbsentBits;
    // block-wide exclusive prefix of the per-thread counts: wave scan + wave totals
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = c;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) pre[wv] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wv; ++w) wbase += pre[w];
    if (c == 0) return;
    uint64_t pos = a.blk[blockIdx.x] + wbase + incl - c;
    int first = 0;
    while (fbits(vals[first]) == kAbsentBits) ++first;
    uint64_t s0 = base + first;
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (toff[mid] <= s0) lo = mid; else hi = mid;
    }
    int seg = lo;
    int vi = seg / a.S, L = seg % a.S;
    int m = a.meta[vi * 4 + 1];
    uint64_t cm = L <= kMaxL ? unrank_colex(s0 - toff[seg], L, m, binom)
                             : unrank_colex64(s0 - toff[seg], L, m, a.binom64);
    for (int j = first; j < kSlotsPerThread; ++j) {
        const uint64_t s = base + j;
        // the last block's slots past the table hold nothing, and the
        // segment search below must not run past the last offset
        // (toff[nseg] = total): it read toff[nseg + 1]
        if (s >= a.total) break;
        if (j > first) {
            if (s >= toff[seg + 1]) {
                while (s >= toff[seg + 1]) ++seg;
                vi = seg / a.S;
                L = seg % a.S;
                m = a.meta[vi * 4 + 1];
                cm = L ? (~0ull >> (64 - L)) : 0ull;
            } else {
                const uint64_t r = cm + (cm & (0 - cm));
                cm = r | (((r ^ cm) >> 2) >> __builtin_ctzll(cm));
            }
        }
        if (fbits(vals[j]) == kAbsentBits) continue;
        uint64_t gs = 0;
        uint64_t rem = cm;
        while (rem) {
            const int b = __builtin_ctzll(rem);
            rem &= rem - 1;
            gs |= 1ull << cand[vi * 64 + b];
        }
        a.sets[pos] = gs;
        a.scores[pos] = vals[j];
        if (L == 0) a.offsets[vi] = (int64_t)pos;
        ++pos;
    }
}


__global__ void quantize_kernel(const float *in, float *out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < count) out[i] = quantize_score(in[i]);
}

// ScoringFunction::calculateScore's return value for arbitrary (variable,
// parent set) pairs (BIC_OLS.cpp:174-276 via calculateScoreAndBeta, :277-388):
// -float(N ln(RSS/N) + lambda ln(N) |P|), 0 parents -> -0.0f (BIC_OLS.cpp:
// 300-303).  One lane per pair, parents in ascending order (parent_vec), the
// Cholesky in the layer kernels' operation order, so a stored set's value is
// the one ulg_cbic_score stored for it.
#define ULG_CONS 0
#include "cbic_score_sets.inc"
#undef ULG_CONS
#define ULG_CONS 1
#include "cbic_score_sets.inc"
#undef ULG_CONS

// A scoring kernel's type, or with CONS its constrained twin's (*_cons_kernel:
// the call's constraint table and its words after the common arguments); the
// dispatch functions below pick either by the same (layer, phase, variant).
template <bool CONS, class... A>
using TwinFn = std::conditional_t<CONS, void (*)(A..., const uint64_t *, int), void (*)(A...)>;
template <bool CONS>
using LayerFn = TwinFn<CONS, ScoreArgs>;
template <int L, int V, bool CONS, bool NARROW = false>
LayerFn<CONS> pick_phase(int phase) {
    if constexpr (CONS)
        return phase == 0 ? score_layer_cons_kernel<L, 0, V, NARROW> : score_layer_cons_kernel<L, 1, V, NARROW>;
    else return phase == 0 ? score_layer_kernel<L, 0, V, NARROW> : score_layer_kernel<L, 1, V, NARROW>;
}
// variants (ulg_set_option "score_variant"): bit 0 unrolled presence gathers
// (layers <= 6), bit 4 two-pass (settle, queue the rest for a walk launch),
// bit 5 bit-sliced walk, bit 6 subset maxima.  1: one-pass (also the form for
// tables of 2^30 slots or more); 65: one-pass with the subset maxima (the
// small layers of 113); 49: two-pass with the bit-sliced walk (the tests'
// every-set-gathered reference); 113: the same with the subset maxima (the
// default).  Gone after measurement: round 4's per-lane walk forms 17 / 81
// and a variant that walked the open sets inside the scoring kernel (C5 5.05
// against 3.59 ms: a 64-set union tree repeats work a 256-set one shares);
// round 1's loop gathers at every layer, stack-machine recursion,
// decision-only per-lane walk and statistics build.
// narrow: the launch's 32-bit form (CbicPlan::launch_narrow), built where
// CbicPlan::narrow_built says so: the default variant's layers 5 and 6
template <int L, bool CONS>
LayerFn<CONS> pick(int phase, int variant, bool narrow) {
    if constexpr (CbicPlan::narrow_built(L, 241))
        if (narrow && variant == 241) return pick_phase<L, 209, CONS, true>(phase);
    if (narrow) return nullptr;
    switch (variant) {
        case 1: return pick_phase<L, 1, CONS>(phase);
        case 49: return pick_phase<L, 17, CONS>(phase);
        case 65: return pick_phase<L, 65, CONS>(phase);
        case 113: return pick_phase<L, 81, CONS>(phase);
        case 241: return pick_phase<L, 209, CONS>(phase);
        default: return nullptr;
    }
}
using SlicedFn = void (*)(const uint64_t *, const unsigned long long *, float *, float *, uint64_t *, uint64_t,
                         unsigned long long *);
template <int L, int K>
SlicedFn sliced_pick(int phase) {
    return phase == 0 ? walk_sliced_kernel<L, 0, K> : walk_sliced_kernel<L, 1, K>;
}
template <int K>
SlicedFn sliced_fn_k(int L, int phase) {
    switch (L) {
        case 1: return sliced_pick<1, K>(phase);
        case 2: return sliced_pick<2, K>(phase);
        case 3: return sliced_pick<3, K>(phase);
        case 4: return sliced_pick<4, K>(phase);
        case 5: return sliced_pick<5, K>(phase);
        case 6: return sliced_pick<6, K>(phase);
        default: return nullptr;
    }
}
// L = 7, 8 (256 / 512 local subsets): 2 and 1 sets per lane keep each of the
// two vectors at 16 registers (C4: 3.95 -> 2.75 ms per step against the
// per-lane walk_kernel)
SlicedFn sliced_fn_wide(int L, int phase) {
    switch (L) {
        case 7: return sliced_pick<7, 2>(phase);
        case 8: return sliced_pick<8, 1>(phase);
        default: return nullptr;
    }
}
// sets per lane: more sets share one walk of the union tree, fewer give more
// waves to hide the walk's latency
// sets per lane of the bit-sliced walk: 2 up to layer 5, 4 at layer 6
// (rounds 2-4: with the open bits in LDS, 4 / 8 measured 0.558 against 0.547
// ms per C3 bench step over three alternating runs, 4 / 4 0.556, though C5
// calls prefer 4 / 8: 3.15 against 3.36 ms); ULG_SLICED_K=1|2|4|8 (every
// layer) or a,b (layers <= 5, layer 6) overrides for A/B
constexpr int kSlicedKSmall = 2;  // default sets per lane up to layer 5
constexpr int kSlicedK6 = 4;      // ... at layer 6
// A layer-6 launch of fewer than `small` sets (the shares of 4 and 8 ranks,
// where a stream group holds one or two variables) walks one set per lane:
// its few waves then each walk a quarter of the union tree, and the launch
// ends with its longest wave (C3 8-rank share 0.80 -> 0.73 ms; the one-GPU
// launches keep the wide union, best there, `profiles/r4/`).
int sliced_k(int L, uint64_t cnt = ~0ull, uint64_t small = 0, int k6 = kSlicedK6) {
    if (L >= 7) return L == 7 ? 2 : 1;
    // ULG_SLICED_K=a (every layer) or a,b (layers <= 5, layer 6): A/B only
    const char *e = std::getenv("ULG_SLICED_K");
    int k = L <= 5 ? kSlicedKSmall : (cnt < small ? 1 : k6);
    if (e) {
        const char *comma = std::strchr(e, ',');
        k = (L <= 5 || !comma) ? std::atoi(e) : std::atoi(comma + 1);
    }
    return (k == 1 || k == 2 || k == 8) ? k : 4;
}
// queued sets per walk wave
SlicedFn sliced_fn(int L, int phase, int k) {
    if (L >= 7) return sliced_fn_wide(L, phase);
    switch (k) {
        case 1: return sliced_fn_k<1>(L, phase);
        case 2: return sliced_fn_k<2>(L, phase);
        case 4: return sliced_fn_k<4>(L, phase);
        default: return sliced_fn_k<8>(L, phase);
    }
}

using BucketFn = void (*)(const uint64_t *, const uint32_t *, const unsigned int *, float *, float *, uint64_t,
                         unsigned long long *);
template <int L, int KL>
BucketFn bucket_pick(int phase) {
    return phase == 0 ? walk_bucket_kernel<L, 0, KL> : walk_bucket_kernel<L, 1, KL>;
}
// layers 5 and 6; KL = sets per lane of the light keys (2 or 4 at layer 5, 4 or 8 at 6)
BucketFn bucket_fn(int L, int phase, int kl) {
    if (L == 5) return kl >= 4 ? bucket_pick<5, 4>(phase) : bucket_pick<5, 2>(phase);
    if (L == 6) return kl >= 8 ? bucket_pick<6, 8>(phase) : bucket_pick<6, 4>(phase);
    return nullptr;
}

const char *kWalkNames[2][kMaxL + 1] = {
    {"", "walk_1_var0", "walk_2_var0", "walk_3_var0", "walk_4_var0", "walk_5_var0", "walk_6_var0", "walk_7_var0",
     "walk_8_var0"},
    {"", "walk_1_rest", "walk_2_rest", "walk_3_rest", "walk_4_rest", "walk_5_rest", "walk_6_rest", "walk_7_rest",
     "walk_8_rest"}};

template <int LF, bool CONS>
TwinFn<CONS, ScoreArgs, const uint64_t *> small_pick() {
    if constexpr (CONS) return score_small_cons_kernel<LF, 65>;
    else return score_small_kernel<LF, 65>;
}
template <bool CONS>
TwinFn<CONS, ScoreArgs, const uint64_t *> small_kernel(int Lf) {
    switch (Lf) {
        case 1: return small_pick<1, CONS>();
        case 2: return small_pick<2, CONS>();
        case 3: return small_pick<3, CONS>();
        default: return small_pick<4, CONS>();
    }
}

template <bool CONS>
LayerFn<CONS> layer_kernel(int L, int phase, int variant, bool narrow = false) {
    switch (L) {
        case 1: return pick<1, CONS>(phase, variant, narrow);
        case 2: return pick<2, CONS>(phase, variant, narrow);
        case 3: return pick<3, CONS>(phase, variant, narrow);
        case 4: return pick<4, CONS>(phase, variant, narrow);
        case 5: return pick<5, CONS>(phase, variant, narrow);
        case 6: return pick<6, CONS>(phase, variant, narrow);
        case 7: return pick<7, CONS>(phase, variant, narrow);
        case 8: return pick<8, CONS>(phase, variant, narrow);
        default: return nullptr;
    }
}
static_assert(kMaxL == 8, "layer_kernel dispatch covers layers 1..8");

const char *kLayerNames[2][kMaxL + 1] = {
    {"", "score_layer_1_var0", "score_layer_2_var0", "score_layer_3_var0", "score_layer_4_var0",
     "score_layer_5_var0", "score_layer_6_var0", "score_layer_7_var0", "score_layer_8_var0"},
    {"", "score_layer_1_rest", "score_layer_2_rest", "score_layer_3_rest", "score_layer_4_rest",
     "score_layer_5_rest", "score_layer_6_rest", "score_layer_7_rest", "score_layer_8_rest"}};

// ---- the scoring call's launches (host) --------------------------------------
// the call's constraint table on the device (words 0: the unconstrained kernels)
struct ConsTable {
    const uint64_t *dev;
    int words, lds;
};

// What the launch steps of one scoring call share.
struct ScoreCall {
    ulg_ctx *c;
    const ScoreLists &ls;
    const CbicPlan &p;
    ConsTable cons;
    ScoreArgs sa;                  // the fields every layer launch shares
    const uint64_t *d_wk;          // the stream groups' work prefixes (p.group_work()) on the device
    std::vector<hipStream_t> gst;  // each group's stream; group 0 is the context's
    const char *wck;               // ULG_WALK_CLOCK: walk diagnostics (synchronising)
    unsigned long long *errf() const { return p.zero_q ? c->d_qcount.p + p.nqc - 1 : nullptr; }
};

// One launch on stream st under its profiling name; LDS above 64 KiB is asked for first.
template <class Fn, class... A>
int launch_kernel(ulg_ctx *c, Fn fn, dim3 grid, dim3 block, int lds, hipStream_t st, const char *name, A... args) {
    if (lds > 64 * 1024)
        ULG_HIP(c, hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    prof_begin_s(c, name, st);
    hipLaunchKernelGGL(fn, grid, block, (size_t)lds, st, args...);
    prof_end_s(c, st);
    return ULG_OK;
}
// A scoring launch: kernel fn, or under constraints its twin cfn, which takes
// the table and its words after the common arguments and stages the table in
// LDS behind the kernel's own layout.
template <class Fn, class ConsFn, class... A>
int launch_twin(ulg_ctx *c, const ConsTable &ct, Fn fn, ConsFn cfn, dim3 grid, dim3 block, int lds, hipStream_t st,
                const char *name, A... args) {
    if (!ct.words) return launch_kernel(c, fn, grid, block, lds, st, name, args...);
    return launch_kernel(c, cfn, grid, block, align16(lds) + ct.lds, st, name, args..., ct.dev, ct.words);
}

// One stream group's part of a wide layer phase; `bits` is the group's own
// slice of c->d_wbits (p.wslice words), so the groups' walks run concurrently
// on their own streams.
struct WideGroup {
    hipStream_t st;
    const uint64_t *d_work, *h_work;
    uint64_t cnt;
    uint64_t *queue;
    unsigned long long *qc, *scnt;
    uint64_t *bits;
    int *d_hmeta;
    WideArgs wa;
    std::vector<int> hm;  // hi-cover launch metadata (kept until its copy ran)
    uint64_t qn = 0;
    uint32_t *hq = nullptr;      // replays handed to the host (indices into the straggler queue)
    unsigned int *hqc = nullptr;
};

// Launch (L, ph) of `cnt` sets with the prefixes d_work / h_work, on stream
// group g's stream with the group's queue, counter, bitset, hi-cover-metadata
// and host-replay slices.
WideGroup wide_group(const ScoreCall &k, int g, int L, int ph, const uint64_t *d_work, const uint64_t *h_work,
                     uint64_t cnt) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    WideGroup wg;
    wg.st = k.gst[g];
    wg.d_work = d_work;
    wg.h_work = h_work;
    wg.cnt = cnt;
    wg.queue = c->d_wqueue.p + g * p.wqwords;
    wg.qc = c->d_qcount.p + p.seg_slot(g, L, ph);
    wg.scnt = c->d_scount.p + g;
    wg.bits = c->d_wbits.p + (size_t)g * p.wslice;
    wg.d_hmeta = p.hoff.empty() ? nullptr : c->d_hmeta.p + (size_t)g * p.hmeta_stride();
    wg.hq = c->d_hq.p + (size_t)g * std::max<uint64_t>(p.wqwords / 6, 1);
    wg.hqc = c->d_hqc.p + g;
    return wg;
}

// table[pairs[2j]] = pairs[2j + 1] (the bits of a float): the host walks' decisions
__global__ void scatter_decisions_kernel(const uint64_t *pairs, uint32_t cnt, float *table) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < cnt) table[pairs[2 * (uint64_t)j]] = __uint_as_float((uint32_t)pairs[2 * (uint64_t)j + 1]);
}

constexpr uint64_t kHostFewReplays = 64;  // launches of at most this many replays ...
constexpr uint64_t kHostFewBudget = 512;   // ... hand walks to the host after this many iterations

// The replays walk_wide_lds_kernel handed over (more than c->wide_host
// iterations): their fills again into the group's bitset slice, one copy
// back, the walks on host threads, the decisions written into the table.
int host_walks(ulg_ctx *c, WideGroup &G, int L, int ph, int q, uint64_t sn, uint64_t slice,
               unsigned long long *errf) {
    const auto th0 = std::chrono::steady_clock::now();
    unsigned int cnt = 0;
    ULG_HIP(c, hipMemcpyAsync(&cnt, G.hqc, 4, hipMemcpyDeviceToHost, G.st));
    ULG_HIP(c, hipStreamSynchronize(G.st));
    const auto th1 = std::chrono::steady_clock::now();  // the LDS replays are done
    if (cnt == 0) return ULG_OK;
    if (cnt > sn) return set_err(c, ULG_ERR_STATE, "ulg_cbic_score: host walk queue overflow");
    std::vector<uint32_t> idx(cnt);
    std::vector<uint64_t> ent((size_t)3 * sn);
    const uint64_t *sq = G.queue + 3 * G.qn;
    ULG_HIP(c, hipMemcpyAsync(idx.data(), G.hq, (size_t)cnt * 4, hipMemcpyDeviceToHost, G.st));
    ULG_HIP(c, hipMemcpyAsync(ent.data(), sq, ent.size() * 8, hipMemcpyDeviceToHost, G.st));
    ULG_HIP(c, hipStreamSynchronize(G.st));
    const uint64_t nw = ((uint64_t)1 << q) >> 6;
    const uint64_t per = std::max<uint64_t>(1, slice / (2 * nw));
    std::vector<uint64_t> bits;
    std::vector<uint32_t> vals(cnt);
    std::vector<uint64_t> slots(cnt);
    double walk_ms = 0.0, copy_ms = 0.0;
    const auto th2 = std::chrono::steady_clock::now();
    for (uint64_t b0 = 0; b0 < cnt; b0 += per) {
        const uint64_t k = std::min<uint64_t>(per, cnt - b0);
        // this chunk's queue indices (the kernel's list is on the host now)
        ULG_HIP(c, hipMemcpyAsync(G.hq, idx.data() + b0, k * 4, hipMemcpyHostToDevice, G.st));
        prof_begin_s(c, "walk_wide_host_fill", G.st);
        if (ph == 0) strag_fill_global_kernel<0><<<(unsigned)k, 256, 0, G.st>>>(G.wa, sq, G.hq, G.bits);
        else strag_fill_global_kernel<1><<<(unsigned)k, 256, 0, G.st>>>(G.wa, sq, G.hq, G.bits);
        prof_end_s(c, G.st);
        ULG_HIP(c, hipGetLastError());
        bits.resize((size_t)(k * 2 * nw));
        ULG_HIP(c, hipStreamSynchronize(G.st));
        const auto tf0 = std::chrono::steady_clock::now();
        ULG_HIP(c, hipMemcpyAsync(bits.data(), G.bits, bits.size() * 8, hipMemcpyDeviceToHost, G.st));
        ULG_HIP(c, hipStreamSynchronize(G.st));
        copy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count();
        if (const char *dd = std::getenv("ULG_DUMP_HOSTWALK")) {  // diagnostics: the bitsets of the largest ones
            static std::atomic<int> nd{0};
            static const int qmin = std::getenv("ULG_DUMP_HOSTWALK_Q") ? std::atoi(std::getenv("ULG_DUMP_HOSTWALK_Q")) : 15;
            if (q >= qmin && nd < 64) {
                char fn[512];
                std::snprintf(fn, sizeof fn, "%s/hostwalk_%d_L%d_p%d_q%d.bin", dd, nd++, L, ph, q);
                if (FILE *f = std::fopen(fn, "wb")) {
                    std::fwrite(bits.data(), 8, 2 * nw, f);
                    std::fclose(f);
                }
            }
        }
        std::atomic<uint64_t> next{0};
        std::atomic<bool> bad{false};
        auto work = [&]() {
            for (uint64_t j = next++; j < k; j = next++) {
                bool e = false;
                const bool dom = host_walk(L, ph, bits.data() + j * 2 * nw, bits.data() + j * 2 * nw + nw, &e);
                if (e) bad = true;
                const uint64_t *en = ent.data() + 3 * (uint64_t)idx[b0 + j];
                // the stored value is -ts: flip the float's sign bit
                vals[b0 + j] = dom ? kAbsentBits : ((uint32_t)(en[2] >> 32) ^ 0x80000000u);
                slots[b0 + j] = en[0];
            }
        };
        const unsigned nth = (unsigned)std::min<uint64_t>(
            k, std::min((unsigned)c->opt.wide_host_threads, std::max(1u, std::thread::hardware_concurrency())));
        const auto twa = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nth; ++t) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
        walk_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - twa).count();
        if (bad) {
            const unsigned long long one = 1;
            ULG_HIP(c, hipMemcpyAsync(errf, &one, 8, hipMemcpyHostToDevice, G.st));
        }
    }
    // the decisions: one copy of (slot, value) pairs into the group's bitset
    // slice (free again), then one scatter launch
    const auto tw1 = std::chrono::steady_clock::now();
    std::vector<uint64_t> pairs((size_t)2 * cnt);
    for (unsigned j = 0; j < cnt; ++j) {
        pairs[2 * (size_t)j] = slots[j];
        pairs[2 * (size_t)j + 1] = vals[j];
    }
    ULG_HIP(c, hipMemcpyAsync(G.bits, pairs.data(), pairs.size() * 8, hipMemcpyHostToDevice, G.st));
    scatter_decisions_kernel<<<(cnt + 255) / 256, 256, 0, G.st>>>(G.bits, cnt, G.wa.table);
    ULG_HIP(c, hipGetLastError());
    ULG_HIP(c, hipStreamSynchronize(G.st));  // pairs is about to go
    static const bool wstat = std::getenv("ULG_WALK_STATS") != nullptr;
    if (wstat) {
        const auto tw2 = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::milli>(b - a).count();
        };
        std::fprintf(stderr,
                     "walk_host_stats L=%d phase=%d q=%d handed=%u of %llu ms=%.2f (gpu replays %.2f, lists %.2f, "
                     "bits copy %.2f, walks %.2f, write %.2f)\n",
                     L, ph, q, cnt, (unsigned long long)sn, ms(th0, tw2), ms(th0, th1), ms(th1, th2), copy_ms, walk_ms,
                     ms(tw1, tw2));
    }
    return ULG_OK;
}

// A group's wide scoring launch; its queue length follows into *pin.
int wide_score(const ScoreCall &k, int L, int ph, WideGroup &G, unsigned long long *pin) {
    ulg_ctx *c = k.c;
    WideArgs &wa = G.wa;
    wa.gram = c->gram.p;
    wa.binom = c->d_binom64.p;
    wa.cand = c->d_cand.p;
    wa.meta = c->d_meta.p;
    wa.tbl_off = c->d_tbl_off.p;
    wa.work = G.d_work;
    wa.table = c->table.p;
    wa.queue = G.queue;
    wa.qcount = G.qc;
    wa.hmax = nullptr;
    wa.pval = nullptr;
    wa.hoff = nullptr;
    wa.reduced = c->opt.wide_reduced;
    wa.N = (double)c->N;
    wa.pen = c->pen;
    wa.n = c->n;
    wa.nv = k.ls.nv;
    wa.S = k.ls.S;
    wa.L = L;
    const uint64_t blocks = (G.cnt + kBlock - 1) / kBlock;
    if (int rc = launch_twin(c, k.cons, wide_fn(L, ph), wide_cons_fn(L, ph), dim3((unsigned)blocks), dim3(kBlock),
                             c->n * c->n * 8, G.st, ph == 0 ? "score_wide_var0" : "score_wide_rest", G.wa))
        return rc;
    ULG_HIP(c, hipGetLastError());
    ULG_HIP(c, hipMemcpyAsync(pin, G.qc, 8, hipMemcpyDeviceToHost, G.st));
    return ULG_OK;
}

// The hi-cover tables of this launch's variables, built on the group's
// stream: [lvars][tile prefix][one block prefix per strided pass], one upload.
int wide_hicover(const ScoreCall &k, int L, int ph, WideGroup &G) {
    ulg_ctx *c = k.c;
    const std::vector<int> &meta = k.p.meta;
    const int nv = k.ls.nv;
    hipStream_t st = G.st;
    WideArgs &wa = G.wa;
    const int S = k.ls.S, kmax = k.ls.kmax;
    std::vector<int> lv;
    for (int i = 0; i < nv; ++i)
        if (G.h_work[i + 1] > G.h_work[i] && k.p.hoff[i] != ~0ull) lv.push_back(i);
    const int nl = (int)lv.size();
    if (nl == 0) return ULG_OK;
    int maxm = 0;
    for (int vi : lv) maxm = std::max(maxm, meta[vi * 4 + 1]);
    const int passes = maxm > kHiTileBits ? (maxm - kHiTileBits + kHiGroup - 1) / kHiGroup : 0;
    std::vector<int> &hm = G.hm;
    hm.assign((size_t)nl + (size_t)(nl + 1) * (1 + passes), 0);
    for (int i = 0; i < nl; ++i) hm[i] = lv[i];
    int *tp = hm.data() + nl;
    for (int i = 0; i < nl; ++i) {
        const int m = meta[lv[i] * 4 + 1];
        tp[i + 1] = tp[i] + (m <= kHiTileBits ? 1 : 1 << (m - kHiTileBits));
    }
    for (int pp = 0; pp < passes; ++pp) {
        int *bp = tp + (size_t)(nl + 1) * (1 + pp);
        const int bit_lo = kHiTileBits + pp * kHiGroup;
        for (int i = 0; i < nl; ++i) {
            const int m = meta[lv[i] * 4 + 1];
            const int Gb = std::min(kHiGroup, m - bit_lo);
            bp[i + 1] = bp[i] + (Gb > 0 ? (int)(((1ull << (m - Gb)) + 255) / 256) : 0);
        }
    }
    ULG_HIP(c, hipMemcpyAsync(G.d_hmeta, hm.data(), hm.size() * 4, hipMemcpyHostToDevice, st));
    HiArgs ha{G.d_hmeta, G.d_hmeta + nl, nl, c->d_meta.p, c->d_tbl_off.p, c->table.p, c->d_binom64.p,
              c->d_hmax.p, c->d_hmax.p + c->hmax_half, c->d_hoff.p, S, L, kmax, 0};
    prof_begin_s(c, "wide_hicover", st);
    if (ph == 0) hikey_tile_kernel<0><<<tp[nl], 1024, 0, st>>>(ha);
    else hikey_tile_kernel<1><<<tp[nl], 1024, 0, st>>>(ha);
    for (int pp = 0; pp < passes; ++pp) {
        ha.prefix = G.d_hmeta + nl + (size_t)(nl + 1) * (1 + pp);
        ha.bit_lo = kHiTileBits + pp * kHiGroup;
        const int nb = tp[(size_t)(nl + 1) * (1 + pp) + nl];
        if (nb > 0) hikey_strided_kernel<<<nb, 256, 0, st>>>(ha);
    }
    prof_end_s(c, st);
    ULG_HIP(c, hipGetLastError());
    wa.hmax = c->d_hmax.p;
    wa.pval = c->d_hmax.p + c->hmax_half;
    wa.hoff = c->d_hoff.p;
    return ULG_OK;
}

// The walks of the sets a group's scoring launch queued, in chunks whose
// checked bitsets (2^q bits per walking set, q = L when P holds variable 0,
// else L + 1) fit the group's slice.  budget: the steps after which a walk
// moves to the LDS replays (0: never); their count follows into *pin_long.
int wide_walks(const ScoreCall &k, int L, int ph, WideGroup &G, uint64_t &budget, unsigned long long *pin_long) {
    ulg_ctx *c = k.c;
    static const bool wstat = std::getenv("ULG_WALK_STATS") != nullptr;  // diagnostics: synchronises
    const int q = ph == 0 ? L : L + 1;
    const WideWalkFn wf = wide_walk_fn(L, ph);
    const uint64_t wpl = q <= 6 ? 1ull : (1ull << (q - 6));
    hipStream_t st = G.st;
    WideArgs &wa = G.wa;
    const uint64_t per = std::max<uint64_t>(1, std::min<uint64_t>(G.qn, k.p.wslice / wpl));  // the slice holds >= wpl
    unsigned long long *ws = nullptr;
    if (wstat) {
        int rc2;
        if ((rc2 = ensure(c, c->d_stats, 16))) return rc2;
        ws = c->d_stats.p;
        ULG_HIP(c, hipStreamSynchronize(st));
        ULG_HIP(c, hipMemsetAsync(ws, 0, 64, st));
    }
    // long walks move to the LDS kernel (reduced walks with hi-cover tables only)
    budget = (wa.hoff && wa.reduced && q <= kStragQMax && c->opt.wide_lds)
                     ? (c->opt.wide_lds == 2 ? 1 : strag_budget())
                     : 0;
    uint64_t *sq = G.queue + 3 * G.qn;  // straggler queue after this launch's entries (the queue has room)
    if (budget) ULG_HIP(c, hipMemsetAsync(G.scnt, 0, 8, st));
    const auto tw0 = std::chrono::steady_clock::now();
    for (uint64_t base = 0; base < G.qn; base += per) {
        const uint64_t nk = std::min<uint64_t>(per, G.qn - base);
        ULG_HIP(c, hipMemsetAsync(G.bits, 0, (size_t)(nk * wpl * 8), st));
        prof_begin_s(c, ph == 0 ? "walk_wide_var0" : "walk_wide_rest", st);
        hipLaunchKernelGGL(wf, dim3((unsigned)((nk + 63) / 64)), dim3(64), 0, st, wa, base, base + nk, G.bits, wpl,
                           k.errf(), ws, budget, sq, G.scnt);
        prof_end_s(c, st);
        ULG_HIP(c, hipGetLastError());
    }
    if (budget) ULG_HIP(c, hipMemcpyAsync(pin_long, G.scnt, 8, hipMemcpyDeviceToHost, st));
    if (wstat) {
        unsigned long long h[4];
        ULG_HIP(c, hipMemcpyAsync(h, ws, 32, hipMemcpyDeviceToHost, st));
        ULG_HIP(c, hipStreamSynchronize(st));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
        std::fprintf(stderr,
                     "walk_stats L=%d phase=%d queued=%llu walks=%llu steps=%llu max=%llu over2^20=%llu "
                     "launch_ms=%.1f\n",
                     L, ph, (unsigned long long)G.qn, h[0], h[1], h[2], h[3], ms);
    }
    return ULG_OK;
}

// A group's sn long walks, replayed with their bitsets in LDS; the longest
// of those finish on host threads (host_walks).
int wide_lds_replays(const ScoreCall &k, int L, int ph, WideGroup &G, unsigned long long sn) {
    ulg_ctx *c = k.c;
    static const bool wstat = std::getenv("ULG_WALK_STATS") != nullptr;
    const int q = ph == 0 ? L : L + 1;
    const uint64_t slice = k.p.wslice;
    unsigned long long *errf = k.errf();
    // skip bitset in LDS; the hi bitset too up to q = kStragHiLdsQ, else in
    // this group's checked-bitset slice (free once its walks are done)
    const bool hl = q <= kStragHiLdsQ;
    const uint64_t nw = ((uint64_t)1 << q) >> 6;
    const size_t lds = (size_t)(hl ? 2 : 1) * nw * 8 + 64 * 8 + 64;  // bitsets, xlow, lc
    using LdsFn = void (*)(WideArgs, const uint64_t *, uint64_t *, unsigned long long *, unsigned long long *,
                           uint64_t, uint32_t *, unsigned int *, uint32_t);
    const LdsFn kf = ph == 0 ? (hl ? walk_wide_lds_kernel<0, true> : walk_wide_lds_kernel<0, false>)
                             : (hl ? walk_wide_lds_kernel<1, true> : walk_wide_lds_kernel<1, false>);
    ULG_HIP(c, hipFuncSetAttribute((const void *)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const uint64_t per = hl ? sn : std::max<uint64_t>(1, slice / nw);
    unsigned long long *ws = wstat ? c->d_stats.p : nullptr;
    if (wstat) ULG_HIP(c, hipMemsetAsync(ws, 0, 128, G.st));
    const auto tl0 = std::chrono::steady_clock::now();
    // walks past this many iterations finish on the host; with few
    // replays in the launch the host takes them sooner (it runs them in
    // parallel threads, while the GPU's launch time is its longest walk)
    // Host threads take the long walks only of launches with few replays
    // (wide_host_max): with thousands of long walks (C1 at lambda 0.5) a
    // few host threads would queue them behind each other while the GPU
    // runs them all at once (C1 10.7 s GPU-only against 32 s with every
    // launch handing over).
    const uint64_t hbud = sn > c->opt.wide_host_max ? 0
                          : sn <= kHostFewReplays ? std::min<uint64_t>(c->opt.wide_host_iters, kHostFewBudget)
                                                  : c->opt.wide_host_iters;
    // ... and so do launches of few replays over 2^q >= 2^wide_host_q
    // local subsets: at the top layers of the largest candidate sets
    // nearly every replay outlives the LDS budget anyway (C4 v = 23:
    // L >= 15 hands over 13 of 14, 13 of 15, 1 of 1), so its LDS phase is
    // pure latency
    if (hbud && (sn <= c->opt.wide_host_first || (c->opt.wide_host_q > 0 && q >= c->opt.wide_host_q && sn <= 128))) {
        // so few replays that the host takes them all at once: no GPU
        // replay phase (its length is its longest walk's), straight to
        // the fills, the copy and the host threads
        std::vector<uint32_t> all((size_t)sn);
        for (uint32_t j = 0; j < (uint32_t)sn; ++j) all[j] = j;
        const unsigned int n32 = (unsigned int)sn;
        ULG_HIP(c, hipMemcpyAsync(G.hq, all.data(), all.size() * 4, hipMemcpyHostToDevice, G.st));
        ULG_HIP(c, hipMemcpyAsync(G.hqc, &n32, 4, hipMemcpyHostToDevice, G.st));
        int rc2;
        if ((rc2 = host_walks(c, G, L, ph, q, sn, slice, errf))) return rc2;
        return ULG_OK;
    }
    if (hbud) ULG_HIP(c, hipMemsetAsync(G.hqc, 0, 4, G.st));
    for (uint64_t base = 0; base < sn; base += per) {
        const uint64_t nk = std::min<uint64_t>(per, sn - base);
        prof_begin_s(c, "walk_wide_lds", G.st);
        // many short replays: one wave per block, so more walks run at once
        // (the walk is one wave's; waves 1-3 only speed up the fill)
        const unsigned th = sn >= kStragWide ? 64u : (unsigned)kStragThreads;
        hipLaunchKernelGGL(kf, dim3((unsigned)nk), dim3(th), lds, G.st, G.wa,
                           G.queue + 3 * (G.qn + base), G.bits, errf, ws, hbud, G.hq, G.hqc, (uint32_t)base);
        prof_end_s(c, G.st);
        ULG_HIP(c, hipGetLastError());
    }
    if (hbud) {
        int rc2;
        if ((rc2 = host_walks(c, G, L, ph, q, sn, slice, errf))) return rc2;
    }
    if (wstat) {
        unsigned long long h[16];
        ULG_HIP(c, hipMemcpyAsync(h, ws, 128, hipMemcpyDeviceToHost, G.st));
        ULG_HIP(c, hipStreamSynchronize(G.st));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count();
        std::fprintf(stderr,
                     "walk_lds_stats L=%d phase=%d q=%d replays=%llu iters=%llu max=%llu fill_max_us=%.1f "
                     "walk_max_us=%.1f launch_ms=%.1f\n",
                     L, ph, q, h[4], h[5], h[6], h[7] / 100.0, h[8] / 100.0, ms);
    }
    return ULG_OK;
}

// One wide layer phase for every stream group, in stages so the groups stay
// concurrent: every group's scoring launch; the queue lengths (one D2H each
// into pinned memory, then the syncs -- the launches already overlap); every
// group's hi-cover tables and walks; the long-walk counts; the LDS replays.
// pin: 2 * gs.size() pinned words of the caller's (queue lengths, long-walk counts)
int score_wide_groups(const ScoreCall &k, int L, int ph, std::vector<WideGroup> &gs, unsigned long long *pin) {
    ulg_ctx *c = k.c;
    const int ng = (int)gs.size();
    int rc;
    for (int gi = 0; gi < ng; ++gi)
        if ((rc = wide_score(k, L, ph, gs[gi], pin + gi))) return rc;
    for (int gi = 0; gi < ng; ++gi) {
        ULG_HIP(c, hipStreamSynchronize(gs[gi].st));
        gs[gi].qn = pin[gi];
    }
    std::vector<uint64_t> budget(ng, 0);
    for (int gi = 0; gi < ng; ++gi) {
        if (gs[gi].qn == 0) continue;
        if (gs[gi].d_hmeta && (rc = wide_hicover(k, L, ph, gs[gi]))) return rc;
        if ((rc = wide_walks(k, L, ph, gs[gi], budget[gi], pin + ng + gi))) return rc;
    }
    for (int gi = 0; gi < ng; ++gi) {
        if (gs[gi].qn == 0 || !budget[gi]) continue;
        ULG_HIP(c, hipStreamSynchronize(gs[gi].st));
        if (pin[ng + gi] && (rc = wide_lds_replays(k, L, ph, gs[gi], pin[ng + gi]))) return rc;
    }
    // the hi-cover metadata vectors must outlive their copies
    for (int gi = 0; gi < ng; ++gi)
        if (!gs[gi].hm.empty()) ULG_HIP(c, hipStreamSynchronize(gs[gi].st));
    return ULG_OK;
}


// ULG_WALK_CLOCK diagnostics: every walk wave's start / end clock and its
// union points (steps) into <dir>/sliced_L<L>_p<phase>.bin (synchronising)
int dump_walk_clock(ulg_ctx *c, hipStream_t st, uint64_t sb, const char *dir, int L, int ph) {
    std::vector<uint64_t> hw((size_t)3 * sb);
    ULG_HIP(c, hipMemcpyAsync(hw.data(), c->d_dump.p, hw.size() * 8, hipMemcpyDeviceToHost, st));
    ULG_HIP(c, hipStreamSynchronize(st));
    char fn[512];
    std::snprintf(fn, sizeof fn, "%s/sliced_L%d_p%d.bin", dir, L, ph);
    if (FILE *f = std::fopen(fn, "wb")) {
        std::fwrite(hw.data(), 8, hw.size(), f);
        std::fclose(f);
    }
    return ULG_OK;
}

// Diagnostics (ULG_WALK_CLOCK with ULG_WALK_QUEUE_DUMP, after a layer's walk
// launch): the walk queue of that launch, compacted, with each entry's
// decision as the walk left it in the table -- scripts/walk_sched_study.cpp
// replays the walks offline.  File: nseg, W, then per segment its count,
// count x (1 + 2W) entry words and count decision words (the table's bits at
// the entry's slot).
int dump_walk_queue(ulg_ctx *c, hipStream_t st, const uint64_t *queue, const unsigned long long *qc,
                           uint64_t nseg, int W, uint64_t nslots, const char *dir, int L, int ph) {
    std::vector<unsigned long long> cnt(nseg * kSegStride);
    ULG_HIP(c, hipMemcpyAsync(cnt.data(), qc, cnt.size() * 8, hipMemcpyDeviceToHost, st));
    ULG_HIP(c, hipStreamSynchronize(st));
    char fn[512];
    std::snprintf(fn, sizeof fn, "%s/queue_L%d_p%d.bin", dir, L, ph);
    FILE *f = std::fopen(fn, "wb");
    if (!f) return ULG_OK;
    const uint64_t hdr[2] = {nseg, (uint64_t)W};
    std::fwrite(hdr, 8, 2, f);
    const uint64_t ew = 1 + 2 * (uint64_t)W;
    std::vector<uint32_t> tab((size_t)nslots);
    ULG_HIP(c, hipMemcpyAsync(tab.data(), reinterpret_cast<const uint32_t *>(c->table.p), tab.size() * 4,
                              hipMemcpyDeviceToHost, st));
    ULG_HIP(c, hipStreamSynchronize(st));
    for (uint64_t s = 0; s < nseg; ++s) {
        const uint64_t n = std::min<uint64_t>(cnt[s * kSegStride], kSegEntries);
        std::vector<uint64_t> e(n * ew);
        std::vector<uint32_t> d(n);
        if (n) {
            ULG_HIP(c, hipMemcpyAsync(e.data(), queue + s * kSegEntries * ew, e.size() * 8, hipMemcpyDeviceToHost, st));
            ULG_HIP(c, hipStreamSynchronize(st));
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t slot = (uint32_t)e[i * ew];
                d[i] = slot < tab.size() ? tab[slot] : 0u;
            }
        }
        std::fwrite(&n, 8, 1, f);
        std::fwrite(e.data(), 8, e.size(), f);
        std::fwrite(d.data(), 4, d.size(), f);
    }
    std::fclose(f);
    return ULG_OK;
}

// The call's error word (kErr* bits) as a status.
int call_error(ulg_ctx *c, unsigned long long w) {
    c->last_err_word = w;
    if (w & kErrWide)
        return set_err(c, ULG_ERR_UNSUPPORTED,
                       "ulg_cbic_score: a find_best_subset_score walk in a wide layer exceeded its cap (2^30 steps "
                       "in walk_wide_kernel, 2^32 iterations or 24 frames in the LDS / host replay)");
    if (w & (kErrQueue | kErrSlot))
        return set_err(c, ULG_ERR_STATE,
                       (w & kErrQueue) ? "ulg_cbic_score: a walk-queue segment overflowed (internal sizing error)"
                                       : "ulg_cbic_score: a walk entry named a slot past the call's table");
    return ULG_OK;
}

// The wide layers of every variable that reaches them, one variable per task
// (p.pool_order) on G host threads; thread t drives stream gst[t] with stream
// group t's queue, counter, bitset and hi-cover-metadata slices.  Results are
// the grouped form's (a variable's decisions read only its own slabs).
int wide_pool(const ScoreCall &k) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    const int G = p.G;
    // every stream's earlier layers first (the slabs the wide layers read)
    for (int g = 0; g < G; ++g) ULG_HIP(c, hipStreamSynchronize(k.gst[g]));
    int rc;
    if ((rc = upload(c, c->d_vwork, c->mir_vwork, p.vw))) return rc;
    ULG_HIP(c, hipStreamSynchronize(c->stream));  // the other threads' streams read it next
    std::atomic<size_t> next{0};
    std::vector<int> rcs(G, ULG_OK);
    auto run = [&](int t) {
        if (hipSetDevice(c->device) != hipSuccess) {
            rcs[t] = set_err(c, ULG_ERR_HIP, "hipSetDevice failed in a wide-layer thread");
            return;
        }
        for (size_t task = next++; task < p.pool_order.size(); task = next++) {
            const int top = std::min(k.ls.mv[p.pool_order[task]], k.ls.max_parents);
            for (int L = kMaxL + 1; L <= top; ++L)
                for (int ph = 0; ph < 2; ++ph) {
                    const size_t wo = task * p.wstride + ((size_t)L * 2 + ph) * (p.nv + 1);
                    const uint64_t cnt = p.vw[wo + p.nv];
                    if (cnt == 0) continue;
                    std::vector<WideGroup> one{wide_group(k, t, L, ph, c->d_vwork.p + wo, p.vw.data() + wo, cnt)};
                    // this slot's counter served the previous variable's launch
                    if (hipMemsetAsync(one[0].qc, 0, 8, one[0].st) != hipSuccess) {
                        rcs[t] = set_err(c, ULG_ERR_HIP, "hipMemsetAsync failed in a wide-layer thread");
                        return;
                    }
                    const int r = score_wide_groups(k, L, ph, one, c->wide_pinned.p + 2 * t);
                    if (r) {
                        rcs[t] = r;
                        next = p.pool_order.size();  // the other threads stop at their next task
                        return;
                    }
                }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < G; ++t) th.emplace_back(run, t);
    run(0);
    for (auto &x : th) x.join();
    for (int r : rcs)
        if (r) return r;
    return ULG_OK;
}

// A wide layer phase in grouped form: every stream group's part, staged together.
int launch_wide_grouped(const ScoreCall &k, int L, int ph) {
    const CbicPlan &p = k.p;
    std::vector<WideGroup> wide;
    for (int g = 0; g < p.G; ++g) {
        const uint64_t cnt = p.launch_count(g, L, ph);
        if (cnt == 0) continue;
        if ((cnt + kBlock - 1) / kBlock > 0x7fffffffull)
            return set_err(k.c, ULG_ERR_UNSUPPORTED, "ulg_cbic_score: layer too large");
        const size_t wo = p.work_offset(g, L, ph);
        wide.push_back(wide_group(k, g, L, ph, k.d_wk + wo, p.group_work().data() + wo, cnt));
    }
    return wide.empty() ? ULG_OK : score_wide_groups(k, L, ph, wide, k.c->wide_pinned.p);
}

// The call's first launch: the empty sets' slots, and the queue counters zeroed.
int launch_prologue(const ScoreCall &k) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    const uint64_t nqc = p.zero_q ? p.nqc : 0;
    const uint64_t nz = std::max<uint64_t>((uint64_t)p.nv, std::max<uint64_t>(nqc, p.nqseg));
    const dim3 grid((unsigned)((nz + 255) / 256)), block(256);
    unsigned long long *qcount = p.zero_q ? c->d_qcount.p : nullptr, *qseg = p.zero_q ? c->d_qseg.p : nullptr;
    // the twin takes (table, n) where the scoring twins take (table, words)
    if (k.cons.words)
        return launch_kernel(c, call_prologue_cons_kernel, grid, block, 0, c->stream, "call_prologue", c->d_tbl_off.p,
                             p.nv, k.ls.S, c->table.p, qcount, nqc, qseg, p.nqseg, k.cons.dev, k.ls.n);
    return launch_kernel(c, call_prologue_kernel, grid, block, 0, c->stream, "call_prologue", c->d_tbl_off.p, p.nv,
                         k.ls.S, c->table.p, qcount, nqc, qseg, p.nqseg);
}

// The launch image of layer launch (g, L, ph), when the call built one.
void set_image(const ScoreCall &k, ScoreArgs &sa, int g, int L, int ph) {
    const int64_t at = k.p.image_offset(g, L, ph);
    sa.image = at < 0 ? nullptr : reinterpret_cast<const uint4 *>(k.c->d_image.p + at);
    sa.image16 = at < 0 ? 0 : k.p.image_bytes(k.ls, L) / 16;
}

// A small layer phase (L <= p.Ls) on the context stream, one-pass over all
// variables; layers <= p.Lf run together in one fused launch, sent at (1, 0).
int launch_small(const ScoreCall &k, int L, int ph) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    const int n = k.ls.n, nv = p.nv, S = k.ls.S;
    ScoreArgs ss = k.sa;
    if (L <= p.Lf) {
        if (L != 1 || ph != 0) return ULG_OK;
        ss.hsub_out = p.Lf < p.kmax;  // layer Lf's phase 1 maxima: read only by a layer above
        return launch_twin(c, k.cons, small_kernel<false>(p.Lf), small_kernel<true>(p.Lf), dim3((unsigned)nv),
                           dim3(kFusedThreads), lds_layout(n, nv, S, p.Lf, 65).total, c->stream, "score_small_fused",
                           ss, (const uint64_t *)c->d_work.p);
    }
    const size_t wo = p.work_offset(0, L, ph);
    const uint64_t cnt = p.work[wo + nv];
    if (cnt == 0) return ULG_OK;
    ss.work = c->d_work.p + wo;
    ss.total = cnt;
    ss.lut_off = p.lut_any ? c->d_lutoff.p + p.lut_offset(L, ph) : nullptr;
    set_image(k, ss, 0, L, ph);
    ss.hsub_out = !(L == p.kmax && ph == 1);
    return launch_twin(c, k.cons, layer_kernel<false>(L, ph, p.vsmall), layer_kernel<true>(L, ph, p.vsmall),
                       dim3((unsigned)((cnt + kBlock - 1) / kBlock)), dim3(kBlock),
                       lds_layout(n, nv, S, L, p.vsmall).total, c->stream, kLayerNames[ph][L], ss);
}

// The bucketed walk of an unrolled launch's queue (layers 5 and 6): a
// counting sort of the queue by walk key, then the table's waves.  The
// profiled walk time includes the sort (count + scatter).
int walk_bucketed(const ScoreCall &k, int g, int L, int ph, const ScoreArgs &sa, uint64_t blocks, int wk) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    hipStream_t st = k.gst[g];
    const unsigned long long *qc = sa.qcount;
    const uint64_t nseg = seg_count(blocks);
    const int kl = L == 6 ? (wk >= 8 ? 8 : 4) : (wk >= 4 ? 4 : 2);
    uint32_t *kbase = c->d_qoffs.p + (size_t)g * kBucketMax * p.nseg_max;
    uint32_t *sidx = c->d_qsidx.p + (size_t)g * p.qcap;
    uint32_t *qaux = c->d_qaux.p + (size_t)g * p.qcap;
    const unsigned int *hdr = reinterpret_cast<const unsigned int *>(qc + nseg * kSegStride);
    prof_begin_s(c, kWalkNames[ph][L], st);
    walk_bucket_count_kernel<<<(unsigned)((nseg + kBucketSegs - 1) / kBucketSegs), 256, 0, st>>>(
        qc, (uint32_t)nseg, L, sa.qkey, qaux, kbase);
    const uint64_t items = nseg * (kSegEntries / 256);
    walk_bucket_scatter_kernel<<<(unsigned)std::min<uint64_t>(items, 2048), 256, 0, st>>>(qc, qaux, kbase,
                                                                                          (uint32_t)nseg, L, sidx);
    hipLaunchKernelGGL(bucket_fn(L, ph, kl), dim3((unsigned)std::min<uint64_t>(p.wave_cap, 4096)), dim3(64), 0, st,
                       (const uint64_t *)sa.queue, (const uint32_t *)sidx, hdr, c->table.p,
                       sa.hsub_out ? sa.hsub : nullptr, k.ls.total_slots, sa.err);
    prof_end_s(c, st);
    return ULG_OK;
}

// The bit-sliced walk of an unrolled launch's queue in queue order: one wave
// per (queue segment, chunk of 64 * K entries).
int walk_sliced(const ScoreCall &k, int g, int L, int ph, const ScoreArgs &sa, uint64_t blocks, int wk) {
    ulg_ctx *c = k.c;
    hipStream_t st = k.gst[g];
    const char *wck = k.wck;
    const int kk = L == 7 ? 2 : (L == 8 ? 1 : wk);
    const uint64_t per = 64ull * (uint64_t)kk;
    const uint64_t sb = seg_count(blocks) * ((kSegEntries + per - 1) / per);
    int rc;
    if (wck && (rc = ensure(c, c->d_dump, (size_t)3 * sb))) return rc;
    if (wck) ULG_HIP(c, hipMemsetAsync(c->d_dump.p, 0, 24 * sb, st));
    prof_begin_s(c, kWalkNames[ph][L], st);
    hipLaunchKernelGGL(sliced_fn(L, ph, wk), dim3((unsigned)sb), dim3(64), 0, st, sa.queue, sa.qcount, c->table.p,
                       sa.hsub_out ? sa.hsub : nullptr, wck ? c->d_dump.p : nullptr, k.ls.total_slots, sa.err);
    prof_end_s(c, st);
    if (wck && (rc = dump_walk_clock(c, st, sb, wck, L, ph))) return rc;
    if (wck && std::getenv("ULG_WALK_QUEUE_DUMP") &&
        (rc = dump_walk_queue(c, st, sa.queue, sa.qcount, seg_count(blocks), bits_words(L), k.ls.total_slots, wck, L,
                              ph)))
        return rc;
    return ULG_OK;
}

// An unrolled layer phase of stream group g: its scoring launch, then (the
// two-pass variants) the walk of the undecided lanes it queued, densely
// packed, in bucketed or queue order.
int launch_unrolled(const ScoreCall &k, int g, int L, int ph) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    const uint64_t cnt = p.launch_count(g, L, ph);
    if (cnt == 0) return ULG_OK;
    const uint64_t blocks = (cnt + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_cbic_score: layer too large");
    const bool two_pass = (p.variant & 16) != 0;
    const bool bk = p.bucket && (L == 5 || L == 6);
    ScoreArgs sa = k.sa;
    sa.work = k.d_wk + p.work_offset(g, L, ph);
    sa.total = cnt;
    sa.lut_off = p.lut_any ? c->d_lutoff.p + p.lut_offset(L, ph) : nullptr;
    set_image(k, sa, g, L, ph);
    sa.queue = two_pass ? c->d_queue.p + (size_t)g * p.qwords : nullptr;
    sa.qcount = two_pass ? c->d_qseg.p + p.segoff[p.seg_slot(g, L, ph)] : nullptr;
    sa.qkey = bk ? c->d_qkey.p + (size_t)g * p.qcap : nullptr;
    // nothing reads the subset maxima of the top layer's second phase
    sa.hsub_out = !(L == p.kmax && ph == 1);
    const bool nw = p.launch_narrow(g, L, ph);
    if (nw && !layer_kernel<false>(L, ph, p.variant, true))
        return set_err(c, ULG_ERR_STATE, "ulg_cbic_score: no narrow kernel for a launch planned narrow");
    int rc;
    if ((rc = launch_twin(c, k.cons, layer_kernel<false>(L, ph, p.variant, nw), layer_kernel<true>(L, ph, p.variant, nw),
                          dim3((unsigned)blocks), dim3(kBlock), lds_layout(k.ls.n, p.nv, k.ls.S, L, p.variant).total,
                          k.gst[g], kLayerNames[ph][L], sa)))
        return rc;
    if (!two_pass) return ULG_OK;
    const int wk = sliced_k(L, cnt, (uint64_t)c->opt.walk_small_sets, c->opt.walk_k6);
    if (bk) return walk_bucketed(k, g, L, ph, sa, blocks, wk);
    if ((p.variant & 32) && sliced_fn(L, ph, wk)) return walk_sliced(k, g, L, ph, sa, blocks, wk);
    return ULG_OK;
}

// Every layer's launches in order; done_L: the last complete layer (below
// kmax when the -r budget ran out).  Small layers on the context stream, then
// the fork: the side streams start after the uploads / prologue / small
// layers, and the compaction on the context stream waits for every group.
int launch_layers(const ScoreCall &k, int &done_L) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    const int G = p.G, kmax = p.kmax;
    // -r (score_calculator.cpp:33-52,78): checked after every complete layer
    const auto t_call = std::chrono::steady_clock::now();
    int rc;
    bool forked = false;
    done_L = kmax;
    bool pooled = false;
    for (int L = 1; L <= kmax && !pooled; ++L) {
        for (int ph = 0; ph < 2; ++ph) {
            if (L <= p.Ls) {
                if ((rc = launch_small(k, L, ph))) return rc;
                continue;
            }
            if (G > 1 && !forked) {
                ULG_HIP(c, hipEventRecord(c->sync_events[0], c->stream));
                for (int g = 1; g < G; ++g) ULG_HIP(c, hipStreamWaitEvent(k.gst[g], c->sync_events[0], 0));
                forked = true;
            }
            if (L > kMaxL && p.use_pool) {  // the pool runs every wide layer
                if ((rc = wide_pool(k))) return rc;
                pooled = true;
                break;
            }
            if (L > kMaxL) {
                if ((rc = launch_wide_grouped(k, L, ph))) return rc;
                continue;
            }
            for (int g = 0; g < G; ++g)
                if ((rc = launch_unrolled(k, g, L, ph))) return rc;
        }
        if (c->opt.time_limit_ms > 0 && L < kmax) {
            for (int g = 0; g < (forked ? G : 1); ++g) ULG_HIP(c, hipStreamSynchronize(k.gst[g]));
            const double ms =
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
            if (ms > (double)c->opt.time_limit_ms) {
                done_L = L;
                c->out_of_time = 1;
                break;
            }
        }
    }
    for (int g = 1; g < G && forked; ++g) {
        ULG_HIP(c, hipEventRecord(c->sync_events[g], k.gst[g]));
        ULG_HIP(c, hipStreamWaitEvent(c->stream, c->sync_events[g], 0));
    }
    ULG_HIP(c, hipGetLastError());
    return ULG_OK;
}

uint64_t dbits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}

}  // namespace

extern "C" {

int ulg_cbic_load(ulg_ctx *c, const double *data, int64_t N, int n, double lambda) {
    if (!c || !data || N < 2 || n < 1 || n > kMaxVars) return set_err(c, ULG_ERR_ARG, "ulg_cbic_load: bad arguments");
    // an async call in flight reads the Gram matrix this load replaces, and its
    // pending flag would outlive `scored`: collect it first, as ulg_disc_load does
    if (int rc0 = finish_pending(c)) return rc0;
    ULG_HIP(c, hipSetDevice(c->device));
    c->loaded = false;
    c->scored = false;
    if (!c->cons_var.empty()) {  // constraints belong to the data they were set for
        graph_reset(c);
        c->cons_var.clear();
        c->cons_req.clear();
        c->cons_forb.clear();
    }
    c->n = n;
    c->N = N;
    c->lambda = lambda;
    c->npad = (n + 15) / 16 * 16;
    const int tiles = c->npad / 16;
    const int chunks = (int)((N + kGramRows - 1) / kGramRows);
    int rc;
    if ((rc = ensure(c, c->raw, (size_t)(N * n))) || (rc = ensure(c, c->z, (size_t)(N * c->npad))) ||
        (rc = ensure(c, c->gram, (size_t)(n * n))) || (rc = ensure(c, c->colstat, (size_t)(2 * n))) ||
        (rc = ensure(c, c->partials, (size_t)chunks * tiles * tiles * 256)))
        return rc;
    ULG_HIP(c, hipMemcpyAsync(c->raw.p, data, sizeof(double) * (size_t)(N * n), hipMemcpyHostToDevice, c->stream));
    prof_begin(c, "colstats");
    colstats_kernel<<<n, kBlock, 0, c->stream>>>(c->raw.p, N, c->colstat.p);
    prof_end(c);
    const int64_t tot = N * c->npad;
    prof_begin(c, "normalise");
    normalise_kernel<<<(unsigned)((tot + kBlock - 1) / kBlock), kBlock, 0, c->stream>>>(c->raw.p, N, n, c->npad,
                                                                                         c->colstat.p, c->z.p);
    prof_end(c);
    prof_begin(c, "gram_mfma_f64");
    gram_mfma_kernel<<<dim3(chunks, tiles * tiles), 64, 0, c->stream>>>(c->z.p, N, c->npad, tiles, c->partials.p);
    prof_end(c);
    prof_begin(c, "gram_reduce");
    gram_reduce_kernel<<<(n * n + kBlock - 1) / kBlock, kBlock, 0, c->stream>>>(c->partials.p, chunks, tiles, n,
                                                                               c->gram.p);
    prof_end(c);
    // the BIC penalty per parent, once per load and from the device's own
    // log: the host's libm may round ln(N) differently
    if ((rc = ensure(c, c->d_pen, 1))) return rc;
    penalty_kernel<<<1, 1, 0, c->stream>>>((double)N, lambda, c->d_pen.p);
    ULG_HIP(c, hipGetLastError());
    ULG_HIP(c, hipMemcpyAsync(&c->pen, c->d_pen.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    // the host copy of the Gram matrix the launch images are built from
    c->h_gram.resize((size_t)n * n);
    ULG_HIP(c, hipMemcpyAsync(c->h_gram.data(), c->gram.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost,
                              c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->loaded = true;
    fnml_drop(c);  // the discrete data is no longer the context's
    return ULG_OK;
}

int ulg_cbic_gram(ulg_ctx *c, double *out) {
    if (!c || !out) return ULG_ERR_ARG;
    if (!c->loaded) return set_err(c, ULG_ERR_STATE, "ulg_cbic_gram: no data loaded");
    ULG_HIP(c, hipSetDevice(c->device));
    ULG_HIP(c, hipMemcpy(out, c->gram.p, sizeof(double) * (size_t)(c->n * c->n), hipMemcpyDeviceToHost));
    return ULG_OK;
}

int ulg_cbic_score_finish(ulg_ctx *c, int64_t *total_stored, int64_t *total_scored) {
    if (!c) return ULG_ERR_ARG;
    if (c->async_pending) {
        c->async_pending = false;
        ULG_HIP(c, hipSetDevice(c->device));
        ULG_HIP(c, hipStreamSynchronize(c->stream));
        prof_collect(c);
        c->total_stored = (int64_t)c->async_pinned.p[0];
        c->last_err_word = c->async_pinned.p[1];
        if (int rc = call_error(c, c->async_pinned.p[1])) {
            c->scored = false;
            return rc;
        }
    }
    if (!c->scored) return set_err(c, ULG_ERR_STATE, "ulg_cbic_score_finish: nothing scored");
    if (total_stored) *total_stored = c->total_stored;
    if (total_scored) *total_scored = c->total_scored;
    return ULG_OK;
}

namespace {

// The unrank tables the plan added to `staged`, a copy of the context's cache
// (p.lut_new): room for them behind the tables already there, whose entries
// move along when the buffer grows, and one fill launch each -- on the context
// stream, before the call's launches and outside their capture.  Then the
// call's offsets.  Only when all of that is enqueued does `staged` become the
// context's cache: after any earlier return (here, or in reserve_buffers
// before it) the context's cache still names exactly the tables d_lut holds
// filled, and the next call plans the missing ones again.
int reserve_luts(ulg_ctx *c, const CbicPlan &p, LutCache &staged) {
    if (!p.lut_new.empty()) {
        const uint64_t old_total = c->lut_cache.total, total = staged.total;
        if (c->d_lut.cap < total) {
            DevBuf<uint32_t> grown;
            if (int rc = ensure(c, grown, (size_t)std::max<uint64_t>(total, 2 * c->d_lut.cap))) return rc;
            if (old_total) {
                hipError_t e = hipMemcpyAsync(grown.p, c->d_lut.p, old_total * sizeof(uint32_t),
                                              hipMemcpyDeviceToDevice, c->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                if (e != hipSuccess)  // d_lut and the context's cache stay as they were
                    return set_err(c, ULG_ERR_HIP, std::string("unrank table copy failed: ") + hipGetErrorString(e));
            }
            c->d_lut = std::move(grown);
        }
        for (const LutTable &t : p.lut_new)
            unrank_lut_fill_kernel<<<(unsigned)((t.count + kBlock - 1) / kBlock), kBlock, 0, c->stream>>>(
                c->d_lut.p + t.off, (uint32_t)t.count, t.l, t.U, c->d_binom.p);
        ULG_HIP(c, hipGetLastError());
    }
    if (p.lut_any)
        if (int rc = upload(c, c->d_lutoff, c->mir_lutoff, p.lutoff)) return rc;
    c->lut_cache = std::move(staged);
    return ULG_OK;
}

// Every device buffer the plan sizes, the uploads of its tables (skipped when
// the device already holds the same bytes) and the groups' streams and events.
int reserve_buffers(ulg_ctx *c, const ScoreLists &ls, const CbicPlan &p) {
    const uint64_t total_slots = ls.total_slots;
    const int nv = ls.nv, G = p.G;
    int rc;
    // the output lists are sized for every slot, so the compaction needs no
    // mid-call sync for the stored count
    if ((rc = ensure(c, c->table, total_slots)) || (rc = upload(c, c->d_tbl_off, c->mir_tbl_off, ls.toff)) ||
        (rc = upload(c, c->d_work, c->mir_work, p.work)) || (rc = upload(c, c->d_cand, c->mir_cand, ls.cand)) ||
        (rc = upload(c, c->d_meta, c->mir_meta, p.meta)) || (rc = ensure(c, c->out_sets, total_slots)) ||
        (rc = ensure(c, c->out_scores, total_slots)) || (rc = ensure(c, c->out_offsets, (size_t)nv + 1)))
        return rc;
    if (p.cons_words && (rc = upload(c, c->d_cons, c->mir_cons, p.ct))) return rc;
    c->cons_call_words = p.cons_words;
    if ((p.variant & 64) && (rc = ensure(c, c->d_hsub, total_slots))) return rc;
    while ((int)c->aux_streams.size() < G - 1) {
        hipStream_t st;
        ULG_HIP(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        c->aux_streams.push_back(st);
    }
    while ((int)c->sync_events.size() < 2 * G) {
        hipEvent_t ev;
        ULG_HIP(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->sync_events.push_back(ev);
    }
    if (G > 1 && (rc = upload(c, c->d_workg, c->mir_workg, p.workg))) return rc;
    if (p.zero_q &&
        ((rc = ensure(c, c->d_queue, (size_t)G * p.qwords)) || (rc = ensure(c, c->d_qcount, p.nqc)) ||
         (rc = ensure(c, c->d_wqueue, (size_t)G * p.wqwords)) || (rc = ensure(c, c->d_qseg, (size_t)p.nqseg))))
        return rc;
    if (p.bucket &&
        ((rc = ensure(c, c->d_qkey, (size_t)(G * p.qcap))) || (rc = ensure(c, c->d_qaux, (size_t)(G * p.qcap))) ||
         (rc = ensure(c, c->d_qsidx, (size_t)(G * p.qcap))) ||
         (rc = ensure(c, c->d_qoffs, (size_t)(G * kBucketMax * p.nseg_max)))))
        return rc;
    if (p.kmax > kMaxL) {
        // wide-layer walks: the checked bitsets, allocated before any launch
        if ((rc = ensure(c, c->d_wbits, (size_t)(G * p.wslice))) || (rc = ensure(c, c->d_scount, (size_t)G)) ||
            (rc = ensure(c, c->d_hq, (size_t)G * std::max<uint64_t>(p.wqwords / 6, 1))) ||
            (rc = ensure(c, c->d_hqc, (size_t)G)))
            return rc;
        if (!p.hoff.empty()) {
            c->hmax_half = p.htot;  // d_hmax = [hi-cover maxima][present values]
            if ((rc = ensure(c, c->d_hmax, (size_t)(2 * p.htot))) || (rc = upload(c, c->d_hoff, c->mir_hoff, p.hoff)) ||
                (rc = ensure(c, c->d_hmeta, (size_t)G * p.hmeta_stride())))
                return rc;
        }
        if ((int)c->wide_host.size() < 2 * G) {
            if ((rc = ensure(c, c->wide_pinned, 2 * (size_t)G))) return rc;
            c->wide_host.assign(2 * G, 0);
        }
    }
    return ensure(c, c->d_blk, (size_t)p.nb + 2);
}

// What a captured launch sequence depends on: the call, the options and every
// buffer address its kernels were given.
void graph_key(const ulg_ctx *c, const ScoreLists &ls, const CbicPlan &p, const uint64_t *candidates,
               std::vector<uint64_t> &gkey) {
    auto ptr = [](const void *q) { return (uint64_t)(uintptr_t)q; };
    gkey.assign({(uint64_t)ls.nv, (uint64_t)ls.max_parents, (uint64_t)p.variant, (uint64_t)p.G, (uint64_t)p.Ls,
                 (uint64_t)c->opt.score_xcd, (uint64_t)ls.n, (uint64_t)c->N, dbits(c->lambda), (uint64_t)c->prof,
                 (uint64_t)c->opt.walk_small_sets, (uint64_t)c->opt.walk_k6, (uint64_t)c->opt.walk_bucket, ptr(c->d_qaux.p),
                 ptr(c->d_qsidx.p), ptr(c->d_qkey.p), ptr(c->d_qoffs.p), ptr(c->table.p), ptr(c->d_work.p),
                 ptr(c->d_workg.p), ptr(c->d_queue.p), ptr(c->d_qcount.p), ptr(c->d_qseg.p), ptr(c->d_cand.p),
                 ptr(c->d_meta.p), ptr(c->d_tbl_off.p), ptr(c->out_sets.p), ptr(c->out_scores.p),
                 ptr(c->out_offsets.p), ptr(c->d_blk.p), ptr(c->gram.p), ptr(c->d_binom.p), ptr(c->d_binom64.p),
                 ptr(c->d_hsub.p), (uint64_t)ls.total_slots, (uint64_t)c->opt.score_small_layers, (uint64_t)c->opt.score_fused,
                 (uint64_t)p.cons_words, ptr(p.cons_words ? c->d_cons.p : nullptr), dbits(c->pen),
                 (uint64_t)c->opt.score_unrank_lut, ptr(p.lut_any ? c->d_lut.p : nullptr),
                 ptr(p.lut_any ? c->d_lutoff.p : nullptr), (uint64_t)c->opt.score_lds_image,
                 ptr(p.image_any ? c->d_image.p : nullptr), (uint64_t)c->opt.score_narrow,
                 // the sets per lane of the sliced walks as ULG_SLICED_K resolves them now
                 // (layers <= 5, layer 6): sliced_k reads the variable at launch time
                 (uint64_t)sliced_k(5), (uint64_t)sliced_k(6, ~0ull, 0, (int)c->opt.walk_k6)});
    for (int i = 0; i < ls.nv; ++i) gkey.push_back((uint64_t)ls.vars[i]);
    for (int i = 0; i < ls.nv; ++i) gkey.push_back(candidates[i]);
    for (const std::string &nm : c->prof_only) gkey.push_back(std::hash<std::string>{}(nm));
}

// The slabs into the output lists: stored sets per block, their scan (the
// total and the error word land behind it), the (set, score) pairs.  After an
// exhausted -r budget the layers never launched hold no stored set.
int compact(const ScoreCall &k, int done_L) {
    ulg_ctx *c = k.c;
    const ScoreLists &ls = k.ls;
    const int nv = ls.nv, S = ls.S;
    const int64_t nb = k.p.nb;
    for (int i = 0; i < nv && done_L < ls.kmax; ++i) {
        const uint64_t b = ls.toff[(size_t)i * S + done_L + 1], e = ls.toff[(size_t)i * S + S];
        if (e > b) ULG_HIP(c, hipMemsetAsync(c->table.p + b, 0xff, (size_t)(e - b) * 4, c->stream));
    }
    c->completed_layer = done_L;
    prof_begin(c, "count_stored");
    count_kernel<<<(unsigned)nb, kBlock, 0, c->stream>>>(c->table.p, ls.total_slots, c->d_blk.p);
    prof_end(c);
    prof_begin(c, "scan_stored");
    scan_kernel<<<1, 1024, 0, c->stream>>>(c->d_blk.p, nb, c->out_offsets.p + nv, k.errf());
    prof_end(c);
    const WriteArgs wa{c->table.p,      c->d_blk.p,    c->d_tbl_off.p,  c->d_meta.p,      c->d_cand.p, c->d_binom.p,
                       c->d_binom64.p,  ls.total_slots, nv,             S,                c->out_sets.p,
                       c->out_scores.p, c->out_offsets.p};
    const size_t nseg = (size_t)nv * (size_t)S;
    const size_t toff_bytes = nseg <= (size_t)kWriteLdsSegs ? (nseg + 1) * sizeof(uint64_t) : 0;
    prof_begin(c, "write_stored");
    write_kernel<<<(unsigned)nb, kBlock, toff_bytes, c->stream>>>(wa);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    return ULG_OK;
}

// An early return between BeginCapture and EndCapture (a failed launch,
// "layer too large") must not leave the context stream capturing: the
// guard ends the capture, drops the partial graph and the key.
struct CaptureGuard {
    ulg_ctx *c;
    bool active;
    ~CaptureGuard() {
        if (!active) return;
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(c->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        c->gkey.clear();
        (void)hipGetLastError();
    }
};

// The call's launches, prologue to write_kernel.  The sequence has no host
// sync when every layer is unrolled and no budget / diagnostic is on, and it
// is the same on every call with the same variables, limits and buffers: it
// is captured once into a hipGraph (all stream groups, the fork and join
// events, the profiling events) and replayed, which removes the host launch
// path of ~40 kernels per call (score_graph, default on).
int launch_call(const ScoreCall &k, const uint64_t *candidates) {
    ulg_ctx *c = k.c;
    const int kmax = k.p.kmax;
    const bool use_graph = c->opt.score_graph && !c->prof && kmax <= kMaxL && c->opt.time_limit_ms == 0 && !k.wck;
    std::vector<uint64_t> gkey;
    CaptureGuard capture_guard{c, false};
    c->out_of_time = 0;
    if (use_graph) {
        graph_key(c, k.ls, k.p, candidates, gkey);
        if (c->gexec && gkey == c->gkey) {
            c->completed_layer = kmax;
            ULG_HIP(c, hipGraphLaunch(c->gexec, c->stream));
            for (const ProfRec &r : c->gprof) c->pending.push_back(r);
            return ULG_OK;
        }
        graph_reset(c);
        ++c->graph_captures;
        ULG_HIP(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
        capture_guard.active = true;
    }
    const size_t pend0 = c->pending.size();
    int rc, done_L = kmax;
    if ((rc = launch_prologue(k)) || (rc = launch_layers(k, done_L)) || (rc = compact(k, done_L))) return rc;
    if (!use_graph) return ULG_OK;
    hipGraph_t graph = nullptr;
    capture_guard.active = false;
    ULG_HIP(c, hipStreamEndCapture(c->stream, &graph));
    c->graph = graph;
    ULG_HIP(c, hipGraphInstantiate(&c->gexec, graph, nullptr, nullptr, 0));
    c->gkey = gkey;
    // the profiling events recorded inside the graph belong to it now
    c->gprof.assign(c->pending.begin() + (std::ptrdiff_t)pend0, c->pending.end());
    for (ProfRec &r : c->gprof) r.graph = true;
    c->pending.resize(pend0);
    ULG_HIP(c, hipGraphLaunch(c->gexec, c->stream));
    for (const ProfRec &r : c->gprof) c->pending.push_back(r);
    return ULG_OK;
}

// The stored count and the error word through the context's pinned words (a
// pageable destination goes through a staging copy), and the call's lists
// into the context.  Async: no host sync; ulg_cbic_score_finish collects the
// words once the launches are done.
int collect(ulg_ctx *c, const ScoreLists &ls, int64_t nb, bool async, int64_t *total_stored, int64_t *total_scored) {
    if (int rc = ensure(c, c->async_pinned, 2)) return rc;
    ULG_HIP(c, hipMemcpyAsync(c->async_pinned.p, c->d_blk.p + nb, 16, hipMemcpyDeviceToHost, c->stream));
    int64_t stored = 0;
    if (!async) {
        ULG_HIP(c, hipStreamSynchronize(c->stream));
        stored = (int64_t)c->async_pinned.p[0];
        prof_collect(c);
        if (int rc = call_error(c, c->async_pinned.p[1])) return rc;
    }
    publish(c, ls, stored, async);
    if (total_stored) *total_stored = c->total_stored;
    if (total_scored) *total_scored = c->total_scored;
    return ULG_OK;
}

int cbic_score(ulg_ctx *c, const int *vars, int nv, const uint64_t *candidates, int max_parents,
               int64_t *total_stored, int64_t *total_scored, bool async) {
    if (!c) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!c->loaded) return set_err(c, ULG_ERR_STATE, "ulg_cbic_score: call ulg_cbic_load first");
    ScoreLists &ls = c->lists;
    CbicPlan &p = c->plan;
    if (ScoreLists::Status st = ls.build(c->n, vars, nv, candidates, max_parents))
        return lists_error(c, "ulg_cbic_score", st);
    ULG_HIP(c, hipSetDevice(c->device));
    const char *wck = std::getenv("ULG_WALK_CLOCK");
    p.build(ls, c->cons_var, c->cons_req, c->cons_forb, c->opt, wck != nullptr);
    // the tables are planned on a copy of the context's cache, which takes
    // the copy's place only once they are allocated and their fills enqueued
    LutCache staged = c->lut_cache;
    p.build_luts(ls, c->opt.score_unrank_lut, staged);
    if (int rc = reserve_buffers(c, ls, p)) return rc;
    if (int rc = reserve_luts(c, p, staged)) return rc;
    // the launch images last: they hold the tables' offsets, and a call that
    // failed above has changed neither d_image nor its mirror
    p.build_images(ls, c->h_gram.data(), host_binom().data(), c->opt.score_lds_image != 0);
    if (p.image_any)
        if (int rc = upload(c, c->d_image, c->mir_image, p.image)) return rc;

    ScoreCall k{c, ls, p, ConsTable{p.cons_words ? c->d_cons.p : nullptr, p.cons_words, p.cons_lds}, ScoreArgs{},
                p.G > 1 ? c->d_workg.p : c->d_work.p, std::vector<hipStream_t>(p.G), wck};
    k.gst[0] = c->stream;
    for (int g = 1; g < p.G; ++g) k.gst[g] = c->aux_streams[g - 1];
    ScoreArgs &sa = k.sa;  // work, queue, qcount and qkey stay null: each launch sets its own
    sa.hsub_out = 1;
    sa.gram = c->gram.p;
    sa.binom = c->d_binom.p;
    sa.cand = c->d_cand.p;
    sa.meta = c->d_meta.p;
    sa.tbl_off = c->d_tbl_off.p;
    sa.table = c->table.p;
    sa.hsub = (p.variant & 64) ? c->d_hsub.p : nullptr;
    sa.err = k.errf();
    sa.N = (double)c->N;
    sa.pen = c->pen;
    sa.lut = p.lut_any ? c->d_lut.p : nullptr;
    sa.n = ls.n;
    sa.nv = ls.nv;
    sa.S = ls.S;
    sa.xcd = c->opt.score_xcd;
    if (int rc = launch_call(k, candidates)) return rc;
    return collect(c, ls, p.nb, async && p.kmax <= kMaxL && c->opt.time_limit_ms == 0, total_stored, total_scored);
}

}  // namespace

int ulg_cbic_score(ulg_ctx *c, const int *vars, int nv, const uint64_t *candidates, int max_parents,
                   int64_t *total_stored, int64_t *total_scored) {
    return cbic_score(c, vars, nv, candidates, max_parents, total_stored, total_scored, false);
}

int ulg_cbic_score_async(ulg_ctx *c, const int *vars, int nv, const uint64_t *candidates, int max_parents) {
    return cbic_score(c, vars, nv, candidates, max_parents, nullptr, nullptr, true);
}

int ulg_cbic_fetch(ulg_ctx *c, uint64_t *sets, float *scores, int64_t *offsets, int device_ptrs) {
    if (!c) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!c->scored) return set_err(c, ULG_ERR_STATE, "ulg_cbic_fetch: nothing scored");
    ULG_HIP(c, hipSetDevice(c->device));
    const hipMemcpyKind k = device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t cnt = (size_t)c->total_stored;
    if (sets && cnt) ULG_HIP(c, hipMemcpyAsync(sets, c->out_sets.p, cnt * 8, k, c->stream));
    if (scores && cnt) ULG_HIP(c, hipMemcpyAsync(scores, c->out_scores.p, cnt * 4, k, c->stream));
    if (offsets) ULG_HIP(c, hipMemcpyAsync(offsets, c->out_offsets.p, (size_t)(c->nv + 1) * 8, k, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    return ULG_OK;
}

int ulg_cbic_set_constraints(ulg_ctx *c, int count, const int *vars, const uint64_t *required,
                             const uint64_t *forbidden) {
    if (!c) return ULG_ERR_ARG;
    if (!c->loaded && !c->disc_loaded)
        return set_err(c, ULG_ERR_ARG, "ulg_cbic_set_constraints: call ulg_cbic_load or ulg_disc_load first");
    if (count < 0 || (count > 0 && (!vars || !required || !forbidden)))
        return set_err(c, ULG_ERR_ARG, "ulg_cbic_set_constraints: bad arguments");
    const int n = c->n;
    const uint64_t allmask = (n >= 64) ? ~0ull : ((1ull << n) - 1ull);
    std::vector<int> per(n, 0);
    for (int i = 0; i < count; ++i) {
        if (vars[i] < 0 || vars[i] >= n)
            return set_err(c, ULG_ERR_ARG, "ulg_cbic_set_constraints: variable out of range");
        if ((required[i] | forbidden[i]) & ~allmask)
            return set_err(c, ULG_ERR_ARG, "ulg_cbic_set_constraints: mask bit >= n");
        if (++per[vars[i]] > ULG_MAX_CONSTRAINT_ALTERNATIVES)
            return set_err(c, ULG_ERR_UNSUPPORTED,
                           "ulg_cbic_set_constraints: more than ULG_MAX_CONSTRAINT_ALTERNATIVES (64) alternatives "
                           "for variable " + std::to_string(vars[i]));
    }
    if (int rc0 = finish_pending(c)) return rc0;  // the launches in flight read the tables
    ULG_HIP(c, hipSetDevice(c->device));
    // the captured scoring graph holds the kernels and the table pointer of
    // the constraints it was captured under
    graph_reset(c);
    c->cons_var.assign(vars, vars + count);
    c->cons_req.assign(required, required + count);
    c->cons_forb.assign(forbidden, forbidden + count);
    c->cons_call_words = 0;
    if (count == 0) return ULG_OK;
    // ulg_cbic_score_sets' table: by variable, in variable masks
    std::vector<uint64_t> ct((size_t)n + 1, 0);
    for (int v = 0; v < n; ++v) {
        ct[v] = (ct.size() - (size_t)(n + 1)) / 2;
        for (int i = 0; i < count; ++i)
            if (vars[i] == v) {
                ct.push_back(required[i]);
                ct.push_back(forbidden[i]);
            }
    }
    ct[n] = (ct.size() - (size_t)(n + 1)) / 2;
    int rc;
    if ((rc = ensure(c, c->d_cons_var, ct.size()))) return rc;
    ULG_HIP(c, hipMemcpy(c->d_cons_var.p, ct.data(), ct.size() * 8, hipMemcpyHostToDevice));
    return ULG_OK;
}

int ulg_cbic_score_vars(ulg_ctx *c, const int *vars, int nv, const uint64_t *candidates, int max_parents,
                        uint64_t *sets, float *scores, int64_t *offsets, int64_t cap) {
    int64_t stored = 0;
    int rc = ulg_cbic_score(c, vars, nv, candidates, max_parents, &stored, nullptr);
    if (rc) return rc;
    if (stored > cap) return set_err(c, ULG_ERR_ARG, "ulg_cbic_score_vars: output capacity too small");
    return ulg_cbic_fetch(c, sets, scores, offsets, 0);
}

int ulg_cbic_score_sets(ulg_ctx *c, int64_t count, const int *vars, const uint64_t *parents, float *neg_scores) {
    if (!c || count < 0 || (count > 0 && (!vars || !parents || !neg_scores))) return ULG_ERR_ARG;
    if (!c->loaded) return set_err(c, ULG_ERR_STATE, "ulg_cbic_score_sets: call ulg_cbic_load first");
    if (count == 0) return ULG_OK;
    const int n = c->n;
    const uint64_t allmask = (n >= 64) ? ~0ull : ((1ull << n) - 1ull);
    std::vector<uint64_t> pairs((size_t)count * 2);
    for (int64_t i = 0; i < count; ++i) {
        if (vars[i] < 0 || vars[i] >= n) return set_err(c, ULG_ERR_ARG, "ulg_cbic_score_sets: variable out of range");
        if (parents[i] & ~allmask) return set_err(c, ULG_ERR_ARG, "ulg_cbic_score_sets: parent bit >= n");
        if (__builtin_popcountll(parents[i] & ~(1ull << vars[i])) > kWideMax)
            return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_cbic_score_sets: more than ULG_MAX_PARENTS_GPU (31) parents");
        pairs[2 * i] = (uint64_t)vars[i];
        pairs[2 * i + 1] = parents[i];
    }
    ULG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->d_sets_in, (size_t)count * 2)) || (rc = ensure(c, c->qbuf_out, (size_t)count))) return rc;
    ULG_HIP(c, hipMemcpyAsync(c->d_sets_in.p, pairs.data(), (size_t)count * 16, hipMemcpyHostToDevice, c->stream));
    // the twin takes the by-variable table (ulg_cbic_set_constraints) after the common arguments
    const dim3 grid((unsigned)((count + kBlock - 1) / kBlock)), block(kBlock);
    if ((rc = c->cons_var.empty()
                  ? launch_kernel(c, score_sets_kernel, grid, block, n * n * 8, c->stream, "score_sets", c->gram.p,
                                  c->d_sets_in.p, count, n, c->N, c->pen, c->qbuf_out.p)
                  : launch_kernel(c, score_sets_cons_kernel, grid, block, n * n * 8, c->stream, "score_sets",
                                  c->gram.p, c->d_sets_in.p, count, n, c->N, c->pen, c->qbuf_out.p,
                                  c->d_cons_var.p)))
        return rc;
    ULG_HIP(c, hipMemcpyAsync(neg_scores, c->qbuf_out.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ULG_OK;
}

int ulg_quantize_costs(ulg_ctx *c, const float *scores, float *costs, int64_t count) {
    if (!c || count < 0 || (count > 0 && (!scores || !costs))) return ULG_ERR_ARG;
    if (count == 0) return ULG_OK;
    ULG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->qbuf_in, (size_t)count)) || (rc = ensure(c, c->qbuf_out, (size_t)count))) return rc;
    ULG_HIP(c, hipMemcpyAsync(c->qbuf_in.p, scores, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
    prof_begin(c, "quantize");
    quantize_kernel<<<(unsigned)((count + kBlock - 1) / kBlock), kBlock, 0, c->stream>>>(c->qbuf_in.p, c->qbuf_out.p,
                                                                                       count);
    prof_end(c);
    ULG_HIP(c, hipMemcpyAsync(costs, c->qbuf_out.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ULG_OK;
}

#ifdef ULG_GATHER_STATS
// diagnostic build: the gather counters (2 * (kMaxL + 1) * 16 values), then
// the walk's hits by depth (as many), both zeroed
int ulg_diag_gather_stats(ulg_ctx *c, unsigned long long *out) {
    if (!c || !out) return ULG_ERR_ARG;
    ULG_HIP(c, hipSetDevice(c->device));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    ULG_HIP(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gstats), sizeof(g_gstats)));
    static const unsigned long long zero[2 * (kMaxL + 1) * 16] = {};
    ULG_HIP(c, hipMemcpyToSymbol(HIP_SYMBOL(g_gstats), zero, sizeof(zero)));
    ULG_HIP(c, hipMemcpyFromSymbol(out + 2 * (kMaxL + 1) * 16, HIP_SYMBOL(g_wstats), sizeof(g_wstats)));
    ULG_HIP(c, hipMemcpyToSymbol(HIP_SYMBOL(g_wstats), zero, sizeof(zero)));
    return ULG_OK;
}
#endif

}  // extern "C"
