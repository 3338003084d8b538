// cbic_layer_dev.h -- what the cBIC scorer's translation units share on the
// device: the layer launches' arguments (ScoreArgs), the constraint test,
// the error word's bits, the walk queue's append, a set's head and its
// one-pass form (the texts cbic_score_layer.inc and cbic_score_small.inc are
// compiled around, once in cbic_layers.hip and once in cbic_layers_cons.hip),
// and the 64-bit colex rank of the wide layers and the compaction.  Built on
// cbic_dev.h's blocks; types and functions here are in namespace ulg.
#pragma once
#include "cbic_dev.h"

namespace ulg {

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
// cbic_score_{layer,small,wide,sets}.inc compiled a second time with
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
// what the presence gathers of the compacted sets find.  One copy per
// translation unit: ulg_diag_gather_stats reads cbic_layers.hip's, the
// unconstrained kernels' (the diagnostic runs hold no constraints).
static __device__ unsigned long long g_gstats[2 * (kMaxL + 1) * 16];

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
    gather_keys<L, PHASE, V, BS, LdPlain, 2, TO>(present, hib, ls, -tk, binom, zk, a.table, toffv);
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
        queue_walk<L, PHASE, BS, sizeof(M) == 4>(present, hib, a.queue + seg * kSegEntries * (uint64_t)(1 + 2 * W),
                                                 a.qcount + seg * kSegStride, a.err, sk, tk,
                             a.qkey ? a.qkey + seg * kSegEntries : nullptr);
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

}  // namespace ulg
