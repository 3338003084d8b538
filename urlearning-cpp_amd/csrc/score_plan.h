// score_plan.h -- the host arithmetic of a scoring call, free of HIP: the
// candidate lists and slot table both scorers share (ScoreLists) and every
// size, prefix and offset the cBIC scorer derives from them before its first
// launch (CbicPlan).  Plain C++17: host/plan_check.cpp checks it against
// brute-force subset enumeration without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ulg.h"
#include "options.h"  // Options: the plan reads the scorer's options from it

#if defined(__HIPCC__)
#define ULG_HD __host__ __device__
#else
#define ULG_HD
#endif

namespace ulg {

constexpr int kMaxVars = 63;                     // varset = uint64, bit 63 kept free
constexpr int kMaxL = ULG_UNROLLED_PARENTS_GPU;  // unrolled layers on the device
constexpr int kWideMax = ULG_MAX_PARENTS_GPU;    // wide layers kMaxL+1 .. kWideMax (cbic_wide.hip)

constexpr int kBlock = 256;

// Constraint tables of at most kConsLdsWords words are copied into LDS behind
// the block's layout (cbic_layer_dev.h cons_stage).
constexpr int kConsLdsWords = 256;

// The walk queue of a two-pass launch is cut into nseg = ceil(blocks /
// kSegBlocks) segments, each with its own counter on its own 128-byte line:
// one counter for the whole launch took ~23 K wave atomics in a row at C3's
// layer 6 and cost a third of the scoring kernel (318 -> 204 us without it).
// Block b queues into segment b mod nseg, so the blocks resident at any time
// spread over all counters and every segment is a cross-section of the
// launch (segments of neighbouring blocks cluster the long walks into the
// same walk waves: the layer-6 walk launch took 2x longer).  Segment s holds
// its queued sets at entries [s * kSegEntries, s * kSegEntries + count_s);
// the walk kernel takes one (segment, chunk) per wave.
constexpr int kSegBlocks = 32;
constexpr uint64_t kSegEntries = (uint64_t)kSegBlocks * kBlock;
constexpr int kSegStride = 16;  // counters 128 B apart
// A bucketed launch's header after its segment counters (zeroed with them):
// every key's set total (u32 64..191).
constexpr int kBucketHdrWords = 128;
constexpr int kBucketMax = 128;  // walk keys: 64 first-level patterns, the all-open one split 64 ways
constexpr uint64_t kWideBitsWords = 1ull << 27;  // checked bitsets, all stream groups together (1 GiB)
constexpr int kHiMaxBits = 24;  // 64 MB of floats per variable at most
constexpr int kSlotsPerThread = 16;  // contiguous slots per thread (four 16-B loads)
constexpr int kSlotsPerBlock = kBlock * kSlotsPerThread;

ULG_HD inline uint64_t seg_count(uint64_t blocks) { return (blocks + kSegBlocks - 1) / kSegBlocks; }
// 64-bit words of a layer-L set's local bitset (2^(L+1) bits)
ULG_HD constexpr int bits_words(int L) { return (L + 1) <= 6 ? 1 : (1 << ((L + 1) - 6)); }

constexpr int kBinomK = kMaxL + 2;  // binomial table columns C(a, 0..kBinomK-1)

// LDS carve: gram | binom | work, this launch's unrank-table offsets | tbl_off | meta | candidate lists |
// recursion stack (variant bit 1)
// | LDS bitsets (3 per lane when they have >= 4 words) | the block's
// undecided sets after the subset-maxima test (variant bits 4 + 6: a count,
// then per entry compact mask, slot, ts, children maximum, variable) (16-B
// aligned).  Host and device: the layer kernels carve their LDS with it, and
// CbicPlan::build_images lays the launch images out with it
// (host/lds_image_check.cpp).
struct LdsLayout {
    int gram, binom, work, lutoff, toff, meta, cand, stack, bits, cmp, cmp2, total;
};
constexpr int kCmpEntryBytes = 8 + 4 + 4 + 4 + 4;
ULG_HD inline int align16(int x) { return (x + 15) & ~15; }
#ifndef ULG_LDS_ALIAS
#define ULG_LDS_ALIAS 1
#endif
ULG_HD inline LdsLayout lds_layout(int n, int nv, int S, int L, int V) {
    LdsLayout l;
    if (ULG_LDS_ALIAS && (V & 208) == 208 && bits_words(L) < 4) {
        // the two-pass kernels with the second compaction (variant bit 7):
        // the Gram matrix, the work prefixes and the candidate lists are
        // read only before the block's first barrier (the scores and the
        // subset-maxima settle), and the compaction entries and their words
        // are written only after it -- so they share one region.  The
        // counters, the binomials, the slab offsets and the metadata, read
        // throughout, sit in front of it.  C3 layer 6: 26.7 -> 19 KB per
        // block, 6 -> 8 blocks per CU (C5: 5 -> 8).
        const int W = bits_words(L);
        l.binom = 0;
        l.toff = align16(l.binom + 64 * kBinomK * 4);
        l.meta = align16(l.toff + (nv * S + 1) * 8);
        l.cmp = align16(l.meta + nv * 4 * 4);  // 16 bytes of counters, then the entries
        const int ra = l.cmp + 16;             // the shared region
        l.gram = ra;
        l.work = align16(l.gram + n * n * 8);
        l.lutoff = l.work + (nv + 1) * 8;  // [nv] int32, read where work[] is: a straddling wave's lanes
        l.cand = align16(l.lutoff + nv * 4);
        l.stack = l.bits = align16(l.cand + nv * 64);
        l.cmp2 = align16(ra + kBlock * kCmpEntryBytes);
        const int endc = l.cmp2 + 2 * W * kBlock * 8;
        l.total = l.stack > endc ? l.stack : endc;
        return l;
    }
    l.gram = 0;
    l.binom = align16(l.gram + n * n * 8);
    l.work = align16(l.binom + 64 * kBinomK * 4);
    l.lutoff = l.work + (nv + 1) * 8;
    l.toff = align16(l.lutoff + nv * 4);
    l.meta = align16(l.toff + (nv * S + 1) * 8);
    l.cand = align16(l.meta + nv * 4 * 4);
    l.stack = align16(l.cand + nv * 64);
    l.bits = l.stack;
    const int W = bits_words(L);
    l.cmp = align16(l.bits + (W >= 4 ? 3 * W * kBlock * 8 : 0));
    // variant bit 7: the second compaction carries each set's gathered
    // present / hi words (register bitsets only, W < 4)
    l.cmp2 = align16(l.cmp + ((V & 80) == 80 ? 16 + kBlock * kCmpEntryBytes : 0));
    l.total = l.cmp2 + ((V & 208) == 208 && W < 4 ? 2 * W * kBlock * 8 : 0);
    return l;
}

// C(a, b), saturating at 2^64 - 1
inline uint64_t binom64(int a, int b) {
    if (b < 0 || b > a) return 0;
    if (b > a - b) b = a - b;
    unsigned __int128 r = 1;
    for (int i = 1; i <= b; ++i) r = r * (unsigned)(a - b + i) / (unsigned)i;
    return r > ~0ull ? ~0ull : (uint64_t)r;
}

// The variables of one scoring call, their candidate lists (the variable
// itself never enters a set, score_calculator.cpp:100) and the table slots of
// their parent sets: slab (i, L) holds variable i's sets of L parents in colex
// order.  Shared by ulg_cbic_score and ulg_disc_score.
struct ScoreLists {
    enum Status { kOk = 0, kBadList, kNotDistinct, kTooWide };

    int n = 0, nv = 0;
    int max_parents = 0;         // clamped to 1 .. n - 1
    int kmax = 0, S = 0;         // largest parent set of the call; layers 0 .. kmax
    std::vector<int> vars;       // [nv]
    std::vector<uint64_t> cmask; // [nv] candidates as a variable mask
    std::vector<uint8_t> cand;   // [nv][64] compact index -> variable
    std::vector<int> mv;         // [nv] candidate count
    std::vector<uint64_t> toff;  // [nv * S + 1] slab (i, L) -> first slot, then the total
    uint64_t total_slots = 0;

    // kTooWide leaves cand / mv / kmax built and toff untouched
    Status build(int n_, const int *vars_, int nv_, const uint64_t *candidates, int max_parents_) {
        if (!vars_ || !candidates || nv_ < 1 || nv_ > n_) return kBadList;
        uint64_t seen = 0;
        for (int i = 0; i < nv_; ++i) {
            if (vars_[i] < 0 || vars_[i] >= n_ || ((seen >> vars_[i]) & 1ull)) return kNotDistinct;
            seen |= 1ull << vars_[i];
        }
        n = n_;
        nv = nv_;
        max_parents = (max_parents_ < 1 || max_parents_ > n - 1) ? n - 1 : max_parents_;
        const uint64_t allmask = (n >= 64) ? ~0ull : ((1ull << n) - 1ull);
        vars.assign(vars_, vars_ + nv);
        cmask.resize(nv);
        cand.assign((size_t)nv * 64, 0);
        mv.resize(nv);
        kmax = 0;
        for (int i = 0; i < nv; ++i) {
            const uint64_t C = candidates[i] & allmask & ~(1ull << vars[i]);
            int m = 0;
            for (int b = 0; b < n; ++b)
                if ((C >> b) & 1ull) cand[(size_t)i * 64 + m++] = (uint8_t)b;
            cmask[i] = C;
            mv[i] = m;
            kmax = std::max(kmax, std::min(m, max_parents));
        }
        S = kmax + 1;
        if (kmax > kWideMax) return kTooWide;
        toff.resize((size_t)nv * S + 1);
        uint64_t acc = 0;
        for (int i = 0; i < nv; ++i)
            for (int L = 0; L < S; ++L) {
                toff[(size_t)i * S + L] = acc;
                acc += binom64(mv[i], L);  // L <= kmax <= max_parents
            }
        toff[(size_t)nv * S] = acc;
        total_slots = acc;
        return kOk;
    }

    // variable i's sets of L parents
    uint64_t slab_count(int i, int L) const { return toff[(size_t)i * S + L + 1] - toff[(size_t)i * S + L]; }

    // parent sets in layers 0 .. L of every variable
    int64_t scored_up_to(int L) const {
        int64_t s = 0;
        for (int i = 0; i < nv; ++i) s += (int64_t)(toff[(size_t)i * S + std::min(L, kmax) + 1] - toff[(size_t)i * S]);
        return s;
    }

    // the text after the caller's name in its error message
    static const char *status_text(Status st) {
        switch (st) {
            case kBadList: return ": bad variable list";
            case kNotDistinct: return ": variables must be distinct and < n";
            case kTooWide: return ": parent sets larger than ULG_MAX_PARENTS_GPU (31) are not supported";
            default: return "";
        }
    }
};

#if defined(__HIPCC__)
#define ULG_UNROLL _Pragma("unroll")
#else
#define ULG_UNROLL
#endif

// Children ranks of a layer-L set P = {a_1 < ... < a_L} (compact mask cm) from
// a clamped 32-bit binomial table C(a, b) at binom[a * STRIDE + b]:
//   rank(P\a_i)       = sum_{j<i} C(a_j, j)   + sum_{j>i} C(a_j, j-1)
//   rank(P\a_i + {0}) = sum_{j<i} C(a_j, j+1) + sum_{j>i} C(a_j, j)   (a_1 >= 1)
// Returns P's own colex rank, sum_j C(a_j, j): the binomials are the e[] the
// children's ranks already fetch, so the two-pass kernels take the set's slot
// from here instead of adding the same table reads up again (rank_colex).
// Ranks of the unrolled layers fit 32 bits.  Host and device: the layer
// kernels' child_ranks (cbic_dev.h) is this function, and
// host/unrank_lut_check.cpp runs it against the enumeration order.
// M: the mask and rank type, uint64_t, or uint32_t in the narrow layer kernels
// (launches whose every mask fits 32 bits, CbicPlan::narrow_fits): the same
// integers from one-register masks (host/narrow_check.cpp).
ULG_HD inline int mask_ctz(uint64_t x) { return __builtin_ctzll(x); }
ULG_HD inline int mask_ctz(uint32_t x) { return __builtin_ctz(x); }
// The L lowest elements of a mask in increasing order (the mask holds at
// least L): set_head's walk of a set's members (cbic_layer_dev.h); child_ranks_t
// below walks the same chain, and the compiler shares the two.
template <int L, class M>
ULG_HD inline __attribute__((always_inline)) void mask_elements(M mask, int (&el)[L]) {
    M rem = mask;
    ULG_UNROLL
    for (int j = 0; j < L; ++j) {
        el[j] = mask_ctz(rem);
        rem &= rem - 1;
    }
}
template <int L, bool WITH0, int STRIDE, class M>
ULG_HD inline __attribute__((always_inline)) uint32_t child_ranks_t(M cm, const uint32_t *binom, M (&rc)[L], M (&rz)[L]) {
    uint32_t e[L], d[L], f[L];
    M rem = cm;
    ULG_UNROLL
    for (int j = 0; j < L; ++j) {
        const int aj = mask_ctz(rem);
        rem &= rem - 1;
        e[j] = binom[aj * STRIDE + j + 1];
        d[j] = binom[aj * STRIDE + j];
        f[j] = WITH0 ? binom[aj * STRIDE + j + 2] : 0u;
    }
    uint32_t pe = 0, pf = 0;
    ULG_UNROLL
    for (int i = 0; i < L; ++i) {
        uint32_t sd = 0, se = 0;
        ULG_UNROLL
        for (int j = i + 1; j < L; ++j) {
            sd += d[j];
            se += e[j];
        }
        rc[i] = pe + sd;
        rz[i] = pf + se;
        pe += e[i];
        pf += f[i];
    }
    return pe;
}

// Unrank tables (option score_unrank_lut).  The mapping rank -> set of
// unrank_colex(r, l, U) depends only on (U, l), not on the data, the variable
// or the call, so the layer kernels L = kLutMinL .. kMaxL read it from a table
// of C(U, l) 32-bit masks filled once per context (unrank_lut_fill_kernel,
// cbic.hip) instead of computing it in every lane.  The cache only grows: a
// table keeps its offset for the life of the context, and every variable,
// phase, layer and call with the same (U, l) shares it.
constexpr int kLutMinL = 4;     // layers below run in the fused small kernel
constexpr int kLutMaxU = 32;    // a table entry is a 32-bit mask
// kLutDefaultCap, kLutMaxTotal: options.h
struct LutTable {
    int U, l;
    uint64_t off, count;  // entries
};
struct LutCache {
    std::vector<LutTable> tables;  // in the order they were added
    uint64_t total = 0;            // entries of all of them
    const LutTable *find(int U, int l) const {
        for (const LutTable &t : tables)
            if (t.U == U && t.l == l) return &t;
        return nullptr;
    }
};
// the (U, l) a launch (L, ph) unranks variable (m candidates, z: variable 0
// among them) with; false: the variable has no set in that launch
inline bool lut_pair(int m, bool z, int L, int ph, int &U, int &l) {
    if (ph == 0 && !z) return false;
    U = (ph == 0 || z) ? m - 1 : m;
    l = ph == 0 ? L - 1 : L;
    return l >= 0 && l <= U;
}

// Everything ulg_cbic_score derives from the lists before its first launch.
// A layer L >= 1 runs as two launches (score_calculator.cpp:78-123): phase 0
// scores the sets that hold compact index 0 when that is variable 0, phase 1
// the rest.  One object lives in the context and is rebuilt per call, so its
// vectors keep their capacity.
struct CbicPlan {
    int nv = 0, kmax = 0;
    std::vector<int> meta;        // [nv][4]: variable, m, var0in, pad
    size_t wstride = 0;           // words of one [L][phase][nv + 1] prefix family
    std::vector<uint64_t> work;   // [L][phase][nv + 1] set prefixes of each launch
    // tables of 2^30 slots or more: the one-pass form with 64-bit slots (the
    // others keep 32-bit byte offsets in their gathers and slots in entries)
    int variant = 0;
    // Variables never read each other's slabs, so they are striped over G
    // groups on concurrent streams: a group's latency-bound walk kernels
    // overlap the other groups' scoring kernels.  Diagnostics run on one.
    int G = 1;
    std::vector<uint64_t> workg;  // G > 1: [g][L][phase][nv + 1], variables outside group g count 0 sets
    uint64_t qwords = 0;   // per group: every lane of its largest launch may be queued
    uint64_t wqwords = 0;  // the same for the wide layers' queue (3 words per set, entries + straggler copies)
    // walk-queue segment counters per (group, layer, phase) of the unrolled
    // two-pass launches (queue_walk), kSegStride words each, then a
    // walk_bucket header at layers 5 and 6
    std::vector<uint64_t> segoff;  // [G * 2 * (kmax + 1) + 1]
    size_t nqc = 0;  // queue counters per (group, layer, phase), then the wide walks' error flag
    // bucketed walk launches (walk_bucket, layers 5 and 6): per stream group a
    // key/rank word and a sorted index per queue entry, the (key, segment)
    // offsets and the wave table
    bool bucket = false;
    uint64_t qcap = 0;      // queue entries per group (an entry is >= 3 words), 256-aligned
    uint64_t nseg_max = 1;  // most segments of a layer-5/6 launch
    uint64_t wave_cap = 0;  // walk waves of a bucketed launch, at most
    bool zero_q = false;    // the prologue zeroes the counters
    uint64_t nqseg = 0;     // ... this many segment-counter words
    // wide-layer walks: one checked-bitset slice per stream group (2^q bits
    // per walking set, q <= kmax + 1)
    uint64_t wslice = 0;
    std::vector<uint64_t> hoff;  // [nv] hi-cover table offsets (~0: none); empty without tables
    uint64_t htot = 0;
    // Small layers (L <= Ls, little work, latency-bound): one one-pass launch
    // per phase over all variables on the context stream -- no queue, no walk
    // launch, no stream groups.  The rest: per group, score + queued walk.
    int Ls = 0;
    int vsmall = 0;  // the one-pass form (keeping the subset maxima under bit 6)
    // ... of which layers <= Lf in one launch, a workgroup per variable
    // (not under -r: the budget is checked after every layer, and a fused
    // launch would finish layers 2..Lf before the first check)
    int Lf = 0;
    // The wide layers variable by variable (wide_pool 1) pay when the
    // variables that reach them differ in size: the long replays of one then
    // hold no other's next layer (C4: 2-hop sets of 10..18 candidates).  On
    // equal candidate sets (C1: a full skeleton) the grouped form's larger
    // launches keep more replays in flight (C1 at lambda 0.5: 10.7 s against
    // 15.2 s).  wide_pool 2 (default) picks the pool when the wide variables'
    // candidate counts span at least 2.  The pool needs G > 1 and no -r.
    bool use_pool = false;
    std::vector<int> pool_order;  // its tasks: the wide variables, largest candidate sets first
    std::vector<uint64_t> vw;     // [task][L][phase][nv + 1] launch prefixes, only the task's variable counts
    int64_t nb = 0;               // compaction blocks
    // the call's constraint table: the alternatives of the scored variables in
    // their compact candidate numbering (cbic_layer_dev.h cons_violates)
    std::vector<uint64_t> ct;
    int cons_words = 0;  // 0: the call runs the unconstrained kernels
    int cons_lds = 0;    // bytes of LDS the constrained kernels add

    // unrank tables: per launch (L, ph) and variable the offset of its table
    // in the context's cache, -1 = the lanes compute; lut_new = the tables
    // this call added to the cache, to be filled before its first launch
    std::vector<int32_t> lutoff;  // [(L * 2 + ph) * nv + vi]; empty when no launch has a table
    std::vector<LutTable> lut_new;
    bool lut_any = false;
    size_t lut_offset(int L, int ph) const { return ((size_t)L * 2 + ph) * nv; }

    // Narrow launches (option score_narrow): the form of the
    // layer kernels whose set masks, ranks, launch-local indices and slots
    // are 32-bit.  A launch takes it when the form exists for its (layer,
    // variant) and, whichever lane looks, no value can need a 33rd bit: every
    // variable listed in the launch's tables -- all of the call's, whichever
    // stream group scores them -- has at most 32 candidates (a compact mask,
    // shifted left by one for variable 0 or not, ends at bit 31; a lane
    // without an unrank table computes a mask over U <= 32), the launch's
    // sets plus one block of lanes past them fit 32 bits, and every table
    // slot is below 2^30 (the gathers' 32-bit byte offsets).  Anything else
    // runs the 64-bit kernel.
    static constexpr bool narrow_built(int L, int variant) { return variant == 241 && (L == 5 || L == 6); }
    static constexpr bool narrow_fits(int max_m, uint64_t sets, uint64_t total_slots) {
        return max_m <= 32 && sets <= (1ull << 32) - (uint64_t)kBlock && (total_slots >> 30) == 0;
    }
    std::vector<uint8_t> narrow;  // [seg_slot(g, L, ph)] 1: the launch runs the narrow form
    int narrow_launches = 0;      // launches of this call that do
    bool launch_narrow(int g, int L, int ph) const { return !narrow.empty() && narrow[seg_slot(g, L, ph)] != 0; }

    // After build(): which tables the call's layer launches read.  A table
    // exists for U <= kLutMaxU and 0 < C(U, l) <= cap, while the cache stays
    // within int32 offsets; it is added to `cache` the first time any call
    // needs it (variables, then layers, then phases, in order).
    void build_luts(const ScoreLists &ls, int64_t cap, LutCache &cache) {
        lutoff.clear();
        lut_new.clear();
        lut_any = false;
        const int top = std::min(kmax, kMaxL);
        if (cap <= 0 || top < kLutMinL) return;
        lutoff.assign((size_t)(kmax + 1) * 2 * nv, -1);
        for (int i = 0; i < nv; ++i)
            for (int L = kLutMinL; L <= top; ++L)
                for (int ph = 0; ph < 2; ++ph) {
                    int U, l;
                    if (!lut_pair(ls.mv[i], meta[i * 4 + 2] != 0, L, ph, U, l) || U > kLutMaxU) continue;
                    const uint64_t cnt = binom64(U, l);
                    if (cnt == 0 || cnt > (uint64_t)cap) continue;
                    const LutTable *t = cache.find(U, l);
                    if (!t) {
                        if (cache.total + cnt > kLutMaxTotal) continue;
                        cache.tables.push_back(LutTable{U, l, cache.total, cnt});
                        cache.total += cnt;
                        lut_new.push_back(cache.tables.back());
                        t = &cache.tables.back();
                    }
                    lutoff[lut_offset(L, ph) + i] = (int32_t)t->off;
                    lut_any = true;
                }
        if (!lut_any) lutoff.clear();
    }

    // Launch images (option score_lds_image).  Every block of a layer launch
    // (score_layer_kernel and its constrained twin) fills the same constants
    // into LDS before its first barrier; the image of launch (g, L, ph) is
    // those bytes, LDS [0, lay.stack) exactly as lds_layout places them --
    // the Gram matrix, the binomials, the launch's work prefixes and unrank
    // offsets, the slab offsets, the metadata and the candidate lists, the
    // alignment gaps and the aliased carve's counters zero -- so the block
    // copies one flat run of 16-byte pieces.  lay.stack is a multiple of 16.
    // Images lie back to back in `image`; imgoff holds their byte offsets.
    std::vector<unsigned char> image;
    std::vector<int64_t> imgoff;  // [seg_slot(g, L, ph)] -1: the launch has no image
    bool image_any = false;
    int64_t image_offset(int g, int L, int ph) const { return image_any ? imgoff[seg_slot(g, L, ph)] : -1; }
    // the variant a layer launch runs with, and its work prefixes
    int launch_variant(int L) const { return L <= Ls ? vsmall : variant; }
    const uint64_t *launch_work(int g, int L, int ph) const {
        return L <= Ls ? &work[work_offset(0, L, ph)] : &group_work()[work_offset(g, L, ph)];
    }
    int image_bytes(const ScoreLists &ls, int L) const { return lds_layout(ls.n, nv, ls.S, L, launch_variant(L)).stack; }

    // After build() and build_luts(): gram = the n x n Gram matrix of the
    // loaded data, binom = the clamped [64][kBinomK] table.  A small layer
    // (Lf < L <= Ls) is one launch of all variables, group 0's.
    void build_images(const ScoreLists &ls, const double *gram, const uint32_t *binom, bool on) {
        image.clear();
        imgoff.clear();
        image_any = false;
        const int top = std::min(kmax, kMaxL);
        if (!on || !gram || !binom || top <= Lf) return;
        imgoff.assign((size_t)G * 2 * (kmax + 1), -1);
        const int n = ls.n, S = ls.S;
        for (int L = Lf + 1; L <= top; ++L)
            for (int ph = 0; ph < 2; ++ph)
                for (int g = 0; g < (L <= Ls ? 1 : G); ++g) {
                    const uint64_t *w = launch_work(g, L, ph);
                    if (w[nv] == 0) continue;
                    const LdsLayout lay = lds_layout(n, nv, S, L, launch_variant(L));
                    const size_t at = image.size();
                    image.resize(at + (size_t)lay.stack, 0);
                    unsigned char *im = image.data() + at;
                    std::memcpy(im + lay.gram, gram, (size_t)n * n * 8);
                    std::memcpy(im + lay.binom, binom, (size_t)64 * kBinomK * 4);
                    std::memcpy(im + lay.work, w, (size_t)(nv + 1) * 8);
                    if (lut_any) std::memcpy(im + lay.lutoff, &lutoff[lut_offset(L, ph)], (size_t)nv * 4);
                    std::memcpy(im + lay.toff, ls.toff.data(), ((size_t)nv * S + 1) * 8);
                    std::memcpy(im + lay.meta, meta.data(), (size_t)nv * 16);
                    std::memcpy(im + lay.cand, ls.cand.data(), (size_t)nv * 64);
                    imgoff[seg_slot(g, L, ph)] = (int64_t)at;
                    image_any = true;
                }
    }

    size_t work_offset(int g, int L, int ph) const {
        return (size_t)g * (G > 1 ? wstride : 0) + ((size_t)L * 2 + ph) * (nv + 1);
    }
    const std::vector<uint64_t> &group_work() const { return G > 1 ? workg : work; }
    // sets of stream group g's launch (L, ph)
    uint64_t launch_count(int g, int L, int ph) const { return group_work()[work_offset(g, L, ph) + nv]; }
    size_t seg_slot(int g, int L, int ph) const { return (size_t)g * 2 * (kmax + 1) + (size_t)L * 2 + ph; }
    size_t hmeta_stride() const { return nv + (size_t)(nv + 1) * 8; }

    void build(const ScoreLists &ls, const std::vector<int> &cons_var, const std::vector<uint64_t> &cons_req,
               const std::vector<uint64_t> &cons_forb, const Options &o, bool wck) {
        // wck: ULG_WALK_CLOCK diagnostics (synchronising, one stream)
        nv = ls.nv;
        kmax = ls.kmax;
        const std::vector<int> &mv = ls.mv;
        const int max_parents = ls.max_parents;
        meta.assign((size_t)nv * 4, 0);
        for (int i = 0; i < nv; ++i) {
            meta[i * 4 + 0] = ls.vars[i];
            meta[i * 4 + 1] = mv[i];
            meta[i * 4 + 2] = (ls.cmask[i] & 1ull) ? 1 : 0;  // variable 0 is a candidate (compact index 0)
        }
        wstride = (size_t)(kmax + 1) * 2 * (nv + 1);
        work.assign(wstride, 0);
        for (int L = 1; L <= kmax; ++L)
            for (int ph = 0; ph < 2; ++ph) {
                uint64_t *w = &work[((size_t)L * 2 + ph) * (nv + 1)];
                uint64_t s = 0;
                for (int i = 0; i < nv; ++i) {
                    w[i] = s;
                    const bool z = meta[i * 4 + 2] != 0;
                    if (ph == 0) s += z ? binom64(mv[i] - 1, L - 1) : 0;
                    else s += z ? binom64(mv[i] - 1, L) : binom64(mv[i], L);
                }
                w[nv] = s;
            }
        build_constraints(ls, cons_var, cons_req, cons_forb);

        variant = (ls.total_slots >> 30) ? 1 : (int)o.score_variant;
        G = ((variant & 16) && !wck) ? std::max(1, std::min((int)o.score_streams, nv)) : 1;
        workg.assign(G == 1 ? 0 : (size_t)G * wstride, 0);
        for (int g = 0; g < G && G > 1; ++g)
            for (int L = 1; L <= kmax; ++L)
                for (int ph = 0; ph < 2; ++ph) {
                    const uint64_t *w = &work[((size_t)L * 2 + ph) * (nv + 1)];
                    uint64_t *wg = &workg[work_offset(g, L, ph)];
                    uint64_t acc = 0;
                    for (int i = 0; i < nv; ++i) {
                        wg[i] = acc;
                        if (i % G == g) acc += w[i + 1] - w[i];
                    }
                    wg[nv] = acc;
                }
        qwords = wqwords = 0;
        nseg_max = 1;
        const size_t nseg_slots = (size_t)G * 2 * (kmax + 1);
        segoff.assign(nseg_slots + 1, 0);
        for (int g = 0; g < G; ++g)
            for (int L = 0; L <= kmax; ++L)
                for (int ph = 0; ph < 2; ++ph) {
                    const uint64_t cnt = launch_count(g, L, ph);
                    const uint64_t nseg = seg_count((cnt + kBlock - 1) / kBlock);
                    const bool queued = L >= 1 && L <= kMaxL && (variant & 16);
                    const bool bhdr = queued && (L == 5 || L == 6);  // room for a walk_bucket header
                    if (L > kMaxL) wqwords = std::max<uint64_t>(wqwords, 6 * cnt);
                    else if (queued) qwords = std::max<uint64_t>(qwords, nseg * kSegEntries * (uint64_t)(1 + 2 * bits_words(L)));
                    if (L == 5 || L == 6) nseg_max = std::max<uint64_t>(nseg_max, nseg);
                    const size_t i = seg_slot(g, L, ph);
                    segoff[i + 1] = segoff[i] + (queued ? nseg * kSegStride : 0) + (bhdr && cnt ? kBucketHdrWords : 0);
                }
        nqc = nseg_slots + 1;
        bucket = (variant & 112) == 112 && o.walk_bucket && !wck && kmax >= 5;  // the CMP path queues with keys
        qcap = (qwords / 3 + 255) & ~255ull;
        wave_cap = qcap / 64 + kBucketMax;
        zero_q = (variant & 16) || kmax > kMaxL;
        nqseg = zero_q ? std::max<uint64_t>(segoff.back(), 1) : 0;

        wslice = htot = 0;
        hoff.clear();
        if (kmax > kMaxL) {
            const uint64_t wpl_max = kmax + 1 <= 6 ? 1ull : (1ull << (kmax + 1 - 6));
            wslice = std::max<uint64_t>(kWideBitsWords / (uint64_t)G, wpl_max);
            // hi-cover tables for the variables that reach a wide layer
            if (o.wide_prune) {
                hoff.assign(nv, ~0ull);
                for (int i = 0; i < nv; ++i)
                    if (std::min(mv[i], max_parents) > kMaxL && mv[i] <= kHiMaxBits) {
                        hoff[i] = htot;
                        htot += 1ull << mv[i];
                    }
                if (htot == 0) hoff.clear();
            }
        }
        Ls = (variant & 16) && !wck ? std::min(kmax, std::min(kMaxL, (int)o.score_small_layers)) : 0;
        vsmall = variant & 65;
        Lf = vsmall == 65 && o.time_limit_ms == 0 ? std::min(Ls, (int)o.score_fused) : 0;
        narrow.assign(nseg_slots, 0);
        narrow_launches = 0;
        int max_m = 0;
        for (int i = 0; i < nv; ++i) max_m = std::max(max_m, mv[i]);
        for (int g = 0; g < G && o.score_narrow; ++g)
            for (int L = Ls + 1; L <= std::min(kmax, kMaxL); ++L)
                for (int ph = 0; ph < 2; ++ph) {
                    const uint64_t cnt = launch_count(g, L, ph);
                    if (cnt == 0 || !narrow_built(L, variant) || !narrow_fits(max_m, cnt, ls.total_slots)) continue;
                    narrow[seg_slot(g, L, ph)] = 1;
                    ++narrow_launches;
                }
        build_pool(ls, o);
        nb = (int64_t)((ls.total_slots + kSlotsPerBlock - 1) / kSlotsPerBlock);
    }

private:
    void build_constraints(const ScoreLists &ls, const std::vector<int> &cons_var,
                           const std::vector<uint64_t> &cons_req, const std::vector<uint64_t> &cons_forb) {
        ct.clear();
        cons_words = cons_lds = 0;
        if (cons_var.empty()) return;
        ct.assign((size_t)nv + 1, 0);
        for (int i = 0; i < nv; ++i) {
            ct[i] = (ct.size() - (size_t)(nv + 1)) / 2;
            const uint64_t C = ls.cmask[i];
            auto compact = [&](uint64_t mask) {
                uint64_t out = 0;
                for (int k = 0; k < ls.mv[i]; ++k)
                    if ((mask >> ls.cand[(size_t)i * 64 + k]) & 1ull) out |= 1ull << k;
                return out;
            };
            bool any = false, kept = false;
            for (size_t j = 0; j < cons_var.size(); ++j) {
                if (cons_var[j] != ls.vars[i]) continue;
                any = true;
                if (cons_req[j] & ~C) continue;  // requires a non-candidate (or the variable itself)
                kept = true;
                ct.push_back(compact(cons_req[j]));
                ct.push_back(compact(cons_forb[j]));
            }
            if (any && !kept) {  // every set of this variable violates
                ct.push_back(1ull << 63);
                ct.push_back(0);
            }
        }
        ct[nv] = (ct.size() - (size_t)(nv + 1)) / 2;
        if (ct[nv] == 0) return;
        cons_words = (int)ct.size();
        cons_lds = cons_words <= kConsLdsWords ? cons_words * 8 : 0;
    }

    void build_pool(const ScoreLists &ls, const Options &o) {
        const std::vector<int> &mv = ls.mv;
        pool_order.clear();
        vw.clear();
        use_pool = o.wide_pool == 1;
        if (o.wide_pool == 2) {
            int lo_m = 64, hi_m = -1;
            for (int i = 0; i < nv; ++i)
                if (std::min(mv[i], ls.max_parents) > kMaxL) {
                    lo_m = std::min(lo_m, mv[i]);
                    hi_m = std::max(hi_m, mv[i]);
                }
            use_pool = hi_m >= 0 && hi_m - lo_m >= 2;
        }
        use_pool = use_pool && kmax > kMaxL && G > 1 && o.time_limit_ms == 0;
        if (!use_pool) return;
        for (int i = 0; i < nv; ++i)
            if (std::min(mv[i], ls.max_parents) > kMaxL) pool_order.push_back(i);
        std::stable_sort(pool_order.begin(), pool_order.end(), [&](int a, int b) { return mv[a] > mv[b]; });
        vw.assign(pool_order.size() * wstride, 0);
        for (size_t k = 0; k < pool_order.size(); ++k) {
            const int i = pool_order[k];
            for (int L = kMaxL + 1; L <= kmax; ++L)
                for (int ph = 0; ph < 2; ++ph) {
                    const uint64_t *w = &work[((size_t)L * 2 + ph) * (nv + 1)];
                    uint64_t *out = &vw[k * wstride + ((size_t)L * 2 + ph) * (nv + 1)];
                    const uint64_t cnt = w[i + 1] - w[i];
                    for (int j = 0; j <= nv; ++j) out[j] = j > i ? cnt : 0;
                }
        }
    }
};

}  // namespace ulg
