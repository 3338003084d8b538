// cbic_wide.hip -- the wide layers of the cBIC scorer (kMaxL < L <= kWideMax):
// runtime-L scoring and walk kernels, the long walks' LDS replay, the
// hi-cover tables, the host replay, and the grouped and pooled launches.
// See cbic.hip for the design and cbic_call.h for the file map.
#include <cstdio>
#include <atomic>
#include <thread>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "search_internal.h"
#include "host_walk.h"
#include "cbic_call.h"

using namespace ulg;

namespace {

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

}  // namespace

namespace ulg {

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

}  // namespace ulg
