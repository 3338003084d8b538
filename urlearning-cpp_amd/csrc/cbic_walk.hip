// cbic_walk.hip -- the walks of the sets an unrolled layer launch queued (the
// two-pass variants): the bit-sliced walk in queue order and the bucketed
// walk sorted by walk key, with their launches and diagnostics.
// See cbic.hip for the design and cbic_call.h for the file map.
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>


#include "search_internal.h"
#include "cbic_call.h"

using namespace ulg;

namespace {

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
constexpr int kSlicedKSmall = 2;  // default sets per lane up to layer 5 (layer 6: option walk_k6, 4)

}  // namespace

namespace ulg {

// A layer-6 launch of fewer than `small` sets (the shares of 4 and 8 ranks,
// where a stream group holds one or two variables) walks one set per lane:
// its few waves then each walk a quarter of the union tree, and the launch
// ends with its longest wave (C3 8-rank share 0.80 -> 0.73 ms; the one-GPU
// launches keep the wide union, best there, `profiles/r4/`).
int sliced_k(int L, uint64_t cnt, uint64_t small, int k6) {
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

}  // namespace ulg

namespace {

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

}  // namespace

namespace ulg {

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
    const SlicedFn fn = sliced_fn(L, ph, wk);
    if (!fn) return ULG_OK;  // no bit-sliced walk at this layer
    const int kk = L == 7 ? 2 : (L == 8 ? 1 : wk);
    const uint64_t per = 64ull * (uint64_t)kk;
    const uint64_t sb = seg_count(blocks) * ((kSegEntries + per - 1) / per);
    int rc;
    if (wck && (rc = ensure(c, c->d_dump, (size_t)3 * sb))) return rc;
    if (wck) ULG_HIP(c, hipMemsetAsync(c->d_dump.p, 0, 24 * sb, st));
    prof_begin_s(c, kWalkNames[ph][L], st);
    hipLaunchKernelGGL(fn, dim3((unsigned)sb), dim3(64), 0, st, sa.queue, sa.qcount, c->table.p,
                       sa.hsub_out ? sa.hsub : nullptr, wck ? c->d_dump.p : nullptr, k.ls.total_slots, sa.err);
    prof_end_s(c, st);
    if (wck && (rc = dump_walk_clock(c, st, sb, wck, L, ph))) return rc;
    if (wck && std::getenv("ULG_WALK_QUEUE_DUMP") &&
        (rc = dump_walk_queue(c, st, sa.queue, sa.qcount, seg_count(blocks), bits_words(L), k.ls.total_slots, wck, L,
                              ph)))
        return rc;
    return ULG_OK;
}

#ifdef ULG_GATHER_STATS
// diagnostic build: the walk's hits by depth (2 * (kMaxL + 1) * 16 values), zeroed
int walk_hit_stats(ulg_ctx *c, unsigned long long *out) {
    static const unsigned long long zero[2 * (kMaxL + 1) * 16] = {};
    ULG_HIP(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wstats), sizeof(g_wstats)));
    ULG_HIP(c, hipMemcpyToSymbol(HIP_SYMBOL(g_wstats), zero, sizeof(zero)));
    return ULG_OK;
}
#endif

}  // namespace ulg
