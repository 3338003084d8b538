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
//
// This file is the scoring call: plan, buffers, prologue, the order of the
// layers' launches, compaction, graph capture and the C ABI.  The kernels and
// their launches by family: cbic_gram.hip (load), cbic_layers.hip and
// cbic_layers_cons.hip (layers 1..8), cbic_walk.hip (their queued walks),
// cbic_wide.hip (layers 9..31); what they share: cbic_call.h, cbic_layer_dev.h.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>

#include "search_internal.h"
#include "cbic_call.h"

using namespace ulg;

namespace {

// out[r] = unrank_colex(r, l, U) for r < count = C(U, l): a context's unrank
// table (score_plan.h LutCache), equal to the computed mapping by construction.
// Beside reserve_luts, its only launcher.
__global__ void __launch_bounds__(kBlock) unrank_lut_fill_kernel(uint32_t *out, uint32_t count, int l, int U,
                                                                 const uint32_t *binom) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r < count) out[r] = (uint32_t)unrank_colex(r, l, U, binom);
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
                 (uint64_t)sliced_k(5, ~0ull, 0, (int)c->opt.walk_k6),
                 (uint64_t)sliced_k(6, ~0ull, 0, (int)c->opt.walk_k6)});
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

}  // extern "C"
