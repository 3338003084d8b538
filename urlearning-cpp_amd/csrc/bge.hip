// bge.hip -- BGe scoring of the continuous data (ulg_bge_*): the Bayesian
// Gaussian equivalent score (bge.h) of every parent set of a call, from the
// Gram matrix ulg_cbic_load left on the device.
//
// The reference has no continuous Bayesian score; this is the continuous
// counterpart of its BDeu (bdeu_scoring_function.cpp) behind the same list
// plumbing as ulg_disc_score: a slot table per call, the optional prune pass
// and the compaction (slot_table.h), so ulg_cbic_fetch, ulg_pss_format,
// ulg_search_from_scores and the searches read the lists unchanged.
//
// One lane per parent set.  bge_layer_kernel<L> takes a layer of all the
// call's variables: a block stages G, the constants and the binomials in LDS
// once, a lane unranks its set from the colex rank within its variable's
// layer over the variable's compact candidates, and bge_set_score (bge_dev.h)
// does the rest in FP64.  L = 1 .. 8 are fully unrolled with the factor in
// registers; the instance L = 0 takes the layer at run time and covers the
// empty sets and 9 .. 31 parents.  bge_sets_kernel scores arbitrary pairs
// with that same generic form.  There is no dominance walk, no hand-off
// between kernels and no atomic besides the compaction's.
//
// The store rule departs from score_calculator.cpp:59,111 (the empty set iff
// < 1, any other iff < 0): BGe is a log density and is positive as soon as the
// residual variance of normalised data falls below about 0.06, so every
// finite value is stored, the empty set included.  NaN (a constant column in
// the set, a pivot <= 0) is never stored; a set that violates
// ulg_cbic_set_constraints is not evaluated and never stored.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "bge.h"
#include "bge_dev.h"
#include "slot_table.h"
#include "ulg_internal.h"

using namespace ulg;

namespace {

constexpr int kBgeGridCap = 2048;  // blocks; a larger layer takes several passes of the grid

// The dynamic LDS of a layer block.  Lb = L + 1 binomial columns C(a, 0 .. L).
struct BgeLds {
    int g, tab, bin, work, base, vm, cand, total;
};
__host__ __device__ inline BgeLds bge_lds(int n, int nv, int Lb) {
    BgeLds o;
    o.g = 0;
    o.tab = o.g + n * n * 8;
    o.bin = o.tab + 2 * kBgeLayers * 8;
    o.work = o.bin + 64 * Lb * 8;
    o.base = o.work + (nv + 1) * 8;
    o.vm = o.base + nv * 8;
    o.cand = o.vm + nv * 2 * 4;
    o.total = (o.cand + nv * 64 + 15) & ~15;
    return o;
}

struct BgeLayerArgs {
    const double *gram;      // [n][n]
    const double *tab;       // [64]: c_l, A_l
    const uint8_t *cand;     // [nv][64] compact index -> variable
    const int *vm;           // [nv][2]: variable, candidate count
    const uint64_t *toff;    // [nv * S + 1] slot prefixes
    const uint64_t *work;    // [nv + 1] this layer's item prefixes
    const uint64_t *binom64; // [64][64]
    const uint64_t *cons;    // by variable, or null
    float *table;            // per slot: the stored value, or absent
    uint64_t *sets;          // per slot: the set's variable mask
    double t;
    int n, nv, S, L;
};

template <int LC>
__global__ void __launch_bounds__(kBgeBlock) bge_layer_kernel(BgeLayerArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int DM = BgeDim<LC>::kMax;
    constexpr int UN = BgeDim<LC>::kUnroll;
    const int L = LC > 0 ? LC : A.L;
    const int Lb = L + 1;
    const BgeLds o = bge_lds(A.n, A.nv, Lb);
    double *g = reinterpret_cast<double *>(smem + o.g);
    double *tab = reinterpret_cast<double *>(smem + o.tab);
    uint64_t *bin = reinterpret_cast<uint64_t *>(smem + o.bin);
    uint64_t *work = reinterpret_cast<uint64_t *>(smem + o.work);
    uint64_t *base = reinterpret_cast<uint64_t *>(smem + o.base);
    int *vm = reinterpret_cast<int *>(smem + o.vm);
    uint8_t *cand = smem + o.cand;
    for (int i = threadIdx.x; i < A.n * A.n; i += kBgeBlock) g[i] = A.gram[i];
    for (int i = threadIdx.x; i < 2 * kBgeLayers; i += kBgeBlock) tab[i] = A.tab[i];
    for (int i = threadIdx.x; i < 64 * Lb; i += kBgeBlock) bin[i] = A.binom64[(i / Lb) * 64 + i % Lb];
    for (int i = threadIdx.x; i <= A.nv; i += kBgeBlock) work[i] = A.work[i];
    for (int i = threadIdx.x; i < A.nv; i += kBgeBlock) base[i] = A.toff[(uint64_t)i * A.S + L];
    for (int i = threadIdx.x; i < 2 * A.nv; i += kBgeBlock) vm[i] = A.vm[i];
    for (int i = threadIdx.x; i < 64 * A.nv; i += kBgeBlock) cand[i] = A.cand[i];
    __syncthreads();
    const uint64_t total = work[A.nv];
    for (uint64_t w = (uint64_t)blockIdx.x * kBgeBlock + threadIdx.x; w < total; w += (uint64_t)gridDim.x * kBgeBlock) {
        // the variable: the last i with work[i] <= w (w < work[nv], so i < nv)
        int lo = 0, hi = A.nv;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (work[mid] <= w) lo = mid; else hi = mid;
        }
        const int i = lo;
        const uint64_t r0 = w - work[i];
        const int v = vm[2 * i], m = vm[2 * i + 1];
        // colex unrank over the variable's compact candidate indices: the
        // members come out descending, so q[] is ascending in the variable
        int q[DM];
        uint64_t pmask = 0, r = r0;
        int c = m - 1;
#pragma unroll UN
        for (int e = L; e >= 1; --e) {
            while (c > e - 1 && bin[c * Lb + e] > r) --c;
            r -= bin[c * Lb + e];
            const int p = cand[i * 64 + c];
            q[e - 1] = p;
            pmask |= 1ull << p;
            --c;
        }
        q[L] = v;
        const uint64_t slot = base[i] + r0;
        float val = __uint_as_float(kAbsentBits);
        if (!(A.cons && bge_violates(A.cons, A.n, v, pmask))) val = bge_set_score<LC>(g, A.n, q, L, A.t, tab);
        // every finite value is stored, whatever its sign
        A.table[slot] = isfinite(val) ? val : __uint_as_float(kAbsentBits);
        A.sets[slot] = pmask;
    }
}

// arbitrary (variable, parent mask) pairs: the generic form, NaN for a violator
__global__ void __launch_bounds__(kBgeBlock)
bge_sets_kernel(const double *gram, const double *tabg, const uint64_t *pairs, int64_t count, int n, double t,
                const uint64_t *cons, float *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *g = reinterpret_cast<double *>(smem);
    double *tab = g + n * n;
    for (int i = threadIdx.x; i < n * n; i += kBgeBlock) g[i] = gram[i];
    for (int i = threadIdx.x; i < 2 * kBgeLayers; i += kBgeBlock) tab[i] = tabg[i];
    __syncthreads();
    for (int64_t w = (int64_t)blockIdx.x * kBgeBlock + threadIdx.x; w < count; w += (int64_t)gridDim.x * kBgeBlock) {
        const int v = (int)pairs[2 * w];
        const uint64_t P = pairs[2 * w + 1];  // without v's bit, at most kWideMax members (the host checked)
        const int L = __builtin_popcountll(P);
        int q[BgeDim<0>::kMax];
        uint64_t rem = P;
        for (int j = 0; j < L; ++j) {
            q[j] = __builtin_ctzll(rem);
            rem &= rem - 1;
        }
        q[L] = v;
        float val = __uint_as_float(0x7fc00000u);
        if (!(cons && bge_violates(cons, n, v, P))) val = bge_set_score<0>(g, n, q, L, t, tab);
        out[w] = val;
    }
}

// The prior as it stands against the loaded n (ulg_bge_set_prior checked it
// against the n loaded then, if any).
int prior_check(ulg_ctx *c, const char *who) {
    if (!bge_alpha_mu_ok(c->bge_alpha_mu) || !bge_alpha_w_ok(c->bge_alpha_w, c->n))
        return set_err(c, ULG_ERR_ARG,
                       std::string(who) + ": the prior needs 1e-3 <= alpha_mu <= 1e3 and alpha_w = 0 or n + 1 < alpha_w <= n + 1e6");
    return ULG_OK;
}

// c_l and A_l of the loaded data and the prior, on the device (the source is a
// member of the context: it outlives the copy)
int upload_consts(ulg_ctx *c) {
    BgeConsts &K = c->bge_k;
    K = bge_consts(c->N, c->n, c->bge_alpha_mu, c->bge_alpha_w);
    int rc;
    if ((rc = ensure(c, c->d_bge_tab, (size_t)2 * kBgeLayers))) return rc;
    ULG_HIP(c, hipMemcpyAsync(c->d_bge_tab.p, K.tab, sizeof K.tab, hipMemcpyHostToDevice, c->stream));
    return ULG_OK;
}

template <int LC>
void launch_layer(ulg_ctx *c, unsigned grid, size_t lds, const BgeLayerArgs &A) {
    bge_layer_kernel<LC><<<grid, kBgeBlock, lds, c->stream>>>(A);
}

}  // namespace

extern "C" {

int ulg_bge_set_prior(ulg_ctx *c, double alpha_mu, double alpha_w) {
    if (!c) return ULG_ERR_ARG;
    const int n = (c->loaded || c->disc_loaded) ? c->n : 0;
    if (!bge_alpha_mu_ok(alpha_mu))
        return set_err(c, ULG_ERR_ARG, "ulg_bge_set_prior: alpha_mu must be finite, 1e-3 <= alpha_mu <= 1e3");
    if (!bge_alpha_w_ok(alpha_w, n))
        return set_err(c, ULG_ERR_ARG, "ulg_bge_set_prior: alpha_w must be 0 (the default n + alpha_mu + 1) or n + 1 < alpha_w <= n + 1e6");
    c->bge_alpha_mu = alpha_mu;
    c->bge_alpha_w = alpha_w;
    return ULG_OK;
}

int ulg_bge_score(ulg_ctx *c, const int *vars, int nv, const uint64_t *candidates, int max_parents,
                  int64_t *total_stored, int64_t *total_scored) {
    if (!c) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!c->loaded) return set_err(c, ULG_ERR_STATE, "ulg_bge_score: call ulg_cbic_load first");
    int rc;
    if ((rc = prior_check(c, "ulg_bge_score"))) return rc;
    ScoreLists &ls = c->lists;
    const ScoreLists::Status st = ls.build(c->n, vars, nv, candidates, max_parents);
    if (st != ScoreLists::kOk) return lists_error(c, "ulg_bge_score", st);
    const int kmax = ls.kmax, S = ls.S, n = c->n;
    const size_t lds_max = (size_t)bge_lds(n, nv, kmax + 1).total;
    if (lds_max > 64 * 1024) return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_bge_score: the layer block's LDS exceeds 64 KB");
    SlotTable tb;
    tb.build(ls);
    ULG_HIP(c, hipSetDevice(c->device));
    if ((rc = upload_consts(c)) || (rc = slot_table_begin(c, ls, tb))) return rc;
    const BgeConsts &K = c->bge_k;

    BgeLayerArgs A{};
    A.gram = c->gram.p;
    A.tab = c->d_bge_tab.p;
    A.cand = c->d_disc_cand.p;
    A.vm = c->d_disc_vm.p;
    A.toff = c->d_disc_meta.p;
    A.binom64 = c->d_binom64.p;
    A.cons = c->cons_var.empty() ? nullptr : c->d_cons_var.p;
    A.table = c->d_disc_table.p;
    A.sets = c->d_disc_sets.p;
    A.t = K.t;
    A.n = n;
    A.nv = nv;
    A.S = S;
    // -r: checked after every complete layer, as ulg_disc_score does
    const auto t_call = std::chrono::steady_clock::now();
    c->out_of_time = 0;
    int done_L = kmax;
    for (int L = 0; L <= kmax; ++L) {
        const uint64_t items = tb.items(L);
        if (items) {
            A.L = L;
            A.work = c->d_disc_meta.p + tb.work_at(L);
            const unsigned grid = (unsigned)std::min<uint64_t>((items + kBgeBlock - 1) / kBgeBlock, kBgeGridCap);
            const size_t lds = (size_t)bge_lds(n, nv, L + 1).total;
            prof_begin(c, "bge_layer");
            switch (L) {
                case 1: launch_layer<1>(c, grid, lds, A); break;
                case 2: launch_layer<2>(c, grid, lds, A); break;
                case 3: launch_layer<3>(c, grid, lds, A); break;
                case 4: launch_layer<4>(c, grid, lds, A); break;
                case 5: launch_layer<5>(c, grid, lds, A); break;
                case 6: launch_layer<6>(c, grid, lds, A); break;
                case 7: launch_layer<7>(c, grid, lds, A); break;
                case 8: launch_layer<8>(c, grid, lds, A); break;
                default: launch_layer<0>(c, grid, lds, A); break;  // no parents, and 9 .. 31
            }
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
    if (c->opt.bge_prune && (rc = slot_table_prune(c, tb, done_L))) return rc;
    unsigned long long word[kSlotWords];
    if ((rc = slot_table_compact(c, tb, word))) return rc;
    c->last_err_word = 0;
    c->bge_pruned = (int64_t)word[4];
    publish(c, ls, (int64_t)word[3], false);
    if (total_stored) *total_stored = c->total_stored;
    if (total_scored) *total_scored = c->total_scored;
    return ULG_OK;
}

int ulg_bge_score_sets(ulg_ctx *c, int64_t count, const int *vars, const uint64_t *parents, float *scores) {
    if (!c || count < 0 || (count > 0 && (!vars || !parents || !scores))) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!c->loaded) return set_err(c, ULG_ERR_STATE, "ulg_bge_score_sets: call ulg_cbic_load first");
    int rc;
    if ((rc = prior_check(c, "ulg_bge_score_sets"))) return rc;
    if (count == 0) return ULG_OK;
    const int n = c->n;
    const uint64_t allmask = (1ull << n) - 1ull;  // n <= 63
    std::vector<uint64_t> pairs((size_t)count * 2);
    for (int64_t i = 0; i < count; ++i) {
        if (vars[i] < 0 || vars[i] >= n) return set_err(c, ULG_ERR_ARG, "ulg_bge_score_sets: variable out of range");
        if (parents[i] & ~allmask) return set_err(c, ULG_ERR_ARG, "ulg_bge_score_sets: parent bit >= n");
        const uint64_t P = parents[i] & ~(1ull << vars[i]);
        if (__builtin_popcountll(P) > kWideMax)
            return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_bge_score_sets: more than ULG_MAX_PARENTS_GPU (31) parents");
        pairs[2 * i] = (uint64_t)vars[i];
        pairs[2 * i + 1] = P;
    }
    ULG_HIP(c, hipSetDevice(c->device));
    const BgeConsts &K = c->bge_k;
    if ((rc = upload_consts(c)) || (rc = ensure(c, c->d_sets_in, (size_t)count * 2)) ||
        (rc = ensure(c, c->qbuf_out, (size_t)count)))
        return rc;
    ULG_HIP(c, hipMemcpyAsync(c->d_sets_in.p, pairs.data(), (size_t)count * 16, hipMemcpyHostToDevice, c->stream));
    const unsigned grid = (unsigned)std::min<int64_t>((count + kBgeBlock - 1) / kBgeBlock, kBgeGridCap);
    const size_t lds = (size_t)(n * n + 2 * kBgeLayers) * 8;
    prof_begin(c, "bge_sets");
    bge_sets_kernel<<<grid, kBgeBlock, lds, c->stream>>>(c->gram.p, c->d_bge_tab.p, c->d_sets_in.p, count, n, K.t,
                                                        c->cons_var.empty() ? nullptr : c->d_cons_var.p, c->qbuf_out.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    ULG_HIP(c, hipMemcpyAsync(scores, c->qbuf_out.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));  // `pairs` is a pageable source
    prof_collect(c);
    return ULG_OK;
}

}  // extern "C"
