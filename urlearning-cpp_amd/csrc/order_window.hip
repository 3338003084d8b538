// order_window.hip -- exact window re-optimisation of orders over the
// per-variable lists (ulg_order_window; contract: include/ulg.h, "Order
// search").  w consecutive positions of an order are replaced by the best of
// their w! arrangements, found by the subset DP over the window's 2^w subsets:
// the sliding-window move of the order-based literature in its exact form.  It
// reads the lists of the last ulg_order_search_begin* (the order MCMC's device
// copy, OrderMcmcState) and the run buffers of OrderSearchState; the searches'
// own state is not touched.
//
// owindow_kernel<W>: one workgroup of W waves per order, every sweep of the call.
//   static LDS   the order, the predecessor masks, the terms by position, the
//                variable -> local bit table, the window's variables, lists and
//                the prefix of their scatter items
//   dynamic LDS  F[2^w] doubles | T_j[2^(w-1)] words, j < w | c[2^w] bytes
//                (ow_lds_bytes: 137 KB at w = 12)
// A window:
//   setup    lane j < w: x_j, its local bit, its list; T cleared;  barrier
//   scatter  the w lists as one pool of items of kWindowChunk entries: the waves
//            stride the items, the lanes the entries (8 B set, 4 B score,
//            coalesced).  A compatible entry's image is max-combined into
//            T_j[squeeze_j(local mask)] by a 32-bit LDS atomic max, skipped
//            when the word already holds as much;  barrier
//   subset   w - 1 butterfly rounds over all T_j, a lane per pair;  barrier each
//   DP       layer by layer by |M|, a lane per mask (ow_dp_mask); a layer reads
//            the one below;  barrier each
//   accept   every lane sums the present terms and compares; one lane walks
//            back (ow_backtrack) and rewrites order, masks and terms;  barrier
// The terms a window writes are maxima of float32 images, the sums fixed FP64
// expressions: no output depends on W, on the grid or on the number of orders.
// After the last sweep wave_best gives every position's term and chosen set, as
// ulg_order_best does.  A launch is bounded (max_sweeps sweeps of at most n
// windows); plain vector stores and LDS atomics only; no global atomics, no
// communication between workgroups.
#include <algorithm>
#include <cstdio>

#include "order_search_state.h"
#include "order_window_dev.h"

using namespace ulg;

namespace {

constexpr int kWave = kSearchWave;
constexpr uint64_t kGridX = 1ull << 20;

struct WindowArgs {
    const uint64_t *sets;
    const float *scores;
    const int64_t *offsets;
    uint8_t *orders;  // [count][n] in and out
    double *terms;    // [count][n]
    uint64_t *parents;  // [count][n], or null
    double *score;    // [count]
    long long *accepted, *sweeps;  // [count]
    int n, w, stride;
    int64_t count, max_sweeps;
};

template <int W>
__global__ void __launch_bounds__(kWave *W) owindow_kernel(const WindowArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint8_t ord[kWave], bit[kWave], xs[kWindowMaxWidth], nvar[kWindowMaxWidth];
    __shared__ uint64_t pre[kWave];
    __shared__ double term[kWave], nterm[kWindowMaxWidth];
    __shared__ int64_t lb[kWindowMaxWidth], le[kWindowMaxWidth];  // the window's lists
    __shared__ uint32_t items[kWindowMaxWidth + 1];               // the prefix of their items
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int n = a.n, w = a.w;
    const int64_t k = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (k >= a.count) return;  // the whole workgroup
    double *F = reinterpret_cast<double *>(smem);
    uint32_t *T = reinterpret_cast<uint32_t *>(smem + ((size_t)8 << w));
    uint8_t *cc = reinterpret_cast<uint8_t *>(T + ow_table_words(w));
    const uint32_t full = (1u << w) - 1u, half = 1u << (w - 1), words = ow_table_words(w);

    if (tid < kWave) bit[tid] = kWindowOutside;
    if (tid < n) ord[tid] = a.orders[k * n + tid];
    __syncthreads();
    if (tid < n) {
        uint64_t U = 0;
        for (int q = 0; q < tid; ++q) U |= 1ull << ord[q];
        pre[tid] = U;
    }
    __syncthreads();
    for (int p = wave; p < n; p += W) {
        const int v = ord[p];
        const OsBest r = os_decode(wave_best(a.sets, a.scores, a.offsets[v], a.offsets[v + 1], pre[p], lane));
        if (lane == 0) term[p] = r.b;
    }
    __syncthreads();

    long long accepted = 0, sweeps = 0;
    while (sweeps < a.max_sweeps) {
        ++sweeps;
        bool any = false;
        for (int s = 0;; s = ow_next_start(s, a.stride, n, w)) {
            // setup
            if (wave == 0) {
                uint32_t sum = 0;
                if (lane < w) {
                    const int v = ord[s + lane];
                    const int64_t b = a.offsets[v], e = a.offsets[v + 1];
                    xs[lane] = (uint8_t)v, bit[v] = (uint8_t)lane;
                    lb[lane] = b, le[lane] = e;
                    sum = (uint32_t)((e - b + kWindowChunk - 1) / kWindowChunk);  // a list holds at most 2^32 - 1 entries
                }
                for (int d = 1; d < 16; d <<= 1) {
                    const uint32_t o = __shfl_up(sum, d, kWave);
                    if (lane >= d) sum += o;
                }
                if (lane < w) items[lane + 1] = sum;
                if (lane == 0) items[0] = 0u, F[0] = 0.0, cc[0] = 0;
            }
            for (uint32_t i = tid; i < words; i += kWave * W) T[i] = 0u;
            __syncthreads();
            // scatter
            const uint64_t U = pre[s];
            uint64_t V = 0;
            for (int j = 0; j < w; ++j) V |= 1ull << xs[j];
            for (uint32_t item = wave, j = 0; item < items[w]; item += W) {
                while (items[j + 1] <= item) ++j;
                const uint64_t outside = ~(U | (V & ~(1ull << xs[j])));
                const int64_t b = lb[j] + (int64_t)(item - items[j]) * kWindowChunk, e = b + kWindowChunk < le[j] ? b + kWindowChunk : le[j];
                uint32_t *t = T + j * half;
#pragma unroll 4
                for (int64_t i = b + lane; i < e; i += kWave) {
                    const uint64_t S = a.sets[i];
                    const uint32_t image = os_float_image(__float_as_uint(a.scores[i]));
                    if (S & outside) continue;
                    uint32_t *cell = t + ow_squeeze(ow_local_mask(S & V, bit), (int)j);
                    if (*cell < image) atomicMax(cell, image);
                }
            }
            __syncthreads();
            // subset-max
            for (int r = 0; r + 1 < w; ++r) {
                for (uint32_t q = tid; q < (uint32_t)w * (half >> 1); q += kWave * W) ow_butterfly(T, w, r, q);
                __syncthreads();
            }
            // DP
            for (int layer = 1; layer <= w; ++layer) {
                for (uint32_t M = tid; M <= full; M += kWave * W)
                    if (__popc(M) == layer) ow_dp_mask(M, w, T, F, cc);
                __syncthreads();
            }
            // accept
            const bool take = F[full] > ow_sum(term + s, w);
            __syncthreads();  // every lane has read the present terms
            if (take) {
                if (tid == 0) {
                    ow_backtrack(w, T, cc, xs, nvar, nterm);
                    for (int q = 0; q < w; ++q) {
                        ord[s + q] = nvar[q], term[s + q] = nterm[q];
                        if (q) pre[s + q] = pre[s + q - 1] | (1ull << nvar[q - 1]);
                    }
                }
                ++accepted;
                any = true;
            }
            if (tid < w) bit[xs[tid]] = kWindowOutside;
            __syncthreads();
            if (s == n - w) break;
        }
        if (!any) break;
    }

    const double S = ow_sum(term, n);
    for (int p = wave; p < n; p += W) {
        const int v = ord[p];
        const int64_t b = a.offsets[v];
        const OsBest r = os_decode(wave_best(a.sets, a.scores, b, a.offsets[v + 1], pre[p], lane));
        if (lane == 0) {
            a.terms[k * n + p] = r.b;
            if (a.parents) a.parents[k * n + v] = r.ent == kSearchNoEntry ? 0ull : a.sets[b + r.ent];
        }
    }
    if (tid < n) a.orders[k * n + tid] = ord[tid];
    if (tid == 0) a.score[k] = S, a.accepted[k] = accepted, a.sweeps[k] = sweeps;
}

template <int W>
int launch_window(ulg_ctx *c, const WindowArgs &a, size_t lds, size_t limit) {
    hipFuncAttributes fa;
    ULG_HIP(c, hipFuncGetAttributes(&fa, (const void *)owindow_kernel<W>));
    if (fa.sharedSizeBytes + lds > limit) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "ulg_order_window: a window of %d positions needs %zu bytes of LDS, the device gives a workgroup %zu",
                      a.w, fa.sharedSizeBytes + lds, limit);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    ULG_HIP(c, hipFuncSetAttribute((const void *)owindow_kernel<W>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const uint64_t blocks = (uint64_t)a.count;
    const dim3 grid((unsigned)std::min<uint64_t>(blocks, kGridX), (unsigned)((blocks + kGridX - 1) / kGridX));
    prof_begin(c, "owindow");
    owindow_kernel<W><<<grid, kWave * W, lds, c->stream>>>(a);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    return ULG_OK;
}

}  // namespace

extern "C" int ulg_order_window(ulg_ctx *c, int64_t count, uint8_t *orders, int width, int stride, int64_t max_sweeps, double *terms,
                                double *score, uint64_t *parents, int64_t *accepted, int64_t *sweeps) {
    if (!c) return ULG_ERR_ARG;
    const std::string who = "ulg_order_window";
    OrderSearchState *sp = order_search_live(c);
    if (!sp) return set_err(c, ULG_ERR_STATE, who + ": no ulg_order_search_begin");
    OrderSearchState &s = *sp;
    const OrderMcmcState &l = *c->mcmc;
    const int n = s.n;
    if (width < kWindowMinWidth || width > kWindowMaxWidth) return set_err(c, ULG_ERR_ARG, who + ": width must be 2..12");
    if (stride < 0 || stride > width) return set_err(c, ULG_ERR_ARG, who + ": stride must be 0..width");
    if (max_sweeps < 1 || max_sweeps > kWindowMaxSweeps) return set_err(c, ULG_ERR_ARG, who + ": max_sweeps must be 1..2^20");
    if (count < 0 || (count > 0 && !orders)) return set_err(c, ULG_ERR_ARG, who + ": bad arguments");
    if (count > (int64_t)1 << 40) return set_err(c, ULG_ERR_ARG, who + ": count out of range");
    for (int64_t k = 0; k < count; ++k)
        if (!is_permutation(orders + k * n, n)) return set_err(c, ULG_ERR_ARG, who + ": order " + std::to_string(k) + " is not a permutation");
    if (count == 0) return ULG_OK;
    ULG_HIP(c, hipSetDevice(c->device));
    WindowArgs a;
    a.n = n, a.w = ow_width(width, n), a.stride = ow_stride(stride, width, a.w);
    a.count = count, a.max_sweeps = max_sweeps;
    int limit = 0;
    ULG_HIP(c, hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    const size_t cells = (size_t)count * (size_t)n;
    {
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        const double need = 17.0 * (double)cells + 24.0 * (double)count + 5 * 16.0 + 256.0, have = (double)free_b + (double)s.run_bytes();
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld orders of n = %d need %.0f bytes of device memory, %.0f are free", who.c_str(),
                          (long long)count, n, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    int rc;
    if ((rc = ensure(c, s.r_order, cells)) || (rc = ensure(c, s.r_terms, cells)) || (parents && (rc = ensure(c, s.r_parents, cells))) ||
        (rc = ensure(c, s.r_wscore, (size_t)count)) || (rc = ensure(c, s.r_wcount, 2 * (size_t)count)))
        return rc;
    a.sets = l.d_sets.p, a.scores = l.d_scores.p, a.offsets = l.d_offsets.p;
    a.orders = s.r_order.p, a.terms = s.r_terms.p, a.parents = parents ? s.r_parents.p : nullptr;
    a.score = s.r_wscore.p, a.accepted = s.r_wcount.p, a.sweeps = s.r_wcount.p + count;
    ULG_HIP(c, hipMemcpyAsync(s.r_order.p, orders, cells, hipMemcpyHostToDevice, c->stream));
    const size_t lds = ow_lds_bytes(a.w);
    switch (c->opt.window_waves) {
        case 1: rc = launch_window<1>(c, a, lds, (size_t)limit); break;
        case 2: rc = launch_window<2>(c, a, lds, (size_t)limit); break;
        case 4: rc = launch_window<4>(c, a, lds, (size_t)limit); break;
        case 16: rc = launch_window<16>(c, a, lds, (size_t)limit); break;
        default: rc = launch_window<8>(c, a, lds, (size_t)limit); break;
    }
    if (rc) {
        (void)hipStreamSynchronize(c->stream);  // the upload reads the caller's orders
        return rc;
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as they are");
    ULG_HIP(c, hipMemcpyAsync(orders, s.r_order.p, cells, hipMemcpyDeviceToHost, c->stream));
    if (terms) ULG_HIP(c, hipMemcpyAsync(terms, s.r_terms.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (score) ULG_HIP(c, hipMemcpyAsync(score, s.r_wscore.p, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    if (parents) ULG_HIP(c, hipMemcpyAsync(parents, s.r_parents.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (accepted) ULG_HIP(c, hipMemcpyAsync(accepted, s.r_wcount.p, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    if (sweeps) ULG_HIP(c, hipMemcpyAsync(sweeps, s.r_wcount.p + count, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ULG_OK;
}
