// posterior.hip -- exact model averaging over the order lattice (ulg_posterior,
// ulg_posterior_from_scores, ulg_posterior_table; contract: include/ulg.h).
// The sum-product counterpart of search.hip's subset-min transform and of
// search_gpu.hip's layer sweep: (min, +) on float costs becomes (logaddexp, +)
// on FP64 log-weights, plus a backward sweep, a superset transform and a
// gather.
//
// Tables, all doubles holding ln of the quantity (-inf for 0):
//   alpha  [n][2^(n-1)]  alpha_v(S), S with bit v squeezed out
//   f, b   [2^n]         indexed by the mask itself
//   gamma  [2^(n-1)]     one table reused variable after variable
//                        ([n][2^(n-1)] with option "posterior_keep")
// Launches of one call (m = n - 1 table bits):
//   post_fill_kernel      alpha = -inf
//   post_scatter_kernel   the lists into alpha, with the validity checks
//   post_tile_kernel      subset sums along bits 0 .. min(m, 10) - 1 of all n
//                         tables at once, a tile of 2^10 entries in LDS
//   post_strided_kernel   ... along the bits above, 4 per launch
//   post_sweep_kernel     one per layer l = 1 .. n: f and b of the layer's
//                         C(n, l) nodes (colex order) from layer l - 1
//   per variable v:  post_tile_kernel forms g_v = f(S) b(V \ S \ v) as it
//                    loads its tile and takes the superset sums along the low
//                    bits, post_strided_kernel the high bits,
//                    post_gather_kernel reads gamma_v at v's stored sets
//   post_norm_kernel      each variable's sets normalised by their own sum
//   post_edge_kernel      one workgroup per (u, v): the logsumexp of v's sets
//                         that contain u
// A transform is n (n - 1) 2^(n-2) logaddexp per direction.  The tile and the
// 4 bits per strided launch were sized on the assumption that their FP64 exp
// and log1p bound it; measured at n = 25 (Times) that holds for
// the tile launch only: the strided launches move 26.8 GB at 1.5 - 2.0 TB/s,
// nearer the memory bound.  More bits per strided launch (fewer passes over
// the tables) is the open item.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "posterior_dev.h"
#include "posterior_state.h"
#include "ulg_internal.h"

namespace ulg {

void posterior_delete(ulg_ctx *c) {
    delete c->posterior;
    c->posterior = nullptr;
}

}  // namespace ulg

using namespace ulg;

namespace {

constexpr int kB = 256;
constexpr int kTileBits = 10;  // tile kernel: 2^10 doubles = 8 KiB LDS
constexpr int kColBits = 4;    // strided kernel: 2^4 rows ...
constexpr int kRowBits = 5;    // ... of 2^5 contiguous doubles (256 B) = 4 KiB LDS

// bits of the error word
constexpr unsigned kErrSet = 1, kErrScore = 2, kErrDup = 4;

// blocks x threads along x stay below 2^32: larger launches spread over y
constexpr uint64_t kGridX = 1ull << 20;
inline dim3 flat_grid(uint64_t blocks) {
    return dim3((unsigned)std::min<uint64_t>(blocks, kGridX), (unsigned)((blocks + kGridX - 1) / kGridX));
}
__device__ __forceinline__ uint64_t flat_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

__global__ void __launch_bounds__(kB) post_fill_kernel(double *t, uint64_t count) {
    const uint64_t i = flat_block() * kB + threadIdx.x;
    if (i < count) t[i] = neg_inf();
}

// One lane per list entry, blockIdx.y = the variable.  A set with its own
// variable's bit or a bit >= n, and a score that is not finite, set the error
// word and are not written; a second writer of a slot (a duplicate set) finds
// it taken.  alpha must hold -inf throughout.
__global__ void __launch_bounds__(kB) post_scatter_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets,
                                                          int n, double *alpha, unsigned int *err) {
    const int v = blockIdx.y;
    const int64_t b = offsets[v], e = offsets[v + 1];
    const uint64_t bad = ~((n >= 64 ? 0ull : (1ull << n)) - 1ull) | (1ull << v);
    const unsigned long long empty = (unsigned long long)__double_as_longlong(neg_inf());
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(alpha + ((uint64_t)v << (n - 1)));
    for (int64_t i = b + (int64_t)blockIdx.x * kB + threadIdx.x; i < e; i += (int64_t)gridDim.x * kB) {
        const uint64_t S = sets[i];
        const float s = scores[i];
        unsigned w = 0;
        if (S & bad) w |= kErrSet;
        if (!(fabsf(s) <= 3.402823466e+38f)) w |= kErrScore;  // false for a NaN too
        if (!w) {
            const unsigned long long val = (unsigned long long)__double_as_longlong((double)s);
            if (atomicCAS(&slots[post_squeeze((uint32_t)S, v)], empty, val) != empty) w |= kErrDup;
        }
        if (w) atomicOr(err, w);
    }
}

// f(S) b(V \ S \ v) for the S of index i in v's table
__device__ __forceinline__ double form_g(const double *f, const double *b, uint32_t i, int v, int n) {
    return f[post_expand(i, v)] + b[post_expand(post_complement(i, n), v)];
}

// The transform along bits 0 .. T - 1, T = min(m, kTileBits), of `ntab` tables
// of 2^m entries that lie one after the other: a workgroup per tile of 2^T
// contiguous entries.  kSuper: entry i takes in entry i | bit (superset sums),
// else entry i | bit takes in entry i (subset sums).  kFormG: the tile is not
// read from the table but formed from f and b (g_v of variable var).
template <bool kSuper, bool kFormG>
__global__ void __launch_bounds__(kB) post_tile_kernel(double *tab, int m, uint64_t blocks, const double *f, const double *b,
                                                       int var, int n) {
    __shared__ double t[1 << kTileBits];
    const uint64_t blk = flat_block();
    if (blk >= blocks) return;
    const int T = m < kTileBits ? m : kTileBits;
    const uint32_t size = 1u << T;
    const uint64_t base = blk << T;  // tables are 2^m entries each, tiles 2^T: the tiles of all tables in a row
    const uint32_t in_table = (uint32_t)(base & ((1ull << m) - 1ull));
    for (uint32_t i = threadIdx.x; i < size; i += kB) t[i] = kFormG ? form_g(f, b, in_table + i, var, n) : tab[base + i];
    __syncthreads();
    for (int bit = 0; bit < T; ++bit) {
        const uint32_t mask = 1u << bit;
        for (uint32_t p = threadIdx.x; p < (size >> 1); p += kB) {
            const uint32_t i = ((p >> bit) << (bit + 1)) | (p & (mask - 1u));
            const double lo = t[i], hi = t[i | mask];
            if (kSuper) t[i] = post_logaddexp(lo, hi);
            else t[i | mask] = post_logaddexp(hi, lo);
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < size; i += kB) tab[base + i] = t[i];
}

// ... along bits bit_lo .. bit_lo + G - 1, G = min(kColBits, m - bit_lo): a
// workgroup per tile of 2^G rows (one per value of those bits) of 2^kRowBits
// contiguous entries.  bit_lo >= kTileBits >= kRowBits.
template <bool kSuper>
__global__ void __launch_bounds__(kB) post_strided_kernel(double *tab, int m, int bit_lo, uint64_t blocks) {
    __shared__ double t[1 << (kColBits + kRowBits)];
    const uint64_t blk = flat_block();
    if (blk >= blocks) return;
    const int G = m - bit_lo < kColBits ? m - bit_lo : kColBits;
    const int per_table_bits = m - G - kRowBits;  // workgroups per table = 2^this
    double *tv = tab + ((blk >> per_table_bits) << m);
    const uint64_t bid = blk & ((1ull << per_table_bits) - 1ull);
    const int nlow = bit_lo - kRowBits;
    const uint64_t base = ((bid & ((1ull << nlow) - 1ull)) << kRowBits) | ((bid >> nlow) << (bit_lo + G));
    const int size = 1 << (G + kRowBits);
    constexpr int kRowMask = (1 << kRowBits) - 1;
    for (int e = threadIdx.x; e < size; e += kB)
        t[e] = tv[base | ((uint64_t)(e >> kRowBits) << bit_lo) | (uint64_t)(e & kRowMask)];
    __syncthreads();
    for (int j = 0; j < G; ++j) {
        for (int p = threadIdx.x; p < (size >> 1); p += kB) {
            const int lw = p & kRowMask, q = p >> kRowBits;  // q: the rows with bit j clear
            const int r0 = ((q >> j) << (j + 1)) | (q & ((1 << j) - 1));
            const int i0 = (r0 << kRowBits) | lw, i1 = ((r0 | (1 << j)) << kRowBits) | lw;
            const double lo = t[i0], hi = t[i1];
            if (kSuper) t[i0] = post_logaddexp(lo, hi);
            else t[i1] = post_logaddexp(hi, lo);
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < size; e += kB)
        tv[base | ((uint64_t)(e >> kRowBits) << bit_lo) | (uint64_t)(e & kRowMask)] = t[e];
}

// One lane per node S of layer `layer`, colex rank = the lane's index:
//   f(S) = sum_{v in S} f(S \ v) alpha_v(S \ v)
//   b(S) = sum_{v in S} alpha_v(V \ S) b(S \ v)
// both over v ascending.  binom64[a * 64 + k] = C(a, k).
__global__ void __launch_bounds__(kB) post_sweep_kernel(const double *alpha, double *f, double *b, const uint64_t *binom64,
                                                        int n, int layer, uint64_t count) {
    const uint64_t r = flat_block() * kB + threadIdx.x;
    if (r >= count) return;
    uint32_t S = 0;
    {
        uint64_t rr = r;
        int c = n - 1;
        for (int k = layer; k >= 1; --k) {
            while (binom64[c * 64 + k] > rr) --c;
            S |= 1u << c;
            rr -= binom64[c * 64 + k];
            --c;
        }
    }
    const uint32_t rest = ((n >= 32 ? 0u : (1u << n)) - 1u) & ~S;
    const int m = n - 1;
    double fa = neg_inf(), ba = neg_inf();
    for (uint32_t x = S; x; x &= x - 1u) {
        const int v = __builtin_ctz(x);
        const uint32_t P = S ^ (1u << v);
        const double *av = alpha + ((uint64_t)v << m);
        fa = post_logaddexp(fa, f[P] + av[post_squeeze(P, v)]);
        ba = post_logaddexp(ba, av[post_squeeze(rest, v)] + b[P]);
    }
    f[S] = fa;
    b[S] = ba;
}

// t_i = s_i + ln gamma_v(P_i) for the entries of variable v
__global__ void __launch_bounds__(kB) post_gather_kernel(const uint64_t *sets, const float *scores, int64_t begin, int64_t end,
                                                         int v, const double *gamma, double *logpost) {
    const int64_t i = begin + (int64_t)flat_block() * kB + threadIdx.x;
    if (i < end) logpost[i] = (double)scores[i] + gamma[post_squeeze((uint32_t)sets[i], v)];
}

// ln sum_i exp(x_i) over the entries begin <= i < end with take(i), by one
// workgroup of kB lanes: the maximum first, which no order changes; then lane
// l adds exp(x_i - max) over its entries i = begin + l, begin + l + kB, ...
// ascending, and the lanes' sums meet in a fixed binary tree.  The result is
// the same in every lane; -inf when nothing is taken or every x is -inf.
template <typename Take>
__device__ double block_logsumexp(const double *x, int64_t begin, int64_t end, Take take) {
    __shared__ double red[kB];
    double mx = neg_inf();
    for (int64_t i = begin + threadIdx.x; i < end; i += kB)
        if (take(i)) mx = fmax(mx, x[i]);
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = kB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    mx = red[0];
    __syncthreads();
    if (!(mx > neg_inf())) return mx;
    double sum = 0.0;
    for (int64_t i = begin + threadIdx.x; i < end; i += kB)
        if (take(i)) sum += exp(x[i] - mx);  // exp(-inf) = 0
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int s = kB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    sum = red[0];
    __syncthreads();
    return mx + log(sum);
}

// blockIdx.x = v: ln p(Pa_v = P_i) = t_i - L_v, L_v = ln sum_i exp(t_i) over
// v's own entries; -inf throughout when Z = 0
__global__ void __launch_bounds__(kB) post_norm_kernel(const int64_t *offsets, double *logpost, const double *f, int n) {
    const int v = blockIdx.x;
    const int64_t b = offsets[v], e = offsets[v + 1];
    const double L = block_logsumexp(logpost, b, e, [](int64_t) { return true; });
    const bool zero = !(f[(n >= 32 ? 0u : (1u << n)) - 1u] > neg_inf()) || !(L > neg_inf());
    for (int64_t i = b + threadIdx.x; i < e; i += kB) {
        const double t = logpost[i];
        logpost[i] = zero || !(t > neg_inf()) ? neg_inf() : t - L;
    }
}

// blockIdx = (u, v): edge[u * n + v] = sum of p(Pa_v = P) over v's stored P that contain u
__global__ void __launch_bounds__(kB) post_edge_kernel(const uint64_t *sets, const int64_t *offsets, const double *logpost,
                                                       int n, double *edge) {
    const int u = blockIdx.x, v = blockIdx.y;
    double l = neg_inf();
    if (u != v) l = block_logsumexp(logpost, offsets[v], offsets[v + 1], [=](int64_t i) { return ((sets[i] >> u) & 1ull) != 0; });
    if (threadIdx.x == 0) edge[(int64_t)u * n + v] = l > neg_inf() ? exp(l) : 0.0;
}

PosteriorState &state(ulg_ctx *c) {
    if (!c->posterior) c->posterior = new PosteriorState();
    return *c->posterior;
}

// bytes of the tables: alpha, f, b and `gtabs` gamma tables (the figure of "posterior_bytes")
double table_bytes(int n, int gtabs) { return 8.0 * (std::ldexp((double)n + gtabs, n - 1) + std::ldexp(2.0, n)); }

// The subset (kSuper false) or superset sums of `ntab` tables of 2^m entries along every bit
template <bool kSuper>
int transform_high_bits(ulg_ctx *c, double *tab, int ntab, int m, const char *name) {
    for (int bit_lo = kTileBits; bit_lo < m; bit_lo += kColBits) {
        const int G = std::min(kColBits, m - bit_lo);
        const uint64_t blocks = (uint64_t)ntab << (m - G - kRowBits);
        prof_begin(c, name);
        post_strided_kernel<kSuper><<<flat_grid(blocks), kB, 0, c->stream>>>(tab, m, bit_lo, blocks);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    return ULG_OK;
}

// The lists are on the device in s (variable order), s.offsets is the host
// copy of their offsets: everything from the scatter to the outputs.
int run(ulg_ctx *c, PosteriorState &s, double *log_z, double *edge, double *set_logpost) {
    const std::vector<int64_t> &offs = s.offsets;
    const int n = s.n, m = n - 1;
    const bool keep = c->opt.posterior_keep != 0;
    const uint64_t half = 1ull << m, full = 1ull << n;
    s.ready = false;
    s.kept = false;
    int rc;
    if ((rc = ensure(c, s.alpha, (size_t)(n * half))) || (rc = ensure(c, s.f, (size_t)full)) || (rc = ensure(c, s.b, (size_t)full)) ||
        (rc = ensure(c, s.gamma, (size_t)((keep ? n : 1) * half))) || (rc = ensure(c, s.d_logpost, (size_t)s.total)) ||
        (rc = ensure(c, s.d_edge, (size_t)n * n)) || (rc = ensure(c, s.d_err, 1)))
        return rc;
    // 1. scatter, with the checks
    ULG_HIP(c, hipMemsetAsync(s.d_err.p, 0, sizeof(unsigned int), c->stream));
    prof_begin(c, "post_fill");
    post_fill_kernel<<<flat_grid((n * half + kB - 1) / kB), kB, 0, c->stream>>>(s.alpha.p, n * half);
    prof_end(c);
    int64_t longest = 1;
    for (int v = 0; v < n; ++v) longest = std::max(longest, offs[v + 1] - offs[v]);
    prof_begin(c, "post_scatter");
    post_scatter_kernel<<<dim3((unsigned)std::min<int64_t>((longest + kB - 1) / kB, 4096), (unsigned)n), kB, 0, c->stream>>>(
        s.d_sets.p, s.d_scores.p, s.d_offsets.p, n, s.alpha.p, s.d_err.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    unsigned int err = 0;
    ULG_HIP(c, hipMemcpyAsync(&err, s.d_err.p, sizeof(err), hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    if (err) {
        std::string msg = "ulg_posterior:";
        if (err & kErrSet) msg += " a set holds its own variable or a bit >= n;";
        if (err & kErrScore) msg += " a score is NaN or infinite;";
        if (err & kErrDup) msg += " a variable lists a set twice;";
        msg.pop_back();
        return set_err(c, ULG_ERR_ARG, msg);
    }
    // 2. alpha: subset sums of all n tables
    {
        const uint64_t blocks = (uint64_t)n << (m - std::min(m, kTileBits));
        prof_begin(c, "post_alpha_tile");
        post_tile_kernel<false, false><<<flat_grid(blocks), kB, 0, c->stream>>>(s.alpha.p, m, blocks, nullptr, nullptr, 0, n);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
        if ((rc = transform_high_bits<false>(c, s.alpha.p, n, m, "post_alpha_strided"))) return rc;
    }
    // 3. the sweeps: f(0) = b(0) = 1
    ULG_HIP(c, hipMemsetAsync(s.f.p, 0, sizeof(double), c->stream));
    ULG_HIP(c, hipMemsetAsync(s.b.p, 0, sizeof(double), c->stream));
    for (int layer = 1; layer <= n; ++layer) {
        const uint64_t count = host_binom64()[(size_t)n * 64 + layer];
        prof_begin(c, "post_sweep");
        post_sweep_kernel<<<flat_grid((count + kB - 1) / kB), kB, 0, c->stream>>>(s.alpha.p, s.f.p, s.b.p, c->d_binom64.p, n, layer,
                                                                                 count);
        prof_end(c);
        ULG_HIP(c, hipGetLastError());
    }
    // 4. per variable: g_v, its superset sums, gamma_v at the stored sets
    {
        const uint64_t blocks = 1ull << (m - std::min(m, kTileBits));
        for (int v = 0; v < n; ++v) {
            double *g = s.gamma.p + (keep ? (uint64_t)v * half : 0);
            prof_begin(c, "post_gamma_tile");
            post_tile_kernel<true, true><<<flat_grid(blocks), kB, 0, c->stream>>>(g, m, blocks, s.f.p, s.b.p, v, n);
            prof_end(c);
            ULG_HIP(c, hipGetLastError());
            if ((rc = transform_high_bits<true>(c, g, 1, m, "post_gamma_strided"))) return rc;
            const int64_t cnt = offs[v + 1] - offs[v];
            if (cnt > 0) {
                prof_begin(c, "post_gather");
                post_gather_kernel<<<flat_grid((uint64_t)(cnt + kB - 1) / kB), kB, 0, c->stream>>>(s.d_sets.p, s.d_scores.p, offs[v],
                                                                                                  offs[v + 1], v, g, s.d_logpost.p);
                prof_end(c);
                ULG_HIP(c, hipGetLastError());
            }
        }
    }
    // 5. the posteriors of the sets and of the edges
    prof_begin(c, "post_norm");
    post_norm_kernel<<<n, kB, 0, c->stream>>>(s.d_offsets.p, s.d_logpost.p, s.f.p, n);
    prof_end(c);
    prof_begin(c, "post_edge");
    post_edge_kernel<<<dim3((unsigned)n, (unsigned)n), kB, 0, c->stream>>>(s.d_sets.p, s.d_offsets.p, s.d_logpost.p, n, s.d_edge.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    if (log_z) ULG_HIP(c, hipMemcpyAsync(log_z, s.f.p + (full - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (edge) ULG_HIP(c, hipMemcpyAsync(edge, s.d_edge.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, c->stream));
    if (set_logpost && s.total)
        ULG_HIP(c, hipMemcpyAsync(set_logpost, s.d_logpost.p, (size_t)s.total * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    s.ready = true;
    s.kept = keep;
    c->posterior_bytes = (int64_t)table_bytes(n, keep ? n : 1);
    return ULG_OK;
}

// n > 28, or tables and lists beyond the free device memory (what the state
// already holds counts as free: its buffers are reused or replaced).  Nothing
// has been allocated yet.
int refuse_size(ulg_ctx *c, const char *who, int n, int64_t total) {
    const bool keep = c->opt.posterior_keep != 0;
    char buf[256];
    if (n > kPostMaxVars) {
        if (n < 1000)
            std::snprintf(buf, sizeof buf, "%s: n = %d needs %.0f bytes of tables; at most %d variables", who, n,
                          table_bytes(n, keep ? n : 1), kPostMaxVars);
        else
            std::snprintf(buf, sizeof buf, "%s: n = %d; at most %d variables", who, n, kPostMaxVars);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    if (c->posterior) c->posterior->drop_samples();  // the sampler's buffers of an earlier call give way to the tables
    order_mcmc_delete(c);                            // ... as does the order MCMC's state (order_mcmc.hip)
    size_t free_b = 0, total_b = 0;
    ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const double need = table_bytes(n, keep ? n : 1) + 28.0 * (double)total + 8.0 * n * n + 8.0 * (n + 1) + 256.0;
    const double have = (double)free_b + (c->posterior ? (double)c->posterior->held_bytes() : 0.0);
    if (need > have) {
        std::snprintf(buf, sizeof buf, "%s: n = %d with %lld sets needs %.0f bytes of device memory, %.0f are free", who, n,
                      (long long)total, need, have);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    return ULG_OK;
}

}  // namespace

extern "C" {

int ulg_posterior(ulg_ctx *c, int n, const int64_t *offsets, const uint64_t *sets, const float *scores, int device_ptrs,
                  double *log_z, double *edge, double *set_logpost) {
    if (!c) return ULG_ERR_ARG;
    if (n < 1) return set_err(c, ULG_ERR_ARG, "ulg_posterior: n < 1");
    if (!offsets || !log_z || !edge) return set_err(c, ULG_ERR_ARG, "ulg_posterior: bad arguments");
    ULG_HIP(c, hipSetDevice(c->device));
    if (n > kPostMaxVars) return refuse_size(c, "ulg_posterior", n, 0);
    for (int v = 0; v < n; ++v)
        if (offsets[v + 1] < offsets[v]) return set_err(c, ULG_ERR_ARG, "ulg_posterior: offsets not ascending");
    const int64_t total = offsets[n] - offsets[0];
    if (total && (!sets || !scores)) return set_err(c, ULG_ERR_ARG, "ulg_posterior: bad arguments");
    if (int rc = refuse_size(c, "ulg_posterior", n, total)) return rc;
    PosteriorState &s = state(c);
    s.ready = false;
    int rc;
    if ((rc = ensure(c, s.d_sets, (size_t)total)) || (rc = ensure(c, s.d_scores, (size_t)total)) ||
        (rc = ensure(c, s.d_offsets, (size_t)n + 1)))
        return rc;
    s.n = n;
    s.total = total;
    std::vector<int64_t> &offs = s.offsets;
    offs.assign((size_t)n + 1, 0);
    for (int v = 0; v <= n; ++v) offs[v] = offsets[v] - offsets[0];
    const hipMemcpyKind kind = device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (total) {
        ULG_HIP(c, hipMemcpyAsync(s.d_sets.p, sets + offsets[0], (size_t)total * 8, kind, c->stream));
        ULG_HIP(c, hipMemcpyAsync(s.d_scores.p, scores + offsets[0], (size_t)total * 4, kind, c->stream));
    }
    ULG_HIP(c, hipMemcpyAsync(s.d_offsets.p, offs.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    return run(c, s, log_z, edge, set_logpost);
}

int ulg_posterior_from_scores(ulg_ctx *c, double *log_z, double *edge, double *set_logpost) {
    if (!c) return ULG_ERR_ARG;
    if (!log_z || !edge) return set_err(c, ULG_ERR_ARG, "ulg_posterior_from_scores: bad arguments");
    if (int rc0 = finish_pending(c)) return rc0;
    if (!c->scored) return set_err(c, ULG_ERR_STATE, "ulg_posterior_from_scores: no scoring call yet");
    const int n = c->n;
    std::vector<int> where((size_t)std::max(n, 1), -1);
    bool all = c->nv == n && n >= 1;
    for (int i = 0; all && i < n; ++i) {
        const int v = c->vars[i];
        all = v >= 0 && v < n && where[v] < 0;
        if (all) where[v] = i;
    }
    if (!all) return set_err(c, ULG_ERR_STATE, "ulg_posterior_from_scores: every variable must be scored in this context");
    ULG_HIP(c, hipSetDevice(c->device));
    if (n > kPostMaxVars) return refuse_size(c, "ulg_posterior_from_scores", n, 0);
    std::vector<int64_t> src((size_t)n + 1);
    ULG_HIP(c, hipMemcpyAsync(src.data(), c->out_offsets.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t total = src[n];
    if (int rc = refuse_size(c, "ulg_posterior_from_scores", n, total)) return rc;
    PosteriorState &s = state(c);
    s.ready = false;
    int rc;
    if ((rc = ensure(c, s.d_sets, (size_t)total)) || (rc = ensure(c, s.d_scores, (size_t)total)) ||
        (rc = ensure(c, s.d_offsets, (size_t)n + 1)))
        return rc;
    s.n = n;
    s.total = total;
    // the lists by variable index, each variable's sets in their stored order
    std::vector<int64_t> &offs = s.offsets;
    offs.assign((size_t)n + 1, 0);
    for (int v = 0; v < n; ++v) {
        const int i = where[v];
        const int64_t cnt = src[i + 1] - src[i];
        offs[v + 1] = offs[v] + cnt;
        if (cnt) {
            ULG_HIP(c, hipMemcpyAsync(s.d_sets.p + offs[v], c->out_sets.p + src[i], (size_t)cnt * 8, hipMemcpyDeviceToDevice, c->stream));
            ULG_HIP(c, hipMemcpyAsync(s.d_scores.p + offs[v], c->out_scores.p + src[i], (size_t)cnt * 4, hipMemcpyDeviceToDevice,
                                      c->stream));
        }
    }
    ULG_HIP(c, hipMemcpyAsync(s.d_offsets.p, offs.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    return run(c, s, log_z, edge, set_logpost);
}

int ulg_posterior_table(ulg_ctx *c, int which, int var, double *out, int64_t cap, int64_t *count) {
    if (!c || !count || cap < 0 || (cap && !out)) return ULG_ERR_ARG;
    if (!c->posterior || !c->posterior->ready) return set_err(c, ULG_ERR_STATE, "ulg_posterior_table: no posterior call");
    const PosteriorState &s = *c->posterior;
    if (which < 0 || which > 3) return set_err(c, ULG_ERR_ARG, "ulg_posterior_table: which must be 0..3");
    const bool per_var = which == 0 || which == 3;
    if (per_var && (var < 0 || var >= s.n)) return set_err(c, ULG_ERR_ARG, "ulg_posterior_table: bad variable");
    if (which == 3 && !s.kept)
        return set_err(c, ULG_ERR_STATE, "ulg_posterior_table: the gamma tables were not kept (option posterior_keep)");
    const int64_t total = per_var ? (int64_t)1 << (s.n - 1) : (int64_t)1 << s.n;
    *count = total;
    if (cap == 0) return ULG_OK;
    if (cap < total) return set_err(c, ULG_ERR_ARG, "ulg_posterior_table: cap below the table's entries");
    const double *src = which == 0 ? s.alpha.p + (uint64_t)var * (uint64_t)total
                        : which == 1 ? s.f.p
                        : which == 2 ? s.b.p
                                     : s.gamma.p + (uint64_t)var * (uint64_t)total;
    ULG_HIP(c, hipSetDevice(c->device));
    ULG_HIP(c, hipMemcpyAsync(out, src, (size_t)total * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    return ULG_OK;
}

}  // extern "C"
