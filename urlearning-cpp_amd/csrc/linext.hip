// linext.hip -- the number of linear extensions of each DAG of a batch
// (ulg_dag_linear_extensions; contract: include/ulg.h), the weight 1 / ext(G)
// that turns samples of the order-modular posterior into estimates under the
// prior uniform over DAGs.  The lattice recursion
//   c(0) = 1,  c(S) = sum_{v in S, Pa_v subset of S \ v} c(S \ v),  ext = c(V)
// over all 2^n subsets, in 128-bit integers (linext_dev.h): exact, and 0 for a
// graph with a directed cycle.
//
//   linext_init_kernel   c(0) = 1 of every DAG of the batch, and the batch's
//                        one zero cell
//   linext_layer_kernel  one launch per layer l = 1 .. n, post_sweep_kernel's
//                        form: a lane per (DAG, node of the layer), the node
//                        unranked from its colex rank.
// A DAG's table is laid out layer by layer, a layer in colex order
// (linext_dev.h lx_index): lane r of a layer's launch writes entry off(l) + r,
// so a wave stores 1 KB of consecutive bytes, and the entries c(S \ v) that
// the lanes of a wave gather for one v lie close together in layer l - 1
// (their ranks follow from the lanes' own by lx_walk_step, two binomials per
// member out of a 3.5 KB table in LDS).  A table indexed by the subset's number
// spreads a layer over the whole 2^n entries, about one useful entry per 64-byte
// line read or written; it measured 2.1 to 2.4 times slower.
// A workgroup belongs to one DAG (blockIdx.y, z), so the DAG's parent masks
// are wave-uniform: the loop runs over v = n-1 .. 0 for the whole wave and
// reads mask v by a scalar load.  A v that contributes no term reads the zero
// cell instead of c(S \ v): every lane issues the same n 16-byte loads with no
// branch between them, so they are all in flight together, and the ones that
// count nothing hit one cache line.  Plain vector loads and stores, no
// atomics; a lane writes its own node only.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "linext_dev.h"
#include "ulg_internal.h"

using namespace ulg;

namespace {

constexpr int kB = 256;
constexpr uint64_t kGridY = 32768;             // DAGs along y, the rest along z
constexpr uint64_t kMaxBatch = kGridY * 32768;  // z stays below 65536
constexpr double kBatchBytes = 1073741824.0;    // 2^30: the tables of a default batch

__global__ void __launch_bounds__(kB) linext_init_kernel(LxCount *table, int n, uint64_t dags) {
    const uint64_t k = (uint64_t)blockIdx.x * kB + threadIdx.x;
    if (k < dags) table[lx_index(k, n, 0u, 0u)] = LxCount{1, 0};         // layer 0 is entry 0
    if (k == dags) table[lx_index(dags, n, 0u, 0u)] = LxCount{0, 0};  // the zero cell, after the last table
}

// par[dag * n + v]: the parent mask of v.  count = C(n, layer) nodes; off_prev
// and off_cur: the first entries of layers layer - 1 and layer.  out != nullptr
// (the last layer): the node's count also goes to out[dag].
__global__ void __launch_bounds__(kB) linext_layer_kernel(LxCount *table, const uint32_t *__restrict__ par,
                                                          const uint64_t *__restrict__ binom64, int n, int layer, uint32_t count,
                                                          uint32_t off_prev, uint32_t off_cur, uint64_t dags, LxCount *out) {
    __shared__ uint32_t bn[kLxBinomSize];
    for (int i = threadIdx.x; i < kLxBinomSize; i += kB)
        bn[i] = (uint32_t)binom64[(i / kLxBinomStride) * 64 + i % kLxBinomStride];
    __syncthreads();
    const uint64_t dag = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;  // wave-uniform
    if (dag >= dags) return;
    const uint32_t r = blockIdx.x * kB + threadIdx.x;
    if (r >= count) return;
    const uint32_t S = lx_unrank(bn, n, layer, r);
    const uint32_t *pv = par + dag * (uint64_t)n;
    const LxCount *prev = table + lx_index(dag, n, off_prev, 0u);
    const LxCount *zero = table + lx_index(dags, n, 0u, 0u);
    LxCount acc{0, 0};
    LxWalk w;
#pragma unroll 4
    for (int v = n - 1; v >= 0; --v) {
        const uint32_t rank = lx_walk_step(w, bn, S, r, v);
        const LxCount *src = lx_term(S, v, pv[v]) ? prev + rank : zero;
        acc = lx_add(acc, *src);
    }
    table[lx_index(dag, n, off_cur, r)] = acc;
    if (out) out[dag] = acc;
}

double table_bytes(int n) { return 16.0 * (double)(1ull << n); }

}  // namespace

extern "C" {

int ulg_dag_linear_extensions(ulg_ctx *c, int n, int64_t count, const uint64_t *parents, uint64_t *ext_lo, uint64_t *ext_hi,
                              double *log_ext) {
    if (!c) return ULG_ERR_ARG;
    const char *who = "ulg_dag_linear_extensions";
    if (n < 1) return set_err(c, ULG_ERR_ARG, std::string(who) + ": n < 1");
    if (count < 0) return set_err(c, ULG_ERR_ARG, std::string(who) + ": negative count");
    if (count > 0 && (!parents || !ext_lo)) return set_err(c, ULG_ERR_ARG, std::string(who) + ": bad arguments");
    char buf[256];
    if (n > kLinextMaxVars) {
        std::snprintf(buf, sizeof buf, "%s: n = %d; at most %d variables", who, n, kLinextMaxVars);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    // every mask, before any device work: 32 bits hold one (n <= 28)
    std::vector<uint32_t> par;
    try {
        par.resize((size_t)count * (size_t)n);
    } catch (const std::exception &) {
        return set_err(c, ULG_ERR_UNSUPPORTED, std::string(who) + ": the masks do not fit the host memory");
    }
    const uint64_t outside = ~((1ull << n) - 1ull);
    for (int64_t k = 0; k < count; ++k)
        for (int v = 0; v < n; ++v) {
            const uint64_t m = parents[(size_t)k * n + v];
            if ((m & outside) || ((m >> v) & 1ull)) {
                std::snprintf(buf, sizeof buf, "%s: DAG %lld, variable %d: a parent mask with %s", who, (long long)k, v,
                              (m & outside) ? "a bit >= n" : "the variable's own bit");
                return set_err(c, ULG_ERR_ARG, buf);
            }
            par[(size_t)k * n + v] = (uint32_t)m;
        }
    c->linext_batches = 0;
    if (count == 0) return ULG_OK;  // no device work
    ULG_HIP(c, hipSetDevice(c->device));
    // the batch, before anything is allocated: per DAG its table, its masks and
    // its result; per batch the zero cell
    const double per_dag = table_bytes(n) + 4.0 * n + 16.0;
    size_t free_b = 0, total_b = 0;
    ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const double slack = 64.0 + 3 * 16.0;  // the zero cell and the three buffers' slack (dev_buf.h)
    if (per_dag + slack > (double)free_b) {
        std::snprintf(buf, sizeof buf, "%s: one DAG of n = %d needs %.0f bytes of device memory, %.0f are free", who, n,
                      per_dag + slack, (double)free_b);
        return set_err(c, ULG_ERR_UNSUPPORTED, buf);
    }
    // kBatchBytes of tables per batch, within seven eighths of the free memory; one DAG at least (it
    // fits: checked above).  More per batch buys nothing once every launch fills the card, and a
    // large allocation costs more than the count itself.
    uint64_t batch = (uint64_t)std::max(1.0, std::floor((std::min((double)free_b * 0.875, kBatchBytes) - slack) / per_dag));
    batch = std::min<uint64_t>({batch, (uint64_t)count, kMaxBatch});
    if (c->opt.linext_batch > 0) batch = std::min<uint64_t>(batch, (uint64_t)c->opt.linext_batch);

    // the call's own buffers: freed when it returns, on every path
    DevBuf<LxCount> table, d_out;
    DevBuf<uint32_t> d_par;
    int rc;
    if ((rc = ensure(c, table, (size_t)((batch << n) + 1))) || (rc = ensure(c, d_par, (size_t)batch * n)) ||
        (rc = ensure(c, d_out, (size_t)batch)))
        return rc;
    std::vector<LxCount> h_out((size_t)batch);
    uint32_t off[kLinextMaxVars + 2];
    lx_layer_offsets(n, off);
    for (int64_t first = 0; first < count; first += (int64_t)batch) {
        const uint64_t dags = std::min<uint64_t>(batch, (uint64_t)(count - first));
        ULG_HIP(c, hipMemcpyAsync(d_par.p, par.data() + (size_t)first * n, (size_t)dags * n * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, c->stream));
        prof_begin(c, "linext_init");
        linext_init_kernel<<<dim3((unsigned)((dags + 1 + kB - 1) / kB)), kB, 0, c->stream>>>(table.p, n, dags);
        prof_end(c);
        const unsigned gy = (unsigned)std::min<uint64_t>(dags, kGridY), gz = (unsigned)((dags + gy - 1) / gy);
        for (int layer = 1; layer <= n; ++layer) {
            const uint32_t nodes = off[layer + 1] - off[layer];
            prof_begin(c, "linext_layer");
            linext_layer_kernel<<<dim3((nodes + kB - 1) / kB, gy, gz), kB, 0, c->stream>>>(
                table.p, d_par.p, c->d_binom64.p, n, layer, nodes, off[layer - 1], off[layer], dags, layer == n ? d_out.p : nullptr);
            prof_end(c);
        }
        ULG_HIP(c, hipGetLastError());
        ULG_HIP(c, hipMemcpyAsync(h_out.data(), d_out.p, (size_t)dags * sizeof(LxCount), hipMemcpyDeviceToHost, c->stream));
        ULG_HIP(c, hipStreamSynchronize(c->stream));
        prof_collect(c);
        for (uint64_t k = 0; k < dags; ++k) {
            const LxCount x = h_out[(size_t)k];
            ext_lo[first + (int64_t)k] = x.lo;
            if (ext_hi) ext_hi[first + (int64_t)k] = x.hi;
            if (log_ext)
                log_ext[first + (int64_t)k] =
                    (x.lo | x.hi) ? (double)logl((long double)x.hi * 18446744073709551616.0L + (long double)x.lo) : -INFINITY;
        }
        ++c->linext_batches;
    }
    return ULG_OK;
}

}  // extern "C"
