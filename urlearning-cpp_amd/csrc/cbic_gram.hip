// cbic_gram.hip -- the cBIC scorer's data: normalisation, the FP64 Gram matrix
// G = Z'Z on v_mfma_f64_16x16x4_f64 (the only dense contraction on the path)
// and the BIC penalty, once per ulg_cbic_load.  See cbic.hip for the design.
//
// Reference path (ninalu/urlearning-cpp, urlearning/):
//   BIC_OLS_Function ctor          scoring_function/BIC_OLS.cpp:30-123

#include "search_internal.h"

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

// *out = lambda ln(N) with the device's logarithm and one rounded product:
// the value every lane used to compute inside the score's last expression.
__global__ void penalty_kernel(double N, double lambda, double *out) { *out = lambda * log(N); }

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

}  // extern "C"
