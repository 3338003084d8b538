// posterior_sample.hip -- independent (linear order, DAG) draws from the exact
// order-modular posterior (ulg_posterior_sample, ulg_posterior_sample_u;
// contract: include/ulg.h).  Backward sampling through the forward table of
// the last ulg_posterior* call: a sample walks from S = V down to the empty
// set, and the step at |S| = l chooses the sink v of S with probability
// f(S \ v) alpha_v(S \ v) / f(S), then a stored parent set P of v within S \ v
// with probability w_v(P) / alpha_v(S \ v).  No MCMC, no burn-in.
//
// One launch, post_sample_kernel: a wave64 per sample, 4 waves per workgroup.
//   sink step  lane v < n stands for variable v (so the candidates are in
//              ascending order along the wave); a member of S gathers f(S \ v)
//              and alpha_v(S \ v), the others weigh 0; an integer inclusive
//              scan, the threshold, __ballot on C > t.
//   set step   the wave strides v's list 64 entries at a time.  A list of at
//              most 64 entries takes one pass (its total is the scan's last
//              lane); a longer one takes two: the total first (integer sums,
//              order-free), then chunk by chunk with a running base up to the
//              first chunk whose end exceeds t.
// Every choice is made on the integers of posterior_sample_dev.h, so a sample
// depends on the tables, the lists, the seed and its own index alone -- not on
// the launch geometry, the call's `first` or how calls split a range.  Plain
// vector stores only: a lane writes its own variable's parent set; no atomics,
// no floating-point reduction (the log weight is added by v ascending).
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "posterior_sample_dev.h"
#include "posterior_state.h"

using namespace ulg;

namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;  // per workgroup
constexpr int kB = kWave * kWaves;

// blocks x threads along x stay below 2^32: larger launches spread over y
constexpr uint64_t kGridX = 1ull << 20;
inline dim3 flat_grid(uint64_t blocks) {
    return dim3((unsigned)std::min<uint64_t>(blocks, kGridX), (unsigned)((blocks + kGridX - 1) / kGridX));
}
__device__ __forceinline__ uint64_t flat_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// inclusive sum over the lanes 0 .. lane of the wave
__device__ __forceinline__ uint64_t wave_scan(uint64_t x, int lane) {
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, d, kWave);
        if (lane >= d) x += y;
    }
    return x;
}

// The first lane whose running sum exceeds t, -1 when none does (wave-uniform)
__device__ __forceinline__ int first_above(uint64_t C, uint64_t t) {
    const unsigned long long hit = __ballot(C > t);
    return hit ? __ffsll(hit) - 1 : -1;
}

// u == nullptr: the draws are Philox's (seed, sample first + k, position i);
// else u[(k * n + i) * 2 + {0: sink, 1: set}].  err: set to 1 by a wave that
// finds a step without a candidate (every weight 0), which tables of a
// successful call with finite ln Z cannot give; that wave writes nothing else.
__global__ void __launch_bounds__(kB) post_sample_kernel(const uint64_t *sets, const float *scores, const int64_t *offsets,
                                                         const double *alpha, const double *f, int n, uint64_t seed,
                                                         int64_t first, int64_t count, const uint64_t *u, uint64_t *parents,
                                                         uint8_t *order, double *weight, unsigned int *err) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave = flat_block() * kWaves + (threadIdx.x >> 6);
    if (wave >= (uint64_t)count) return;  // the whole wave
    const int64_t k = (int64_t)wave;
    const int m = n - 1;
    uint32_t S = (uint32_t)((1ull << n) - 1ull);
    double fS = f[S];
    // lane v: the parent set and score chosen for variable v; lane i: the variable at position i
    uint64_t my_par = 0;
    double my_score = 0.0;
    int my_var = 0;
    for (int l = n; l >= 1; --l) {
        const uint32_t i = (uint32_t)(l - 1);
        PostDraw d;
        if (u) {
            const uint64_t *uk = u + ((uint64_t)k * n + i) * 2;
            d.sink = uk[0];
            d.set = uk[1];
        } else {
            d = post_draw(seed, (uint64_t)(first + k), i);
        }
        // ---- the sink of S
        double xf = 0.0, xa = 0.0;
        uint64_t q = 0;
        if (lane < n && ((S >> lane) & 1u)) {
            const uint32_t P = S ^ (1u << lane);
            xf = f[P];
            xa = alpha[((uint64_t)lane << m) + post_squeeze(P, lane)];
            q = post_weight_q((xf + xa) - fS);
        }
        uint64_t C = wave_scan(q, lane);
        uint64_t t = post_pick_threshold(d.sink, __shfl((unsigned long long)C, kWave - 1, kWave));
        const int v = first_above(C, t);
        if (v < 0) {
            if (lane == 0) *err = 1u;
            return;
        }
        fS = __shfl(xf, v, kWave);
        const double ln_a = __shfl(xa, v, kWave);
        S ^= 1u << v;  // q > 0: v was a member
        if (lane == (int)i) my_var = v;
        // ---- a stored parent set of v within S
        const int64_t b = offsets[v], e = offsets[v + 1];
        const uint64_t outside = ~(uint64_t)S;
        auto weigh = [&](int64_t idx) -> uint64_t {
            if (idx >= e) return 0;
            if (sets[idx] & outside) return 0;
            return post_weight_q((double)scores[idx] - ln_a);
        };
        int64_t chosen = -1;
        if (e - b <= kWave) {
            C = wave_scan(weigh(b + lane), lane);
            t = post_pick_threshold(d.set, __shfl((unsigned long long)C, kWave - 1, kWave));
            const int j = first_above(C, t);
            if (j >= 0) chosen = b + j;
        } else {
            uint64_t T = 0;
            for (int64_t idx = b + lane; idx < e; idx += kWave) T += weigh(idx);
            for (int s = kWave / 2; s > 0; s >>= 1) T += __shfl_xor((unsigned long long)T, s, kWave);
            t = post_pick_threshold(d.set, T);
            uint64_t base = 0;
            for (int64_t c0 = b; c0 < e; c0 += kWave) {
                C = base + wave_scan(weigh(c0 + lane), lane);
                const int j = first_above(C, t);
                if (j >= 0) {
                    chosen = c0 + j;
                    break;
                }
                base = __shfl((unsigned long long)C, kWave - 1, kWave);
            }
        }
        if (chosen < 0) {
            if (lane == 0) *err = 1u;
            return;
        }
        if (lane == v) {
            my_par = sets[chosen];
            my_score = (double)scores[chosen];
        }
    }
    double w = 0.0;
    for (int v = 0; v < n; ++v) w += __shfl(my_score, v, kWave);
    if (lane < n) {
        parents[(uint64_t)k * n + lane] = my_par;
        if (order) order[(uint64_t)k * n + lane] = (uint8_t)my_var;
    }
    if (weight && lane == 0) weight[k] = w;
}

int sample(ulg_ctx *c, const char *who, uint64_t seed, int64_t first, int64_t count, const uint64_t *u, bool with_u,
           uint64_t *parents, uint8_t *order, double *log_weight) {
    if (!c) return ULG_ERR_ARG;
    const std::string name(who);
    if (first < 0 || count < 0 || first > INT64_MAX - count) return set_err(c, ULG_ERR_ARG, name + ": first or count out of range");
    if (count > 0 && (!parents || (with_u && !u))) return set_err(c, ULG_ERR_ARG, name + ": bad arguments");
    if (!c->posterior || !c->posterior->ready) return set_err(c, ULG_ERR_STATE, name + ": no posterior call");
    if (count == 0) return ULG_OK;  // nothing to draw: no device work, ln Z is not looked at
    PosteriorState &s = *c->posterior;
    const int n = s.n;
    ULG_HIP(c, hipSetDevice(c->device));
    double log_z = 0.0;
    ULG_HIP(c, hipMemcpyAsync(&log_z, s.f.p + ((1ull << n) - 1ull), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    if (!(log_z > -INFINITY)) return set_err(c, ULG_ERR_STATE, name + ": ln Z = -inf, there is nothing to sample");
    // the device buffers of the call, before anything is allocated (what the
    // sampler already holds counts as free: its buffers are reused or replaced)
    {
        const double per = 8.0 * n + (order ? (double)n : 0.0) + (log_weight ? 8.0 : 0.0) + (with_u ? 16.0 * n : 0.0);
        const double need = per * (double)count + 5 * 16.0 + 256.0;
        size_t free_b = 0, total_b = 0;
        ULG_HIP(c, hipMemGetInfo(&free_b, &total_b));
        const double have = (double)free_b + (double)s.sample_bytes();
        if (need > have) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: %lld samples of n = %d need %.0f bytes of device memory, %.0f are free", who,
                          (long long)count, n, need, have);
            return set_err(c, ULG_ERR_UNSUPPORTED, buf);
        }
    }
    const size_t cells = (size_t)count * (size_t)n;
    int rc;
    if ((rc = ensure(c, s.s_parents, cells)) || (order && (rc = ensure(c, s.s_order, cells))) ||
        (log_weight && (rc = ensure(c, s.s_weight, (size_t)count))) || (with_u && (rc = ensure(c, s.s_u, cells * 2))) ||
        (rc = ensure(c, s.s_err, 1)))
        return rc;
    ULG_HIP(c, hipMemsetAsync(s.s_err.p, 0, sizeof(unsigned int), c->stream));
    if (with_u) ULG_HIP(c, hipMemcpyAsync(s.s_u.p, u, cells * 16, hipMemcpyHostToDevice, c->stream));
    const uint64_t blocks = ((uint64_t)count + kWaves - 1) / kWaves;
    prof_begin(c, "post_sample");
    post_sample_kernel<<<flat_grid(blocks), kB, 0, c->stream>>>(s.d_sets.p, s.d_scores.p, s.d_offsets.p, s.alpha.p, s.f.p, n, seed,
                                                                first, count, with_u ? s.s_u.p : nullptr, s.s_parents.p,
                                                                order ? s.s_order.p : nullptr, log_weight ? s.s_weight.p : nullptr,
                                                                s.s_err.p);
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    unsigned int err = 0;
    ULG_HIP(c, hipMemcpyAsync(&err, s.s_err.p, sizeof(err), hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (err) return set_err(c, ULG_ERR_STATE, name + ": a step found no candidate of positive weight");
    ULG_HIP(c, hipMemcpyAsync(parents, s.s_parents.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (order) ULG_HIP(c, hipMemcpyAsync(order, s.s_order.p, cells, hipMemcpyDeviceToHost, c->stream));
    if (log_weight) ULG_HIP(c, hipMemcpyAsync(log_weight, s.s_weight.p, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    return ULG_OK;
}

}  // namespace

extern "C" {

int ulg_posterior_sample(ulg_ctx *c, uint64_t seed, int64_t first, int64_t count, uint64_t *parents, uint8_t *order,
                         double *log_weight) {
    return sample(c, "ulg_posterior_sample", seed, first, count, nullptr, false, parents, order, log_weight);
}

int ulg_posterior_sample_u(ulg_ctx *c, int64_t count, const uint64_t *u, uint64_t *parents, uint8_t *order, double *log_weight) {
    return sample(c, "ulg_posterior_sample_u", 0, 0, count, u, true, parents, order, log_weight);
}

}  // extern "C"
