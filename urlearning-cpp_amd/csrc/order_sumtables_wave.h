// order_sumtables_wave.h -- what the two run kernels over the log-sum tables
// share (ostab_run_kernel of order_sumtables.hip, opick_run_kernel of
// order_picktables.hip): the cross-lane reads of a wave64 and what lane p holds
// of the variable at position p.  Device only; each of the two files includes
// it into its own unnamed namespace.
#pragma once

#include "order_mcmc_run.h"
#include "order_sumtables_dev.h"

namespace {

using namespace ulg;

constexpr int kWave = kMcmcWave;
constexpr int kRunWaves = 4;  // chains per workgroup of the run kernels

__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t x, int d) { return __shfl_xor((unsigned long long)x, d, kWave); }
__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, int d) { return __shfl_up((unsigned long long)x, d, kWave); }

// lane r's value in every lane, r wave-uniform: two scalar reads, no LDS crossbar
__device__ __forceinline__ int lane_get(int x, int r) { return __builtin_amdgcn_readlane(x, r); }
__device__ __forceinline__ uint64_t lane_get64(uint64_t x, int r) {
    const uint32_t lo = (uint32_t)lane_get((int)(uint32_t)x, r), hi = (uint32_t)lane_get((int)(uint32_t)(x >> 32), r);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double lane_getd(double x, int r) { return __longlong_as_double((long long)lane_get64((uint64_t)__double_as_longlong(x), r)); }

// What lane p holds of the variable v at its position: C_v, the table's first
// slot, the variables at the lanes below and their table index (on: lane < n).
struct Place {
    uint64_t C, pre;
    int64_t base;
    uint32_t idx;
};
__device__ __forceinline__ Place place_of(const uint64_t *cand, const int64_t *toff, int v, bool on, int lane) {
    const uint64_t own = on ? 1ull << v : 0ull;
    uint64_t U = own;  // the prefix OR across the lanes, this one included
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t o = shfl_up64(U, d);
        if (lane >= d) U |= o;
    }
    Place r;
    r.C = on ? cand[v] : 0ull, r.base = on ? toff[v] : 0;
    r.pre = U & ~own;
    r.idx = ot_index(r.C, r.pre);
    return r;
}

}  // namespace
