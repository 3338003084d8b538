// cbic_call.h -- the cBIC scoring call on the host, as its translation units
// share it: the call's state (ScoreCall), a launch under its profiling name
// (launch_kernel, launch_twin) and the launch steps that cross files.
//   cbic.hip             the call: plan, buffers, prologue, layer order, compaction, graph, C ABI
//   cbic_layers.hip      launch_small, launch_unrolled (the unconstrained layer kernels)
//   cbic_layers_cons.hip the constrained twins, handed out by layer_cons_kernel / small_cons_kernel
//   cbic_walk.hip        walk_bucketed, walk_sliced, sliced_k
//   cbic_wide.hip        launch_wide_grouped, wide_pool
#pragma once
#include <type_traits>
#include <vector>

#include "search_internal.h"
#include "cbic_layer_dev.h"

namespace ulg {

// the call's constraint table on the device (words 0: the unconstrained kernels)
struct ConsTable {
    const uint64_t *dev;
    int words, lds;
};

// What the launch steps of one scoring call share.
struct ScoreCall {
    ulg_ctx *c;
    const ScoreLists &ls;
    const CbicPlan &p;
    ConsTable cons;
    ScoreArgs sa;                  // the fields every layer launch shares
    const uint64_t *d_wk;          // the stream groups' work prefixes (p.group_work()) on the device
    std::vector<hipStream_t> gst;  // each group's stream; group 0 is the context's
    const char *wck;               // ULG_WALK_CLOCK: walk diagnostics (synchronising)
    unsigned long long *errf() const { return p.zero_q ? c->d_qcount.p + p.nqc - 1 : nullptr; }
};

// One launch on stream st under its profiling name; LDS above 64 KiB is asked for first.
template <class Fn, class... A>
int launch_kernel(ulg_ctx *c, Fn fn, dim3 grid, dim3 block, int lds, hipStream_t st, const char *name, A... args) {
    if (lds > 64 * 1024)
        ULG_HIP(c, hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    prof_begin_s(c, name, st);
    hipLaunchKernelGGL(fn, grid, block, (size_t)lds, st, args...);
    prof_end_s(c, st);
    return ULG_OK;
}
// A scoring launch: kernel fn, or under constraints its twin cfn, which takes
// the table and its words after the common arguments and stages the table in
// LDS behind the kernel's own layout.
template <class Fn, class ConsFn, class... A>
int launch_twin(ulg_ctx *c, const ConsTable &ct, Fn fn, ConsFn cfn, dim3 grid, dim3 block, int lds, hipStream_t st,
                const char *name, A... args) {
    if (!ct.words) return launch_kernel(c, fn, grid, block, lds, st, name, args...);
    return launch_kernel(c, cfn, grid, block, align16(lds) + ct.lds, st, name, args..., ct.dev, ct.words);
}

// A scoring kernel's type, or with CONS its constrained twin's (*_cons_kernel:
// the call's constraint table and its words after the common arguments); the
// dispatch functions (the ends of cbic_score_layer.inc and cbic_score_small.inc)
// pick either by the same (layer, phase, variant).
template <bool CONS, class... A>
using TwinFn = std::conditional_t<CONS, void (*)(A..., const uint64_t *, int), void (*)(A...)>;

// ---- the steps that cross translation units ----------------------------------
// cbic_layers.hip
int launch_small(const ScoreCall &k, int L, int ph);
int launch_unrolled(const ScoreCall &k, int g, int L, int ph);
// cbic_layers_cons.hip: the constrained twin of layer_kernel(L, phase, variant,
// narrow) and of small_kernel(Lf), null where the unconstrained one is
TwinFn<true, ScoreArgs> layer_cons_kernel(int L, int phase, int variant, bool narrow);
TwinFn<true, ScoreArgs, const uint64_t *> small_cons_kernel(int Lf);
// cbic_walk.hip
int walk_bucketed(const ScoreCall &k, int g, int L, int ph, const ScoreArgs &sa, uint64_t blocks, int wk);
int walk_sliced(const ScoreCall &k, int g, int L, int ph, const ScoreArgs &sa, uint64_t blocks, int wk);
int sliced_k(int L, uint64_t cnt, uint64_t small, int k6);
#ifdef ULG_GATHER_STATS
int walk_hit_stats(ulg_ctx *c, unsigned long long *out);  // diagnostic build: ulg_diag_gather_stats' second half
#endif
// cbic_wide.hip
int launch_wide_grouped(const ScoreCall &k, int L, int ph);
int wide_pool(const ScoreCall &k);

}  // namespace ulg
