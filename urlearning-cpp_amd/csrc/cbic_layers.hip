// cbic_layers.hip -- the unrolled layer kernels (layers 1..8, one lane per
// parent set) and the fused small layers of the cBIC scorer, unconstrained
// form, with their launches.  The constrained twins: cbic_layers_cons.hip.
// See cbic.hip for the design and cbic_call.h for the file map.

#include "search_internal.h"
#include "cbic_call.h"

using namespace ulg;

namespace {

// PHASE 0: sets containing variable 0; 1: the rest.  V = variant bits (see
// ulg_set_option "score_variant"), compile-time so each form gets its own
// register allocation.
#define ULG_CONS 0
#include "cbic_score_layer.inc"
#include "cbic_score_small.inc"
#undef ULG_CONS

const char *kLayerNames[2][kMaxL + 1] = {
    {"", "score_layer_1_var0", "score_layer_2_var0", "score_layer_3_var0", "score_layer_4_var0",
     "score_layer_5_var0", "score_layer_6_var0", "score_layer_7_var0", "score_layer_8_var0"},
    {"", "score_layer_1_rest", "score_layer_2_rest", "score_layer_3_rest", "score_layer_4_rest",
     "score_layer_5_rest", "score_layer_6_rest", "score_layer_7_rest", "score_layer_8_rest"}};

// The launch image of layer launch (g, L, ph), when the call built one.
void set_image(const ScoreCall &k, ScoreArgs &sa, int g, int L, int ph) {
    const int64_t at = k.p.image_offset(g, L, ph);
    sa.image = at < 0 ? nullptr : reinterpret_cast<const uint4 *>(k.c->d_image.p + at);
    sa.image16 = at < 0 ? 0 : k.p.image_bytes(k.ls, L) / 16;
}

}  // namespace

namespace ulg {

// A small layer phase (L <= p.Ls) on the context stream, one-pass over all
// variables; layers <= p.Lf run together in one fused launch, sent at (1, 0).
int launch_small(const ScoreCall &k, int L, int ph) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    const int n = k.ls.n, nv = p.nv, S = k.ls.S;
    ScoreArgs ss = k.sa;
    if (L <= p.Lf) {
        if (L != 1 || ph != 0) return ULG_OK;
        ss.hsub_out = p.Lf < p.kmax;  // layer Lf's phase 1 maxima: read only by a layer above
        return launch_twin(c, k.cons, small_kernel(p.Lf), small_cons_kernel(p.Lf), dim3((unsigned)nv),
                           dim3(kFusedThreads), lds_layout(n, nv, S, p.Lf, 65).total, c->stream, "score_small_fused",
                           ss, (const uint64_t *)c->d_work.p);
    }
    const size_t wo = p.work_offset(0, L, ph);
    const uint64_t cnt = p.work[wo + nv];
    if (cnt == 0) return ULG_OK;
    ss.work = c->d_work.p + wo;
    ss.total = cnt;
    ss.lut_off = p.lut_any ? c->d_lutoff.p + p.lut_offset(L, ph) : nullptr;
    set_image(k, ss, 0, L, ph);
    ss.hsub_out = !(L == p.kmax && ph == 1);
    return launch_twin(c, k.cons, layer_kernel(L, ph, p.vsmall), layer_cons_kernel(L, ph, p.vsmall, false),
                       dim3((unsigned)((cnt + kBlock - 1) / kBlock)), dim3(kBlock),
                       lds_layout(n, nv, S, L, p.vsmall).total, c->stream, kLayerNames[ph][L], ss);
}

// An unrolled layer phase of stream group g: its scoring launch, then (the
// two-pass variants) the walk of the undecided lanes it queued, densely
// packed, in bucketed or queue order.
int launch_unrolled(const ScoreCall &k, int g, int L, int ph) {
    ulg_ctx *c = k.c;
    const CbicPlan &p = k.p;
    const uint64_t cnt = p.launch_count(g, L, ph);
    if (cnt == 0) return ULG_OK;
    const uint64_t blocks = (cnt + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_cbic_score: layer too large");
    const bool two_pass = (p.variant & 16) != 0;
    const bool bk = p.bucket && (L == 5 || L == 6);
    ScoreArgs sa = k.sa;
    sa.work = k.d_wk + p.work_offset(g, L, ph);
    sa.total = cnt;
    sa.lut_off = p.lut_any ? c->d_lutoff.p + p.lut_offset(L, ph) : nullptr;
    set_image(k, sa, g, L, ph);
    sa.queue = two_pass ? c->d_queue.p + (size_t)g * p.qwords : nullptr;
    sa.qcount = two_pass ? c->d_qseg.p + p.segoff[p.seg_slot(g, L, ph)] : nullptr;
    sa.qkey = bk ? c->d_qkey.p + (size_t)g * p.qcap : nullptr;
    // nothing reads the subset maxima of the top layer's second phase
    sa.hsub_out = !(L == p.kmax && ph == 1);
    const bool nw = p.launch_narrow(g, L, ph);
    if (nw && !layer_kernel(L, ph, p.variant, true))
        return set_err(c, ULG_ERR_STATE, "ulg_cbic_score: no narrow kernel for a launch planned narrow");
    int rc;
    if ((rc = launch_twin(c, k.cons, layer_kernel(L, ph, p.variant, nw), layer_cons_kernel(L, ph, p.variant, nw),
                          dim3((unsigned)blocks), dim3(kBlock), lds_layout(k.ls.n, p.nv, k.ls.S, L, p.variant).total,
                          k.gst[g], kLayerNames[ph][L], sa)))
        return rc;
    if (!two_pass) return ULG_OK;
    const int wk = sliced_k(L, cnt, (uint64_t)c->opt.walk_small_sets, c->opt.walk_k6);
    if (bk) return walk_bucketed(k, g, L, ph, sa, blocks, wk);
    if (p.variant & 32) return walk_sliced(k, g, L, ph, sa, blocks, wk);
    return ULG_OK;
}

}  // namespace ulg

extern "C" {

#ifdef ULG_GATHER_STATS
// diagnostic build: the gather counters (2 * (kMaxL + 1) * 16 values), then
// the walk's hits by depth (as many), both zeroed
int ulg_diag_gather_stats(ulg_ctx *c, unsigned long long *out) {
    if (!c || !out) return ULG_ERR_ARG;
    ULG_HIP(c, hipSetDevice(c->device));
    ULG_HIP(c, hipStreamSynchronize(c->stream));
    ULG_HIP(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gstats), sizeof(g_gstats)));
    static const unsigned long long zero[2 * (kMaxL + 1) * 16] = {};
    ULG_HIP(c, hipMemcpyToSymbol(HIP_SYMBOL(g_gstats), zero, sizeof(zero)));
    return walk_hit_stats(c, out + 2 * (kMaxL + 1) * 16);  // the walk kernels' copy: cbic_walk.hip
}
#endif

}  // extern "C"
