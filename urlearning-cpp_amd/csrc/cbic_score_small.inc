// cbic_score_small.inc -- the fused small layers (score_small_kernel and its
// fused_phase), included once per form: ULG_CONS 0 (cbic_layers.hip) is the kernel
// as it is without constraints, 1 (cbic_layers_cons.hip) its constrained twin (*_cons_kernel,
// launched while the context holds constraints); see cbic_score_layer.inc.
#if ULG_CONS
#define ULG_FUSED_PHASE fused_phase_cons
#else
#define ULG_FUSED_PHASE fused_phase
#endif
template <int L, int PHASE, int LF, int V>
__device__ __forceinline__ void ULG_FUSED_PHASE(const ScoreArgs &a, const uint64_t *work_all, unsigned char *smem,
                                            const LdsLayout &lay, const double *g, const uint32_t *binom,
                                            const uint64_t *toff, const int *smeta, const uint8_t *scand, int vi
#if ULG_CONS
                                            , const uint64_t *ct
#endif
                                            ) {
    const uint64_t *w = work_all + ((uint64_t)L * 2 + PHASE) * (uint64_t)(a.nv + 1);
    const uint64_t cnt = w[vi + 1] - w[vi];
    ScoreArgs as = a;
    as.hsub_out = a.hsub_out || !(L == LF && PHASE == 1);
    for (uint64_t r = threadIdx.x; r < cnt; r += kFusedThreads) {
        const SetHead<L> hd = set_head<L, PHASE>(smeta, scand, binom, vi, r);
#if ULG_CONS
        float ts = (float)a.n;
        if (!cons_violates(ct, a.nv, vi, hd.cm)) ts = cbic_set_score<L>(g, a.n, hd.v, hd.gv, a.N, a.pen);
#else
        const float ts = cbic_set_score<L>(g, a.n, hd.v, hd.gv, a.N, a.pen);
#endif
        one_pass_set<L, PHASE, V>(as, smem, lay, binom, toff, vi, hd.z, hd.cm, hd.rankP, ts);
    }
    __syncthreads();
#if ULG_CONS
    if constexpr (PHASE == 0)
        ULG_FUSED_PHASE<L, 1, LF, V>(a, work_all, smem, lay, g, binom, toff, smeta, scand, vi, ct);
    else if constexpr (L < LF)
        ULG_FUSED_PHASE<L + 1, 0, LF, V>(a, work_all, smem, lay, g, binom, toff, smeta, scand, vi, ct);
#else
    if constexpr (PHASE == 0) fused_phase<L, 1, LF, V>(a, work_all, smem, lay, g, binom, toff, smeta, scand, vi);
    else if constexpr (L < LF) fused_phase<L + 1, 0, LF, V>(a, work_all, smem, lay, g, binom, toff, smeta, scand, vi);
#endif
}
// a.hsub_out: whether layer LF's phase 1 writes the subset maxima (read by a
// layer above LF); a.work unused (work_all: every (layer, phase) prefix)
template <int LF, int V>
#if ULG_CONS
__global__ void __launch_bounds__(kFusedThreads)
score_small_cons_kernel(ScoreArgs a, const uint64_t *work_all, const uint64_t *cons, int cons_words) {
#else
__global__ void __launch_bounds__(kFusedThreads) score_small_kernel(ScoreArgs a, const uint64_t *work_all) {
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LdsLayout lay = lds_layout(a.n, a.nv, a.S, LF, V);
#if ULG_CONS
    const uint64_t *ct = cons_stage<kFusedThreads>(smem, lay.total, cons, cons_words);
#endif
    double *g = reinterpret_cast<double *>(smem + lay.gram);
    uint32_t *binom = reinterpret_cast<uint32_t *>(smem + lay.binom);
    uint64_t *toff = reinterpret_cast<uint64_t *>(smem + lay.toff);
    int *smeta = reinterpret_cast<int *>(smem + lay.meta);
    uint8_t *scand = reinterpret_cast<uint8_t *>(smem + lay.cand);
    for (int i = threadIdx.x; i < a.n * a.n; i += kFusedThreads) g[i] = a.gram[i];
    for (int i = threadIdx.x; i < 64 * kBinomK; i += kFusedThreads) binom[i] = a.binom[i];
    for (int i = threadIdx.x; i <= a.nv * a.S; i += kFusedThreads) toff[i] = a.tbl_off[i];
    for (int i = threadIdx.x; i < a.nv * 4; i += kFusedThreads) smeta[i] = a.meta[i];
    for (int i = threadIdx.x; i < a.nv * 16; i += kFusedThreads)
        reinterpret_cast<uint32_t *>(scand)[i] = reinterpret_cast<const uint32_t *>(a.cand)[i];
    __syncthreads();
#if ULG_CONS
    ULG_FUSED_PHASE<1, 0, LF, V>(a, work_all, smem, lay, g, binom, toff, smeta, scand, (int)blockIdx.x, ct);
#else
    fused_phase<1, 0, LF, V>(a, work_all, smem, lay, g, binom, toff, smeta, scand, (int)blockIdx.x);
#endif
}
#undef ULG_FUSED_PHASE

// This form's kernel for the fused layers 1..Lf (the host's dispatch).
#if ULG_CONS
#define ULG_SMALL_KERNEL score_small_cons_kernel
#else
#define ULG_SMALL_KERNEL score_small_kernel
#endif
TwinFn<ULG_CONS != 0, ScoreArgs, const uint64_t *> small_kernel(int Lf) {
    switch (Lf) {
        case 1: return ULG_SMALL_KERNEL<1, 65>;
        case 2: return ULG_SMALL_KERNEL<2, 65>;
        case 3: return ULG_SMALL_KERNEL<3, 65>;
        default: return ULG_SMALL_KERNEL<4, 65>;
    }
}
#undef ULG_SMALL_KERNEL
