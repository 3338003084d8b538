// cbic_score_layer.inc -- the body of score_layer_kernel, included once per
// form: ULG_CONS 0 (cbic_layers.hip) is score_layer_kernel, 1
// (cbic_layers_cons.hip) its constrained twin score_layer_cons_kernel (launched while the context holds
// constraints): a set that violates its variable's constraints takes
// ts = float(n) (BIC_OLS.cpp:279-283) without a regression, and everything
// after ts is the same text.  Two kernels from one text, not one template
// with a flag: the unconstrained kernels keep the code, and so the register
// allocation, they had before constraints existed (DESIGN.md 3.1h).
// NARROW (DESIGN.md 3.1p; a launch CbicPlan::launch_narrow picks): every set
// mask, rank, launch-local index and table slot of the launch fits 32 bits,
// and M, the type that carries them, is uint32_t -- one register and one
// instruction where the 64-bit form spends two or more.  The integers, the
// LDS layout and every floating-point expression are the same.
template <int L, int PHASE, int V, bool NARROW = false>
__global__ void __launch_bounds__(kBlock, (score_min_waves<L, PHASE, V>()))
#if ULG_CONS
score_layer_cons_kernel(ScoreArgs a, const uint64_t *cons, int cons_words) {
#else
score_layer_kernel(ScoreArgs a) {
#endif
    using M = std::conditional_t<NARROW, uint32_t, uint64_t>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LdsLayout lay = lds_layout(a.n, a.nv, a.S, L, V);
#if ULG_CONS
    const uint64_t *ct = cons_stage<kBlock>(smem, lay.total, cons, cons_words);
#endif
    double *g = reinterpret_cast<double *>(smem + lay.gram);
    uint32_t *binom = reinterpret_cast<uint32_t *>(smem + lay.binom);
    uint64_t *work = reinterpret_cast<uint64_t *>(smem + lay.work);
    uint64_t *toff = reinterpret_cast<uint64_t *>(smem + lay.toff);
    // the per-variable metadata and candidate lists too: every lane reads
    // them right after its variable is known, and from global memory those
    // would be two more dependent round trips per lane
    int *smeta = reinterpret_cast<int *>(smem + lay.meta);
    uint8_t *scand = reinterpret_cast<uint8_t *>(smem + lay.cand);
    constexpr bool HM = (V & 64) != 0;           // subset maxima kept up to date
    constexpr bool CMP = HM && (V & 16) != 0;     // ... and the sets settled by them first
    // The launch image (a.image, wave-uniform): the block's constants as one
    // flat run of 16-byte pieces, thread t taking pieces t, t + kBlock, ...
    // The loads of up to four passes (every n <= 32) are issued here, ahead
    // of the variable search's scalar round trips and the table read, and
    // written to LDS in front of the barrier; an index past the image reads
    // its last piece again and writes nothing.
    const uint32_t n16 = (uint32_t)a.image16;
    const auto piece = [&](uint32_t j) {  // pass j's piece of this thread, when the image reaches that pass
        // a 32-bit byte offset off the image's base in SGPRs, not a 64-bit pointer per lane
        const uint32_t i = threadIdx.x + j * kBlock, at = (i < n16 ? i : n16 - 1u) << 4;
        return (a.image && j * kBlock < n16)
                   ? *reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(a.image) + at)
                   : uint4{0u, 0u, 0u, 0u};
    };
    const uint4 im0 = piece(0), im1 = piece(1), im2 = piece(2), im3 = piece(3);
    // the wave's variable on the scalar unit, and with it the lane's unrank
    // table entry, before the fill (wave_variable, cbic_layer_dev.h)
    const M gid0 = (M)xcd_block(blockIdx.x, gridDim.x, a.xcd) * kBlock + threadIdx.x;
    const WaveVar wv = wave_variable(a.work, a.lut_off, a.nv, a.total, gid0 - (threadIdx.x & 63u));
    const M wtotal = (M)wv.total, wbase = (M)wv.base;  // wave-uniform; NARROW: below 2^32 with a block to spare
    const bool valid = gid0 < wtotal;
    // CMP: every lane reaches the block's barrier; a lane past the launch's
    // sets scores the last one again and writes nothing
    const M gid = valid ? gid0 : wtotal - 1;
    bool have_um = false;
    uint32_t um = 0u;
    if (wv.vi >= 0 && wv.loff >= 0) {
        um = a.lut[(uint32_t)wv.loff + (uint32_t)(gid - wbase)];
        have_um = true;
    }
    int32_t *slut = reinterpret_cast<int32_t *>(smem + lay.lutoff);
    if (a.image) {
        uint4 *simg = reinterpret_cast<uint4 *>(smem);
        const uint32_t t = threadIdx.x;
        if (t < n16) simg[t] = im0;
        if (t + kBlock < n16) simg[t + kBlock] = im1;
        if (t + 2u * kBlock < n16) simg[t + 2u * kBlock] = im2;
        if (t + 3u * kBlock < n16) simg[t + 3u * kBlock] = im3;
        for (uint32_t i = threadIdx.x + 4u * kBlock; i < n16; i += kBlock) simg[i] = a.image[i];
    } else {
        for (int i = threadIdx.x; i < a.n * a.n; i += kBlock) g[i] = a.gram[i];
        for (int i = threadIdx.x; i < 64 * kBinomK; i += kBlock) binom[i] = a.binom[i];
        for (int i = threadIdx.x; i <= a.nv; i += kBlock) work[i] = a.work[i];
        // the table offsets beside them: a straddling wave's lanes read theirs
        // from LDS, not in a round trip of its own in front of the table read
        if (a.lut_off)
            for (int i = threadIdx.x; i < a.nv; i += kBlock) slut[i] = a.lut_off[i];
        for (int i = threadIdx.x; i <= a.nv * a.S; i += kBlock) toff[i] = a.tbl_off[i];
        for (int i = threadIdx.x; i < a.nv * 4; i += kBlock) smeta[i] = a.meta[i];
        for (int i = threadIdx.x; i < a.nv * 16; i += kBlock)
            reinterpret_cast<uint32_t *>(scand)[i] = reinterpret_cast<const uint32_t *>(a.cand)[i];
    }
    __syncthreads();

    if (!CMP && !valid) return;
    int vi = wv.vi;
    M r = gid - wbase;
    if (wv.vi < 0) {  // the wave straddles variables: each lane finds its own
        int lo = 0, hi = a.nv;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (low_entry<M>(work, mid) <= gid) lo = mid; else hi = mid;
        }
        vi = lo;
        r = gid - low_entry<M>(work, vi);
        if (a.lut_off) {
            const int32_t lo2 = slut[vi];
            if (lo2 >= 0) {
                um = a.lut[(uint32_t)lo2 + (uint32_t)r];
                have_um = true;
            }
        }
    }
    // CMP: the set's rank comes out of child_ranks below
    const SetHead<L, M> hd = set_head<L, PHASE, !CMP, M>(smeta, scand, binom, vi, r, have_um, um);
    const bool z = hd.z;
    const M cm = hd.cm;

#if ULG_CONS
    float ts = (float)a.n;
    if (!cons_violates(ct, a.nv, vi, cm)) ts = cbic_set_score<L>(g, a.n, hd.v, hd.gv, a.N, a.pen);
#else
    const float ts = cbic_set_score<L>(g, a.n, hd.v, hd.gv, a.N, a.pen);
#endif

    if constexpr (CMP) {
        // 1. settle by the subset maxima: ts >= 0, no key >= -ts in U(P), or a
        //    present direct child >= -ts (always visited at the top level)
        const M vbase = (M)vi * a.S;
        M rc[L], rz[L];
        const M rankP = child_ranks<L, PHASE == 1>(cm, binom, rc, rz);
        const M slot = low_entry<M>(toff, vbase + L) + rankP;
        // every load of the settle issued at once (the children's maxima and
        // values, the var-0 toggles' maxima): one memory round trip instead
        // of up to three dependent ones
        float hch = absent_f();  // max over the proper nonempty subsets of P
        float hz = absent_f();   // ... and over the toggles P\a + {0}
        bool dh = false;         // a direct child >= -ts
#ifdef ULG_GATHER_STATS
        uint32_t hotA = 0u;      // children P\a_i holding a key >= -ts (hsub)
        uint32_t hotZ = 0u;      // toggled children P\a_i + {0} holding one
#endif
        {
            float ch[L], cv[L], zv[L];
            // a child's slot: 32-bit either way; NARROW turns it into a 32-bit
            // byte offset beside the table's base (slot_ptr), not a 64-bit address per load
            using S32 = std::conditional_t<NARROW, uint32_t, uint64_t>;
            const uint32_t o1 = (uint32_t)low_entry<M>(toff, vbase + L - 1), o0 = (uint32_t)low_entry<M>(toff, vbase + L);
#pragma unroll
            for (int i = 0; i < L; ++i) {
                if constexpr (L > 1) {
                    ch[i] = *slot_ptr(a.hsub, (S32)(o1 + (uint32_t)rc[i]));
                    cv[i] = *slot_ptr(a.table, (S32)(o1 + (uint32_t)rc[i]));
                }
                if constexpr (PHASE == 1) zv[i] = *slot_ptr(a.hsub, (S32)((z ? o0 : 0u) + (z ? (uint32_t)rz[i] : 0u)));
            }
            const float thr = -ts;
#pragma unroll
            for (int i = 0; i < L; ++i) {
                if constexpr (L > 1) {
                    hch = fmaxf(hch, ch[i]);
                    dh |= cv[i] >= thr;
#ifdef ULG_GATHER_STATS
                    hotA |= (ch[i] >= thr) ? 1u << i : 0u;
#endif
                }
                if constexpr (PHASE == 1) {
                    hz = fmaxf(hz, zv[i]);
#ifdef ULG_GATHER_STATS
                    hotZ |= (zv[i] >= thr) ? 1u << i : 0u;
#endif
                }
            }
            if (!z) hz = absent_f();
#ifdef ULG_GATHER_STATS
            if (!z) hotZ = 0u;
#endif
        }
        bool need = false;
        float out;
        if (ts >= 0.0f) {
            const float s = -ts;
            out = (s < 0.0f) ? s : absent_f();
        } else {
            const float thr = -ts;
            const float hu = fmaxf(hch, hz);
            out = -ts;
            if (hu >= thr) {
                out = absent_f();
                need = !dh;
            }
        }
        if (valid && !need) {
            *slot_ptr(a.table, slot) = out;
            if (a.hsub_out) *slot_ptr(a.hsub, slot) = fmaxf(out, hch);
        }
        // 2. the rest of the block's sets, compacted in LDS, so the presence
        //    gathers (2^(L+1) reads each) run on dense waves
        unsigned int *cnt = reinterpret_cast<unsigned int *>(smem + lay.cmp);
        // (NARROW: 4-byte masks fill the first half of the masks' column; the carve is the same)
        M *ecm = reinterpret_cast<M *>(smem + lay.cmp + 16);
        uint32_t *eslot = reinterpret_cast<uint32_t *>(smem + lay.cmp + 16 + kBlock * 8);
        float *ets = reinterpret_cast<float *>(eslot + kBlock);
        float *ehch = ets + kBlock;
        int *evi = reinterpret_cast<int *>(ehch + kBlock);
        if (threadIdx.x == 0) {
            cnt[0] = 0u;
            cnt[1] = 0u;  // the second compaction's count (variant bit 7)
        }
        __syncthreads();
        if (valid && need) {
            const unsigned int k = atomicAdd(cnt, 1u);
            ecm[k] = cm;
            eslot[k] = (uint32_t)slot;
            ets[k] = ts;
            ehch[k] = hch;
#ifdef ULG_GATHER_STATS
            evi[k] = vi | (int)(hotA << 8) | (int)(hotZ << 16);
#else
            evi[k] = vi;
#endif
        }
        __syncthreads();
        constexpr int W = bits_words(L);
        using BS = std::conditional_t<(W >= 4), BitsLds<W>, Bits<W>>;
        constexpr bool CMP2 = (V & 128) != 0 && W < 4;
        if constexpr (!CMP2)
            if (threadIdx.x >= *cnt) return;
        const int k = threadIdx.x;
        const bool a1 = threadIdx.x < cnt[0];
        const uint64_t seg = walk_segment();
        // this lane's compacted set (the lanes past the count, variant bit 7
        // only, carry a dummy and gather nothing)
        const int vk = a1 ? evi[k] & 0xff : 0;
#ifdef ULG_GATHER_STATS
        const uint32_t hk = a1 ? (uint32_t)evi[k] >> 8 : 0u;  // hotA | hotZ << 8
#endif
        const bool zk = smeta[vk * 4 + 2] != 0;
        const float tk = a1 ? ets[k] : -1.0f;
        const M sk = a1 ? eslot[k] : 0u;
        const M cmk = a1 ? ecm[k] : (M)1;
        const float hk1 = a1 ? ehch[k] : absent_f();
        uint64_t *lds_bits = reinterpret_cast<uint64_t *>(smem + lay.bits) + threadIdx.x;
        const LocalSet<L> ls = local_set<L, PHASE>(cmk, zk);
        BS present = make_bits<BS>(lds_bits);
        BS hib = make_bits<BS>(lds_bits + (size_t)W * kBlock);
        present.clear();
        hib.clear();
        bool q = false;
        if (a1) {
            // the keys the two-level rules read first; the rest only for the
            // sets the rules leave to the walk (the subset maxima already
            // showed a key >= -ts is present, so the rules need no "any key"
            // test)
            gather_keys<L, PHASE, V, BS, LdPlain, 1>(present, hib, ls, -tk, binom, zk, a.table,
                                                    toff_row<M>(toff, vk, a.S));
            const bool dom = settle_rules<L, PHASE, BS, true>(present, hib, ls, q);
#ifdef ULG_GATHER_STATS
            if constexpr (W < 4) {
                BS p2 = make_bits<BS>(lds_bits), h2 = make_bits<BS>(lds_bits);
                p2.clear();
                h2.clear();
                gather_keys<L, PHASE, V, BS, LdPlain, 0>(p2, h2, ls, -tk, binom, zk, a.table,
                                                        toff_row<M>(toff, vk, a.S));
                gather_stats<L, PHASE>(p2, h2, hk & 0xffu, hk >> 8, zk, q);
            }
#endif
            if (!q) {
                const float o = dom ? absent_f() : -tk;
                *slot_ptr(a.table, sk) = o;
                if (a.hsub_out) *slot_ptr(a.hsub, sk) = fmaxf(o, hk1);
            }
        }
        if constexpr (CMP2) {
            // 3. the sets the rules leave to the walk (about a third of the
            //    compacted ones) compacted once more, with their gathered
            //    words, so the rest of the gathers, the walk closure and the
            //    queue run on dense waves: at ~30 % of the lanes every wave
            //    would still issue them
            uint64_t *c2w = reinterpret_cast<uint64_t *>(smem + lay.cmp2);  // [2W][kBlock]
            __syncthreads();  // every lane has read its first entry
            if (q) {
                const unsigned int k2 = atomicAdd(cnt + 1, 1u);
                ecm[k2] = cmk;
                eslot[k2] = (uint32_t)sk;
                ets[k2] = tk;
                ehch[k2] = hk1;
                evi[k2] = vk;
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    c2w[j * kBlock + k2] = present.word(j);
                    c2w[(W + j) * kBlock + k2] = hib.word(j);
                }
            }
            __syncthreads();
            if (threadIdx.x >= cnt[1]) return;
            const int vq = evi[k];
            const bool zq = smeta[vq * 4 + 2] != 0;
            const float tq = ets[k];
            const M sq = eslot[k];
            const float hq = ehch[k];
            const LocalSet<L> lq = local_set<L, PHASE>(ecm[k], zq);
            BS pq = make_bits<BS>(lds_bits), hq_bits = make_bits<BS>(lds_bits);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                pq.w[j] = c2w[j * kBlock + k];
                hq_bits.w[j] = c2w[(W + j) * kBlock + k];
            }
            walk_or_store<L, PHASE, V, BS>(a, pq, hq_bits, lq, tq, binom, zq, toff_row<M>(toff, vq, a.S), seg, sq, hq);
        } else {
            if (q)
                walk_or_store<L, PHASE, V, BS>(a, present, hib, ls, tk, binom, zk, toff_row<M>(toff, vk, a.S), seg, sk,
                                               hk1);
        }
        return;
    }

    one_pass_set<L, PHASE, V>(a, smem, lay, binom, toff, vi, z, cm, hd.rankP, ts);
}

// This form's kernel for (layer, phase, variant, narrow): the host's dispatch,
// one text for both forms like the kernel above.
#if ULG_CONS
#define ULG_LAYER_KERNEL score_layer_cons_kernel
#else
#define ULG_LAYER_KERNEL score_layer_kernel
#endif
using LayerFn = TwinFn<ULG_CONS != 0, ScoreArgs>;
template <int L, int V, bool NARROW = false>
LayerFn pick_phase(int phase) {
    return phase == 0 ? ULG_LAYER_KERNEL<L, 0, V, NARROW> : ULG_LAYER_KERNEL<L, 1, V, NARROW>;
}
// variants (ulg_set_option "score_variant"): bit 0 unrolled presence gathers
// (layers <= 6), bit 4 two-pass (settle, queue the rest for a walk launch),
// bit 5 bit-sliced walk, bit 6 subset maxima.  1: one-pass (also the form for
// tables of 2^30 slots or more); 65: one-pass with the subset maxima (the
// small layers of 113); 49: two-pass with the bit-sliced walk (the tests'
// every-set-gathered reference); 113: the same with the subset maxima (the
// default).  Gone after measurement: round 4's per-lane walk forms 17 / 81
// and a variant that walked the open sets inside the scoring kernel (C5 5.05
// against 3.59 ms: a 64-set union tree repeats work a 256-set one shares);
// round 1's loop gathers at every layer, stack-machine recursion,
// decision-only per-lane walk and statistics build.
// narrow: the launch's 32-bit form (CbicPlan::launch_narrow), built where
// CbicPlan::narrow_built says so: the default variant's layers 5 and 6
template <int L>
LayerFn pick(int phase, int variant, bool narrow) {
    if constexpr (CbicPlan::narrow_built(L, 241))
        if (narrow && variant == 241) return pick_phase<L, 209, true>(phase);
    if (narrow) return nullptr;
    switch (variant) {
        case 1: return pick_phase<L, 1>(phase);
        case 49: return pick_phase<L, 17>(phase);
        case 65: return pick_phase<L, 65>(phase);
        case 113: return pick_phase<L, 81>(phase);
        case 241: return pick_phase<L, 209>(phase);
        default: return nullptr;
    }
}
LayerFn layer_kernel(int L, int phase, int variant, bool narrow = false) {
    switch (L) {
        case 1: return pick<1>(phase, variant, narrow);
        case 2: return pick<2>(phase, variant, narrow);
        case 3: return pick<3>(phase, variant, narrow);
        case 4: return pick<4>(phase, variant, narrow);
        case 5: return pick<5>(phase, variant, narrow);
        case 6: return pick<6>(phase, variant, narrow);
        case 7: return pick<7>(phase, variant, narrow);
        case 8: return pick<8>(phase, variant, narrow);
        default: return nullptr;
    }
}
static_assert(kMaxL == 8, "layer_kernel dispatch covers layers 1..8");
#undef ULG_LAYER_KERNEL
