// cbic_score_wide.inc -- included by cbic_wide.hip once per form: ULG_CONS 0 is the kernel as it
// is without constraints, 1 its constrained twin (*_cons_kernel, launched while
// the context holds constraints); see cbic_score_layer.inc.
template <int LMAX, int PHASE>
#if ULG_CONS
__global__ void __launch_bounds__(kBlock) score_wide_cons_kernel(WideArgs a, const uint64_t *cons, int cons_words) {
#else
__global__ void __launch_bounds__(kBlock) score_wide_kernel(WideArgs a) {
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *g = reinterpret_cast<double *>(smem);
#if ULG_CONS
    const uint64_t *ct = cons_stage<kBlock>(smem, a.n * a.n * 8, cons, cons_words);
#endif
    for (int i = threadIdx.x; i < a.n * a.n; i += kBlock) g[i] = a.gram[i];
    __syncthreads();
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= a.work[a.nv]) return;
    int lo = 0, hi = a.nv;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.work[mid] <= gid) lo = mid; else hi = mid;
    }
    const int vi = lo;
    const int v = a.meta[vi * 4 + 0];
    const int m = a.meta[vi * 4 + 1];
    const bool z = a.meta[vi * 4 + 2] != 0;
    const int L = a.L;
    const uint64_t r = gid - a.work[vi];
    uint64_t cm;
    if (PHASE == 0) cm = (unrank_colex64(r, L - 1, m - 1, a.binom) << 1) | 1ull;
    else if (z) cm = unrank_colex64(r, L, m - 1, a.binom) << 1;
    else cm = unrank_colex64(r, L, m, a.binom);
    const uint64_t slot = a.tbl_off[(uint64_t)vi * a.S + L] + rank_colex64(cm, a.binom);
#if ULG_CONS
    // a violator is stored at -float(n) before any regression: the value its
    // ts = float(n) takes on the ts >= 0 exit below
    if (cons_violates(ct, a.nv, vi, cm)) {
        a.table[slot] = -(float)a.n;
        return;
    }
#endif

    int gv[LMAX];
    {
        uint64_t rem = cm;
        for (int i = 0; i < L; ++i) {
            gv[i] = a.cand[vi * 64 + __builtin_ctzll(rem)];
            rem &= rem - 1;
        }
    }
    // Cholesky of G[P,P] (packed rows, row i at i(i+1)/2), y = L^-1 G[P,v]:
    // the unrolled kernels' operation order
    double Lm[LMAX * (LMAX + 1) / 2];
    double y[LMAX];
    const int n = a.n;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j <= i; ++j) Lm[i * (i + 1) / 2 + j] = g[gv[i] * n + gv[j]];
        y[i] = g[gv[i] * n + v];
    }
    const double cvv = g[v * n + v];
    const double piv = pivot_threshold(a.N, L);
    for (int j = 0; j < L; ++j) {
        const int rj = j * (j + 1) / 2;
        double s = Lm[rj + j];
        for (int k = 0; k < j; ++k) s -= Lm[rj + k] * Lm[rj + k];
        s = s <= piv ? (double)INFINITY : s;
        const double d = sqrt(s);
        Lm[rj + j] = d;
        const double inv = 1.0 / d;
        for (int i = j + 1; i < L; ++i) {
            const int ri = i * (i + 1) / 2;
            double t = Lm[ri + j];
            for (int k = 0; k < j; ++k) t -= Lm[ri + k] * Lm[rj + k];
            Lm[ri + j] = t * inv;
        }
    }
    double yy = 0.0;
    for (int i = 0; i < L; ++i) {
        const int ri = i * (i + 1) / 2;
        double t = y[i];
        for (int k = 0; k < i; ++k) t -= Lm[ri + k] * y[k];
        t = t / Lm[ri + i];
        y[i] = t;
        yy += t * t;
    }
    const double rss = clamp_rss(cvv - yy);
    // BIC_OLS.cpp:366
    const double the_score = a.N * log(rss / a.N) + a.pen * (double)L - 0.0;
    const float ts = (float)the_score;
    if (ts >= 0.0f) {
        const float s = -ts;  // stored by the caller iff < 0 (score_calculator.cpp:111)
        a.table[slot] = (s < 0.0f) ? s : absent_f();
        return;
    }
    const float thr = -ts;
    const uint64_t coff = a.tbl_off[(uint64_t)vi * a.S + L - 1];
    bool dom = false;
    {
        uint64_t rem = cm;
        while (rem) {
            const uint64_t bit = rem & (0 - rem);
            rem ^= bit;
            dom |= a.table[coff + rank_colex64(cm ^ bit, a.binom)] >= thr;  // absent (NaN) never >= thr
        }
    }
    if (dom) {
        a.table[slot] = absent_f();
        return;
    }
    const unsigned long long act = __ballot(1);
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)act) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(a.qcount, (unsigned long long)__popcll(act));
    base = __shfl(base, leader);
    const uint64_t pos = base + (uint64_t)__popcll(act & ((1ull << lane) - 1ull));
    uint64_t *e = a.queue + 3 * pos;
    e[0] = slot;
    e[1] = cm;
    e[2] = (uint64_t)(uint32_t)vi | ((uint64_t)fbits(ts) << 32);
}
