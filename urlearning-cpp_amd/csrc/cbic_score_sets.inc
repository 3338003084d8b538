// cbic_score_sets.inc -- included by cbic.hip once per form: ULG_CONS 0 is the kernel as it
// is without constraints, 1 its constrained twin (*_cons_kernel, launched while
// the context holds constraints); see cbic_score_layer.inc.
#if ULG_CONS
// cons: the by-variable table in variable masks; a violator, the empty set
// included, returns -float(n)
__global__ void __launch_bounds__(kBlock) score_sets_cons_kernel(const double *gram, const uint64_t *pairs,
                                                                 int64_t count, int n, double N, double pen,
                                                                 float *out, const uint64_t *cons) {
#else
__global__ void __launch_bounds__(kBlock) score_sets_kernel(const double *gram, const uint64_t *pairs, int64_t count,
                                                            int n, double N, double pen, float *out) {
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *g = reinterpret_cast<double *>(smem);
    for (int i = threadIdx.x; i < n * n; i += kBlock) g[i] = gram[i];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int v = (int)pairs[2 * i];
    const uint64_t P = pairs[2 * i + 1] & ~(1ull << v);
#if ULG_CONS
    if (cons_violates(cons, n, v, P)) {
        out[i] = -(float)n;
        return;
    }
#endif
    const int L = __builtin_popcountll(P);
    if (L == 0) {
        out[i] = -0.0f;
        return;
    }
    int gv[kWideMax];
    {
        uint64_t rem = P;
        for (int j = 0; j < L; ++j) {
            gv[j] = __builtin_ctzll(rem);
            rem &= rem - 1;
        }
    }
    double Lm[kWideMax * (kWideMax + 1) / 2];
    double y[kWideMax];
    for (int r = 0; r < L; ++r) {
        for (int j = 0; j <= r; ++j) Lm[r * (r + 1) / 2 + j] = g[gv[r] * n + gv[j]];
        y[r] = g[gv[r] * n + v];
    }
    const double cvv = g[v * n + v];
    const double piv = pivot_threshold(N, L);
    for (int j = 0; j < L; ++j) {
        const int rj = j * (j + 1) / 2;
        double s = Lm[rj + j];
        for (int k = 0; k < j; ++k) s -= Lm[rj + k] * Lm[rj + k];
        s = s <= piv ? (double)INFINITY : s;
        const double d = sqrt(s);
        Lm[rj + j] = d;
        const double inv = 1.0 / d;
        for (int r = j + 1; r < L; ++r) {
            const int rr = r * (r + 1) / 2;
            double t = Lm[rr + j];
            for (int k = 0; k < j; ++k) t -= Lm[rr + k] * Lm[rj + k];
            Lm[rr + j] = t * inv;
        }
    }
    double yy = 0.0;
    for (int r = 0; r < L; ++r) {
        const int rr = r * (r + 1) / 2;
        double t = y[r];
        for (int k = 0; k < r; ++k) t -= Lm[rr + k] * y[k];
        t = t / Lm[rr + r];
        y[r] = t;
        yy += t * t;
    }
    const double rss = clamp_rss(cvv - yy);
    const double the_score = N * log(rss / N) + pen * (double)L - 0.0;  // BIC_OLS.cpp:366, pen = lambda ln(N)
    out[i] = -(float)the_score;
}
