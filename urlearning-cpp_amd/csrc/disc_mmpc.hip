// disc_mmpc.hip -- the skeleton producer for discrete data (ulg_disc_mmpc,
// `mmpc --discrete`): Max-Min Parents and Children with G^2 tests on the value
// codes ulg_disc_load holds, and the tests themselves (ulg_disc_g2).
//
// PARITY UNPINNED: the reference has no MMPC (it expects the skeleton file
// from outside, README.md:16).  These rules are the definition; the tests
// restate them in Python (tests/test_disc_mmpc.py).  Round structure,
// tie-breaks and the AND rule are those of oracle/ora_mmpc.c with the
// association below in place of |Fisher z|.
//
// Test (X, T | S).  S ascending, q = prod_{s in S} r_s, cells = q r_X r_T.
//   G^2 = 2 [sum n_xtz ln n_xtz + sum n_z ln n_z - sum n_xz ln n_xz - sum n_tz ln n_tz],
//   empty cells contribute nothing, the result is clamped at 0;
//   dof = (r_X - 1)(r_T - 1) q.
// Reliability (the heuristic power rule).  A test is performed iff
//   N >= h cells and cells <= 32768, h = min_per_cell (default 5).  A test not
//   performed contributes nothing to any minimum.  If the marginal test
//   (S = {}) is not performed the pair's association is 0: never a candidate.
//   dof = 0 (a constant column) gives association 0.
// Association.  a = -ln p, p the chi-square survival function of G^2 with dof
//   degrees of freedom, computed in log space (chi2.h).  X and T are
//   independent given S iff a <= -ln alpha.
// Rounds, for every target T.
//   Forward: assoc[X] = a(X, T | {}); loop { drop every X with assoc <=
//   -ln alpha; F = argmax assoc over the rest (lowest index on ties), stop if
//   none; append F to CPC; assoc[X] = min(assoc[X], a(X, T | S)) over the
//   performed new subsets S of CPC (those containing F, |S| <= max_cond) }.
//   Backward: for X in CPC in insertion order, remove X if some performed S of
//   the current CPC minus X (|S| <= max_cond, the empty set included) gives
//   a <= -ln alpha.
//   Skeleton: X - T iff X in PC(T) and T in PC(X) (the AND rule).
//   max_cond < 0 or > 24 means 24; a CPC larger than 24 is ULG_ERR_UNSUPPORTED.
// Enumeration.  cells only grows with S, so the subsets of one (X, T) query
//   are enumerated by size and the enumeration stops after the first size with
//   no performable subset.  Every enumerated subset counts as a test when it
//   is performed and as skipped when it is not ("disc_mmpc_tests",
//   "disc_mmpc_skipped"); the n (n - 1) ordered marginal tests count too.  The
//   backward phase evaluates every performable subset (a removal needs only
//   one independent S, so the decision is that of stopping at the first).
//
// Kernel.  The host builds the list of performable tests of all targets for a
// round and launches once: one workgroup per test, grid-stride.  A workgroup
// zeroes an int32 LDS histogram of `cells` entries (at most 128 KB, the
// dynamic LDS sized to the batch's largest table), streams the N records with
// coalesced reads of the |S| + 2 code columns and one LDS atomic per record,
// then sums out T, X and both for the three marginals and adds the
// +-fix(n ln n) terms (disc_dev.h) into an int64.  The terms are a function of
// the counts alone and integer adds commute, so a test's sum does not depend
// on the launch, its place in the batch or the scheduling; the host scales it
// by 2 * 2^-shift and turns (G^2, dof) into -ln p in FP64.
//
// Block size: 256 threads, as the scorer's counting kernels.  The record loop
// is bound by the LDS atomics' issue rate and the column reads, not by
// registers; a table of more than 80 KB leaves one workgroup per CU, so the
// four waves of the workgroup are what hides the read latency there, and the
// small tables of the early rounds still fit eight workgroups per CU.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "chi2.h"
#include "disc_dev.h"
#include "ulg_internal.h"

using namespace ulg;

namespace {

constexpr int kG2Block = 256;
constexpr int kG2MaxCells = 32768;  // 128 KB of int32 in LDS
constexpr int kG2MaxCols = 15;      // 2^15 = kG2MaxCells: conditioning columns of arity >= 2
constexpr int kMaxPool = 24;        // CPC and conditioning-set cap (as ulg_mmpc's)

struct G2Test {
    int x, t;
    uint64_t cond;
};

// The decoded test (thread 0): columns of arity 1 hold code 0 only and are left out.
struct G2Item {
    int x, t, rx, rt, k;
    int q;
    int col[kG2MaxCols];
    int base[kG2MaxCols];
};

__global__ void __launch_bounds__(kG2Block)
disc_g2_kernel(DiscData D, const G2Test *tests, int64_t count, int max_cells, long long *out) {
    extern __shared__ __attribute__((aligned(16))) int hist[];
    __shared__ G2Item it;
    __shared__ unsigned long long acc;
    const int tid = threadIdx.x;
    for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
        __syncthreads();  // the previous test's LDS is done with
        if (tid == 0) {
            const G2Test g = tests[w];
            it.x = g.x;
            it.t = g.t;
            it.rx = D.arity[g.x];
            it.rt = D.arity[g.t];
            int k = 0;
            int64_t q = 1;
            for (uint64_t m = g.cond; m; m &= m - 1) {
                const int p = __builtin_ctzll(m);
                const int r = D.arity[p];
                if (r < 2) continue;
                if (k < kG2MaxCols) {
                    it.col[k] = p;
                    it.base[k] = (int)q;
                    ++k;
                }
                q = std::min<int64_t>(q * r, (int64_t)kG2MaxCells + 1);
            }
            // the host sends only tables that fit; anything else counts nothing
            if (q * it.rx * it.rt > (int64_t)max_cells) q = 0;
            it.k = k;
            it.q = (int)q;
            acc = 0ull;
        }
        __syncthreads();
        const int q = it.q, rx = it.rx, rt = it.rt;
        const int cells = q * rx * rt;
        if (cells == 0) {
            if (tid == 0) out[w] = 0;
            continue;
        }
        for (int i = tid; i < cells; i += kG2Block) hist[i] = 0;
        __syncthreads();
        // cell = z + q (code_x + r_x code_t): every code is below its arity (checked at load)
        const uint8_t *cx = D.codes + (int64_t)it.x * D.N, *ct = D.codes + (int64_t)it.t * D.N;
        const int k = it.k;
        for (int64_t r = tid; r < D.N; r += kG2Block) {
            int z = 0;
            for (int a = 0; a < k; ++a) z += (int)D.codes[(int64_t)it.col[a] * D.N + r] * it.base[a];
            atomicAdd(&hist[z + q * ((int)cx[r] + rx * (int)ct[r])], 1);
        }
        __syncthreads();
        long long a = 0;
        const int qx = q * rx;
        // + n_xtz ln n_xtz, - n_xz ln n_xz: one (z, x) per thread, T summed out
        for (int i = tid; i < qx; i += kG2Block) {
            unsigned int nxz = 0;
            for (int b = 0; b < rt; ++b) {
                const unsigned int c = (unsigned int)hist[i + qx * b];
                nxz += c;
                a += fix_nlogn(c, D.shift);
            }
            a -= fix_nlogn(nxz, D.shift);
        }
        // - n_tz ln n_tz: one (z, t) per thread, X summed out
        for (int i = tid; i < q * rt; i += kG2Block) {
            const int z = i % q, b = i / q;
            unsigned int ntz = 0;
            for (int e = 0; e < rx; ++e) ntz += (unsigned int)hist[z + q * (e + rx * b)];
            a -= fix_nlogn(ntz, D.shift);
        }
        // + n_z ln n_z: both summed out
        for (int z = tid; z < q; z += kG2Block) {
            unsigned int nz = 0;
            for (int e = 0; e < rx * rt; ++e) nz += (unsigned int)hist[z + q * e];
            a += fix_nlogn(nz, D.shift);
        }
        if (a) atomicAdd(&acc, (unsigned long long)a);
        __syncthreads();
        if (tid == 0) out[w] = (long long)acc;
    }
}

// cells and dof of (x, t | cond), saturating at INT64_MAX
void table_shape(const ulg_ctx *c, int x, int t, uint64_t cond, int64_t &cells, int64_t &dof) {
    constexpr int64_t kSat = std::numeric_limits<int64_t>::max();
    unsigned __int128 q = 1;
    bool sat = false;
    for (uint64_t m = cond; m; m &= m - 1) {
        q *= (unsigned)c->disc_arity[__builtin_ctzll(m)];
        if (q >> 63) sat = true, q = 1;
    }
    const unsigned rx = (unsigned)c->disc_arity[x], rt = (unsigned)c->disc_arity[t];
    const unsigned __int128 cl = q * rx * rt, df = q * (rx - 1) * (rt - 1);
    cells = sat || (cl >> 63) ? kSat : (int64_t)cl;
    dof = (rx == 1 || rt == 1) ? 0 : (sat || (df >> 63) ? kSat : (int64_t)df);
}

// One launch: the fixed-point sums of `tests` (tables of at most max_cells <= kG2MaxCells cells).
int run_tests(ulg_ctx *c, const std::vector<G2Test> &tests, int64_t max_cells, std::vector<long long> &sums) {
    sums.assign(tests.size(), 0);
    if (tests.empty()) return ULG_OK;
    ULG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->d_g2_tests, tests.size() * 2)) || (rc = ensure(c, c->d_g2_out, tests.size()))) return rc;
    const size_t lds = (size_t)std::max<int64_t>(std::min<int64_t>(max_cells, kG2MaxCells), 4) * sizeof(int);
    ULG_HIP(c, hipFuncSetAttribute((const void *)disc_g2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ULG_HIP(c, hipMemcpyAsync(c->d_g2_tests.p, tests.data(), tests.size() * sizeof(G2Test), hipMemcpyHostToDevice,
                              c->stream));
    const unsigned grid = (unsigned)std::min<size_t>(tests.size(), 2048);
    prof_begin(c, "disc_g2");
    disc_g2_kernel<<<grid, kG2Block, lds, c->stream>>>(disc_data(c), reinterpret_cast<const G2Test *>(c->d_g2_tests.p),
                                                      (int64_t)tests.size(), (int)(lds / sizeof(int)),
                                                      reinterpret_cast<long long *>(c->d_g2_out.p));
    prof_end(c);
    ULG_HIP(c, hipGetLastError());
    ULG_HIP(c, hipMemcpyAsync(sums.data(), c->d_g2_out.p, tests.size() * sizeof(long long), hipMemcpyDeviceToHost,
                              c->stream));
    ULG_HIP(c, hipStreamSynchronize(c->stream));  // `tests` is a pageable source
    prof_collect(c);
    return ULG_OK;
}

inline double g2_of(long long sum, int shift) { return std::max(0.0, 2.0 * std::ldexp((double)sum, -shift)); }

// ---- MMPC --------------------------------------------------------------------
struct Rounds {
    ulg_ctx *c;
    int64_t h;          // min_per_cell
    int max_cond;
    std::vector<G2Test> tests;
    std::vector<int> owner;    // per test: its query
    std::vector<int64_t> dofs;
    int64_t max_cells = 0, performed = 0, skipped = 0;
    int queries = 0;

    void clear() {
        tests.clear();
        owner.clear();
        dofs.clear();
        max_cells = 0;
        queries = 0;
    }
    // One query: the subsets of `pool` (those containing `must` if must >= 0) by size, up to the first size
    // with no performable subset.  Returns the query's index.
    int add_query(int T, int X, int must, const std::vector<int> &pool) {
        std::vector<int> others;
        for (int v : pool)
            if (v != must) others.push_back(v);
        const int no = (int)others.size(), need = must >= 0 ? 1 : 0;
        const uint64_t fixed = must >= 0 ? 1ull << must : 0ull;
        const int qi = queries++;
        std::vector<int> idx;
        for (int s = 0; s + need <= max_cond && s <= no; ++s) {
            int done = 0;
            idx.resize(s);
            for (int i = 0; i < s; ++i) idx[i] = i;
            for (;;) {
                uint64_t mask = fixed;
                for (int i = 0; i < s; ++i) mask |= 1ull << others[idx[i]];
                int64_t cells, dof;
                table_shape(c, X, T, mask, cells, dof);
                if (cells <= kG2MaxCells && c->N >= h * cells) {
                    tests.push_back(G2Test{X, T, mask});
                    owner.push_back(qi);
                    dofs.push_back(dof);
                    max_cells = std::max(max_cells, cells);
                    ++done;
                } else {
                    ++skipped;
                }
                // next combination of s out of no
                int i = s - 1;
                while (i >= 0 && idx[i] == no - s + i) --i;
                if (i < 0) break;
                ++idx[i];
                for (int j = i + 1; j < s; ++j) idx[j] = idx[j - 1] + 1;
            }
            performed += done;
            if (!done) break;
        }
        return qi;
    }
    // The launch; best[q] = the smallest association over query q's performed tests (+inf if none).
    int run(std::vector<double> &best) {
        std::vector<long long> sums;
        if (int rc = run_tests(c, tests, max_cells, sums)) return rc;
        best.assign((size_t)queries, INFINITY);
        const int shift = disc_data(c).shift;
        for (size_t i = 0; i < tests.size(); ++i) {
            const double a = dofs[i] == 0 ? 0.0 : -chi2_log_sf(g2_of(sums[i], shift), (double)dofs[i]);
            best[owner[i]] = std::min(best[owner[i]], a);
        }
        return ULG_OK;
    }
};

}  // namespace

extern "C" {

double ulg_chi2_log_sf(double x, double dof) { return chi2_log_sf(x, dof); }

int ulg_disc_g2(ulg_ctx *c, int64_t count, const int *xs, const int *ts, const uint64_t *conds, double *g2,
                int64_t *dof, int64_t *cells) {
    if (!c || count < 0 || (count > 0 && (!xs || !ts || !conds || !g2 || !dof || !cells))) return ULG_ERR_ARG;
    if (int rc0 = finish_pending(c)) return rc0;
    if (!disc_ready(c)) return set_err(c, ULG_ERR_STATE, "ulg_disc_g2: call ulg_disc_load first");
    const int n = c->n;
    std::vector<G2Test> tests;
    std::vector<int64_t> at;
    int64_t max_cells = 0;
    for (int64_t i = 0; i < count; ++i) {
        if (xs[i] < 0 || xs[i] >= n || ts[i] < 0 || ts[i] >= n || (conds[i] >> n))
            return set_err(c, ULG_ERR_ARG, "ulg_disc_g2: variable out of range");
        if (xs[i] == ts[i] || ((conds[i] >> xs[i]) & 1ull) || ((conds[i] >> ts[i]) & 1ull))
            return set_err(c, ULG_ERR_ARG, "ulg_disc_g2: x, t and the conditioning set must be distinct");
    }
    for (int64_t i = 0; i < count; ++i) {
        table_shape(c, xs[i], ts[i], conds[i], cells[i], dof[i]);
        if (cells[i] > kG2MaxCells) {
            g2[i] = NAN;
            continue;
        }
        tests.push_back(G2Test{xs[i], ts[i], conds[i]});
        at.push_back(i);
        max_cells = std::max(max_cells, cells[i]);
    }
    std::vector<long long> sums;
    if (int rc = run_tests(c, tests, max_cells, sums)) return rc;
    const int shift = disc_data(c).shift;
    for (size_t k = 0; k < tests.size(); ++k) g2[at[k]] = g2_of(sums[k], shift);
    return ULG_OK;
}

int ulg_disc_mmpc(ulg_ctx *c, double alpha, int max_cond, int min_per_cell, uint64_t *rows) {
    if (!c) return ULG_ERR_ARG;
    if (!rows || !(alpha > 0.0 && alpha < 1.0) || min_per_cell < 1)
        return set_err(c, ULG_ERR_ARG, "ulg_disc_mmpc: alpha must be in (0, 1) and min_per_cell >= 1");
    if (int rc0 = finish_pending(c)) return rc0;
    if (!disc_ready(c)) return set_err(c, ULG_ERR_STATE, "ulg_disc_mmpc: call ulg_disc_load first");
    const int n = c->n;
    if (max_cond < 0 || max_cond > kMaxPool) max_cond = kMaxPool;
    const double crit = -std::log(alpha);
    Rounds R{c, (int64_t)min_per_cell, max_cond};
    std::vector<std::vector<double>> assoc(n, std::vector<double>(n, 0.0));
    std::vector<std::vector<char>> alive(n, std::vector<char>(n, 0));
    std::vector<std::vector<int>> cpc(n), qid(n, std::vector<int>(n, -1));
    std::vector<char> active(n, 1);
    std::vector<double> best;
    int rc;
    // a(X, T | {}) for every pair; a pair whose marginal test is not performed keeps association 0
    for (int T = 0; T < n; ++T)
        for (int X = 0; X < n; ++X)
            if (X != T) {
                alive[T][X] = 1;
                qid[T][X] = R.add_query(T, X, -1, {});
            }
    if ((rc = R.run(best))) return rc;
    for (int T = 0; T < n; ++T)
        for (int X = 0; X < n; ++X)
            if (X != T) assoc[T][X] = std::isinf(best[qid[T][X]]) ? 0.0 : best[qid[T][X]];
    // forward: all targets advance one member per round
    for (;;) {
        R.clear();
        bool any = false;
        for (int T = 0; T < n; ++T) {
            if (!active[T]) continue;
            int F = -1;
            for (int X = 0; X < n; ++X) {
                if (!alive[T][X]) continue;
                if (assoc[T][X] <= crit) { alive[T][X] = 0; continue; }
                if (F < 0 || assoc[T][X] > assoc[T][F]) F = X;
            }
            if (F < 0) { active[T] = 0; continue; }
            if ((int)cpc[T].size() >= kMaxPool)
                return set_err(c, ULG_ERR_UNSUPPORTED, "ulg_disc_mmpc: more than 24 candidates");
            any = true;
            alive[T][F] = 0;
            cpc[T].push_back(F);
            for (int X = 0; X < n; ++X) qid[T][X] = alive[T][X] ? R.add_query(T, X, F, cpc[T]) : -1;
        }
        if (!any) break;
        if ((rc = R.run(best))) return rc;
        for (int T = 0; T < n; ++T)
            for (int X = 0; X < n; ++X)
                if (active[T] && alive[T][X] && qid[T][X] >= 0) assoc[T][X] = std::min(assoc[T][X], best[qid[T][X]]);
    }
    // backward: position by position (a removal changes the later pools)
    std::vector<std::vector<char>> keep(n);
    size_t longest = 0;
    for (int T = 0; T < n; ++T) {
        keep[T].assign(cpc[T].size(), 1);
        longest = std::max(longest, cpc[T].size());
    }
    for (size_t i = 0; i < longest; ++i) {
        R.clear();
        std::vector<int> owner;
        for (int T = 0; T < n; ++T) {
            if (i >= cpc[T].size()) continue;
            std::vector<int> rest;
            for (size_t j = 0; j < cpc[T].size(); ++j)
                if (j != i && keep[T][j]) rest.push_back(cpc[T][j]);
            R.add_query(T, cpc[T][i], -1, rest);
            owner.push_back(T);
        }
        if ((rc = R.run(best))) return rc;
        for (size_t k = 0; k < owner.size(); ++k)
            if (best[k] <= crit) keep[owner[k]][i] = 0;
    }
    std::vector<uint64_t> pc(n, 0);
    for (int T = 0; T < n; ++T)
        for (size_t j = 0; j < cpc[T].size(); ++j)
            if (keep[T][j]) pc[T] |= 1ull << cpc[T][j];
    for (int T = 0; T < n; ++T) {
        rows[T] = 0;
        for (int X = 0; X < n; ++X)
            if (((pc[T] >> X) & 1ull) && ((pc[X] >> T) & 1ull)) rows[T] |= 1ull << X;
    }
    c->disc_mmpc_stat[0] = R.performed;
    c->disc_mmpc_stat[1] = R.skipped;
    return ULG_OK;
}

}  // extern "C"
