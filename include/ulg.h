/*
 * ulg.h -- C ABI of the MI355X-native URLearning hot path (libulg.so).
 *
 * Drop-in boundary for the reference's plugin points on the
 * cBIC-score + order-graph-search path (ninalu/urlearning-cpp, paths
 * relative to urlearning/):
 *
 *   ulg_cbic_load        replaces BIC_OLS_Function::BIC_OLS_Function
 *                        (scoring_function/BIC_OLS.cpp:30-123): data load,
 *                        centring/scaling, Gram matrix (the reference's
 *                        printed corr_mat = Z'Z/N, :105).
 *   ulg_cbic_score       replaces ScoreCalculator::calculateScores
 *                        (scoring_function/score_calculator.h:35,
 *                        score_calculator.cpp:33-135) driving
 *                        ScoringFunction::calculateScore (scoring_function.h:16-23,
 *                        BIC_OLS.cpp:174-389) for a batch of variables; the
 *                        stored-set rule and the find_best_subset_score
 *                        dominance recursion are reproduced exactly.
 *   ulg_cbic_set_constraints  replaces the scoring::Constraints* argument
 *                        of the scoring function's constructor
 *                        (scoring_function/constraints.h:36-139, wired in at
 *                        score/score_main.cpp:314-317,351): a violating parent
 *                        set takes the raw score variableCount before any
 *                        regression (BIC_OLS.cpp:279-283).
 *   ulg_cbic_fetch       hands the stored FloatMap contents back (what
 *                        scoringThread prints, score/score_main.cpp:173-203).
 *   ulg_disc_load        replaces the RecordFile / BayesianNetwork / ADTree
 *                        state score_main builds for the discrete scores
 *                        (score/score_main.cpp:283-292): the value codes of
 *                        every record and each variable's cardinality.
 *   ulg_disc_score       replaces ScoreCalculator::calculateScores
 *                        (score_calculator.cpp:33-135) driving
 *                        BICScoringFunction::calculateScore
 *                        (scoring_function/bic_scoring_function.cpp:20-76) and
 *                        LogLikelihoodCalculator::calculate
 *                        (log_likelihood_calculator.cpp:17-77): the AD-tree's
 *                        count queries (ad_tree/ad_tree.cpp:95-164) become one
 *                        contingency-count pass over the records per set.
 *   ulg_disc_score_sets  the per-call BICScoringFunction::calculateScore value.
 *   ulg_bestscore_*      replaces bestscorecalculators::BestScoreCalculator
 *                        (score_cache/best_score_calculator.h:16-26) with the
 *                        list calculator's semantics
 *                        (score_cache/sparse_parent_list.cpp:20-55).
 *   ulg_pdb_*            replaces heuristics::StaticPatternDatabase
 *                        (heuristic/static_pattern_database.cpp:82-247).
 *   ulg_astar            replaces run_astar_on_one_scc
 *                        (astar/astar_main.cpp:216-546).
 *   ulg_triplet_astar    replaces triplet_astar's astar() driver and its
 *                        re-opening run_astar_on_one_scc
 *                        (astar/triplet_astar.cpp:285-674,811-1622).
 *
 * Conventions (mirroring the reference's): the caller owns host buffers;
 * device memory is owned by the context; hot calls report errors by an int
 * status (0 = ok) and ulg_last_error(); one context per host thread and per
 * GPU (one process per GPU for multi-GPU runs).  varsets are uint64 bit
 * masks (bit i = variable i), as in typedefs.h:647-755.  Scores are the
 * .pss "score" (higher is better); costs are A* costs (= -score after the
 * .pss "%f" round trip, score_cache.cpp:151).
 */
#ifndef ULG_H
#define ULG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ulg_ctx ulg_ctx;

#define ULG_OK 0
#define ULG_ERR_ARG 1
#define ULG_ERR_HIP 2
#define ULG_ERR_STATE 3
#define ULG_ERR_UNSUPPORTED 4

/* Largest parent-set size the HIP scorer handles.  Layers up to
 * ULG_UNROLLED_PARENTS_GPU run fully unrolled kernels (register Cholesky,
 * bitset dominance walk); larger layers (the reference's default -p = n-1 on
 * small n, e.g. data/hepatitis.clean.csv) run the wide-layer kernels, whose
 * find_best_subset_score walk keeps a 2^(k+1)-bit checked set per set. */
#define ULG_MAX_PARENTS_GPU 31
#define ULG_UNROLLED_PARENTS_GPU 8
/* Most alternatives ulg_cbic_set_constraints takes for one variable. */
#define ULG_MAX_CONSTRAINT_ALTERNATIVES 64

/* ---- context --------------------------------------------------------- */
/* One device per context: ndev must be 1 (multi-GPU = one process per GPU). */
int ulg_create(const int *device_ids, int ndev, ulg_ctx **out);
void ulg_destroy(ulg_ctx *ctx);
const char *ulg_last_error(const ulg_ctx *ctx);
/* Library build identifier ("gfx950 ..."). */
const char *ulg_version(void);

/* ---- cBIC scoring (BIC_OLS.cpp, score_calculator.cpp) ----------------- */
/* data_colmajor: N x n doubles, column-major (column j = variable j), as
 * Armadillo holds raw_data.  n <= 63.  Normalises each column to zero mean
 * and unit sample variance (N-1) and builds the FP64 Gram matrix Z'Z on the
 * device (MFMA f64).  A pending ulg_cbic_score_async call is collected
 * first (its launches read the Gram matrix this call replaces). */
int ulg_cbic_load(ulg_ctx *ctx, const double *data_colmajor, int64_t N, int n,
                  double lambda);
/* Copy the device Gram matrix Z'Z (n x n, row-major) to host. */
int ulg_cbic_gram(ulg_ctx *ctx, double *gram_out);

/* The skeleton the reference expects from outside (README.md:16, read by
 * Skeleton::read_matrix_file, base/skeleton.cpp:19-105): MMPC with Fisher-z
 * partial-correlation tests on the loaded data's Gram matrix.  Independent
 * iff |atanh(r)| sqrt(N - |S| - 3) <= Phi^-1(1 - alpha/2); conditioning sets
 * of at most max_cond variables (< 0: 24); AND symmetry rule.  rows[i] bit j
 * = edge i-j (no diagonal).  A constant column (every test on it is NaN) has
 * no edge.  Exact rules: oracle/ora_mmpc.c. */
int ulg_mmpc(ulg_ctx *ctx, double alpha, int max_cond, uint64_t *rows);
/* The raw statistics behind ulg_mmpc, for count queries on the loaded data's
 * Gram matrix (tests and diagnostics; the continuous counterpart of
 * ulg_disc_g2): out[i] = the minimum of |z(xs[i], ts[i] | S)| =
 * |atanh(r)| sqrt(N - |S| - 3) over the subsets S of pools[i] (a variable
 * mask) with |S| <= max_cond (< 0 or > 24: 24) that contain musts[i]
 * (musts[i] < 0: every subset; its bit may be set in pools[i] or not).
 * Subsets are taken as subset masks ascending over the pool without must in
 * ascending variable order, the empty (or {must}) set first, and the
 * enumeration stops at the first value <= stops[i] (-inf: never; +inf: the
 * first set's value is the result).  No set of at most max_cond variables
 * (max_cond = 0 with a must) gives +inf; N - |S| - 3 <= 0 or a residual
 * variance <= 0 gives 0; r is clamped to +-(1 - 1e-15); a set whose
 * value is NaN (a constant column) never replaces the minimum, so a query
 * with nothing else gives +inf.  Each query is one lane of
 * ulg_mmpc's own query launch (mmpc_query_kernel, the instance chosen by the
 * largest conditioning set of the call as there).  ULG_ERR_ARG for x = t, for
 * x or t equal to must or in the pool, for an index or a mask bit out of
 * range and for more than 24 conditioning variables (pool and must);
 * ULG_ERR_STATE without continuous data.  The context's lists stay as they
 * are. */
int ulg_mmpc_min_z(ulg_ctx *ctx, int64_t count, const int *ts, const int *xs, const int *musts,
                   const uint64_t *pools, int max_cond, const double *stops, double *out);

/* Score all parent sets of size <= max_parents within each variable's
 * candidate set (candidates[i] for variable vars[i]; the variable's own bit
 * is ignored).  max_parents < 1 or > n - 1 means n - 1, the reference's
 * "a value less than 1 means no limit" (score_main.cpp:228,296-298).  Runs the layer-synchronous HIP scorer; results stay on the
 * device until ulg_cbic_fetch.  *total_stored = number of stored sets,
 * *total_scored = number of parent sets evaluated (incl. empty sets). */
int ulg_cbic_score(ulg_ctx *ctx, const int *vars, int nv,
                   const uint64_t *candidates, int max_parents,
                   int64_t *total_stored, int64_t *total_scored);
/* The same call split in two, so one host thread can keep several contexts'
 * scoring in flight (e.g. two steps of a throughput loop on one GPU):
 * ulg_cbic_score_async queues the whole call and returns without waiting
 * (when every layer is unrolled and no time limit is set; otherwise it runs
 * synchronously), ulg_cbic_score_finish waits for it and returns the counts
 * ulg_cbic_score would have.  Any later scorer call on the context
 * (ulg_cbic_score*, ulg_cbic_fetch) finishes a pending one first. */
int ulg_cbic_score_async(ulg_ctx *ctx, const int *vars, int nv,
                         const uint64_t *candidates, int max_parents);
int ulg_cbic_score_finish(ulg_ctx *ctx, int64_t *total_stored, int64_t *total_scored);
/* Copy the stored sets out.  offsets[nv+1]; variable vars[i] owns
 * [offsets[i], offsets[i+1]); within a variable, sets are ordered by
 * (|set|, set value) -- the reference's Gosper insertion order.
 * device_ptrs = 1: sets/scores/offsets are device pointers (e.g. torch
 * tensors on this context's device); 0: host pointers.
 * Stream contract: the copies run on the context's own stream, and the call
 * is synchronous -- it returns after they are complete, with host or device
 * pointers alike, so the destination may be read on any stream afterwards.
 * The copies are NOT ordered after work another stream queued on the
 * destination (e.g. a torch zero fill on torch's current stream): the caller
 * must finish that work first, or record an event after it and pass it to
 * ulg_stream_wait_event before this call. */
int ulg_cbic_fetch(ulg_ctx *ctx, uint64_t *sets, float *scores,
                   int64_t *offsets, int device_ptrs);
/* The context's stream waits (on the device, no host sync) for a hipEvent_t
 * the caller recorded on another stream of the same device; every later
 * launch and copy of the context is ordered after it. */
int ulg_stream_wait_event(ulg_ctx *ctx, void *event);
/* Convenience: ulg_cbic_score + ulg_cbic_fetch to host buffers of
 * capacity cap entries; returns ULG_ERR_ARG if cap is too small. */
int ulg_cbic_score_vars(ulg_ctx *ctx, const int *vars, int nv,
                        const uint64_t *candidates, int max_parents,
                        uint64_t *sets, float *scores, int64_t *offsets,
                        int64_t cap);

/* scoring::Constraints (scoring_function/constraints.h:36-139) for the loaded data:
 * alternative i says variable vars[i] may take a parent set P with required[i] ⊆ P and
 * P ∩ forbidden[i] = ∅; a variable with at least one alternative must satisfy one of them.
 * count = 0 clears.  Valid after ulg_cbic_load or ulg_disc_load, cleared by the next load
 * of either kind; applies to ulg_cbic_score*, ulg_cbic_score_sets, ulg_disc_score* and
 * everything that reads their lists (for the discrete scores see ulg_disc_score).
 * A violating set scores variableCount (BIC_OLS.cpp:279-283), so it is stored
 * at -float(n) -- the empty set too, when every alternative of its variable
 * requires a parent -- and the dominance walks of larger sets see it as a
 * present key.  The reference's uninitialised Constraints::empty
 * (constraints.h:59) is taken as 0.  Masks with a bit >= n, a variable out
 * of range or a call before any load return ULG_ERR_ARG; more than
 * ULG_MAX_CONSTRAINT_ALTERNATIVES alternatives for one variable return
 * ULG_ERR_UNSUPPORTED.  ulg_get_info("constraints") is the number held. */
int ulg_cbic_set_constraints(ulg_ctx *ctx, int count, const int *vars,
                             const uint64_t *required, const uint64_t *forbidden);

/* Per-call counterpart of ScoringFunction::calculateScore(variable, parents,
 * cache) (scoring_function.h:16-23, BIC_OLS.cpp:174-276): for each pair
 * (vars[i], parents[i]) the value it returns, -float(the_score) with
 * the_score = N ln(RSS/N) + lambda ln(N) |P| (calculateScoreAndBeta,
 * BIC_OLS.cpp:277-388; no parents -> -0.0f), batched on the device from the
 * loaded Gram matrix with the layer scorer's Cholesky, so a stored set's value
 * equals what ulg_cbic_score stored for it.  The variable's own bit is
 * ignored (parent_vec skips it).  The cache insertion rule (store iff the
 * value is < 0 and no subset dominates) stays with ulg_cbic_score, which
 * applies it layer by layer.  At most 31 parents per set. */
int ulg_cbic_score_sets(ulg_ctx *ctx, int64_t count, const int *vars,
                        const uint64_t *parents, float *neg_scores);

/* ---- discrete scoring: BIC (bic_scoring_function.cpp, log_likelihood_calculator.cpp),
 *      BDeu (bdeu_scoring_function.cpp) and fNML (fnml_scoring_function.cpp) ---- */
#define ULG_SCORE_BIC 1
/* 2 is not a kind: it has always been refused with ULG_ERR_ARG and stays so. */
#define ULG_SCORE_BDEU 3
/* 0 and 4 are not kinds either. */
#define ULG_SCORE_FNML 5
/* codes_colmajor: N x n value codes, column-major (column j = variable j);
 * arity[j] = cardinality of variable j.  n <= 63, 1 <= arity <= 255,
 * 2 <= N < 2^31.  Every code must be below its column's arity; the upload
 * pass checks that on the device and the call returns ULG_ERR_ARG otherwise.
 * A context holds continuous or discrete data, whichever was loaded last:
 * ulg_cbic_score*, ulg_cbic_score_sets, ulg_cbic_gram and ulg_mmpc after
 * ulg_disc_load return ULG_ERR_STATE, and ulg_disc_* after ulg_cbic_load
 * likewise.  Either load clears ulg_cbic_set_constraints. */
int ulg_disc_load(ulg_ctx *ctx, const uint8_t *codes_colmajor, int64_t N, int n, const int *arity);
/* ulg_cbic_score's arguments and counts for a discrete score (kind =
 * ULG_SCORE_BIC, ULG_SCORE_BDEU or ULG_SCORE_FNML, see below; anything else is
 * ULG_ERR_ARG).
 * What follows is the BIC value.  max_parents is taken as
 * given (< 1 or > n - 1 means n - 1): the BIC limit log(2N / log N) is the
 * command line's job (score_main.cpp:300-304).  The value of (v, P) is
 *   sum_cells n_jk ln n_jk - sum_j n_j ln n_j - (r_v - 1) prod_{p in P} r_p ln(N) / 2
 * from the exact integer counts in FP64, rounded to float once; each
 * n ln n term is accumulated as a fixed-point integer, so the value does not
 * depend on scheduling or on the kernel path that counted.  The empty set is
 * stored iff its value is < 1, every other set iff its value is < 0
 * (score_calculator.cpp:62,116); there is no dominance test.  A variable of
 * arity 1 scores 0 for every set.  A set that violates
 * ulg_cbic_set_constraints scores 1 and is never stored
 * (bic_scoring_function.cpp:34-37).  The lists replace the context's
 * (ulg_cbic_fetch, ulg_pss_format, ulg_search_from_scores read them);
 * time_limit_ms is checked after each complete layer.  q r_v >= 2^63 cells
 * (q = prod r_p) returns ULG_ERR_UNSUPPORTED, as do sets of more than
 * ULG_MAX_PARENTS_GPU parents.  A refused call leaves the previous lists.
 *
 * Option "disc_prune" (ulg_set_option, 0 or 1, default 0, sticky; any other
 * value is ULG_ERR_ARG; only this call reads it): 1 applies the reference's
 * end-of-scoring prune() (score_calculator.cpp:137-197, whose call the
 * reference commented out in score_main.cpp:166-171 for the continuous case)
 * to every variable's list before it is stored.  On the float values above, a
 * set P is removed iff a kept proper subset Q has (float)(s(Q) - s(P)) >=
 * -2 FLT_EPSILON (2.3841858e-07f): Q scores at least as well, ties included.
 * Only stored sets dominate, but through any number of sets that are not
 * stored; a removed set removes nothing.  That is prune()'s sort-and-scan
 * wherever its comparator is a strict weak order (|score| >= 4).  One extra
 * launch per completed layer (disc_prune_kernel) and one float per table
 * slot; with 0 no kernel runs and nothing is allocated.  total_stored then
 * counts the kept sets, total_scored is unchanged and
 * ulg_get_info("disc_pruned") gives the sets removed (0 with the option off).
 * ulg_disc_score_sets, ulg_disc_counts and ulg_cbic_* ignore the option.
 *
 * kind = ULG_SCORE_BDEU: the Bayesian Dirichlet equivalent uniform score with
 * equivalent sample size ess (ulg_disc_set_ess).  With r = r_v, q = prod r_p,
 *   a_j = ess / q,  a_jk = ess / (q r)                                  (FP64)
 *   s(v, P) = sum over non-empty cells   [ lgamma(a_jk + n_jk) - lgamma(a_jk) ]
 *           + sum over non-empty configs [ lgamma(a_j) - lgamma(a_j + n_j) ]
 * Each bracketed term is computed in FP64 from the exact integer count and
 * rounded once to a fixed-point integer (scale 2^-shift, a function of N and
 * ess: csrc/disc_bdeu.h); the integer sum is converted back and rounded to
 * float once.  The value is therefore bit-identical on the dense and sparse
 * counting paths, across calls and for any grid.  Everything else is as for
 * BIC: the store rule (the empty set iff < 1, every other set iff < 0), 0 for
 * a variable of arity 1, 1 and never stored for a set that violates the
 * constraints, ULG_ERR_UNSUPPORTED from 2^63 cells or above
 * ULG_MAX_PARENTS_GPU parents, time_limit_ms, option "disc_prune" and every
 * ulg_get_info value.  BDeu has no parent limit of its own: the reference
 * applies log(2N / log N) to "bic" only (score_main.cpp:300-304).
 * Two departures from the reference: it keeps a_j, a_jk, their lgamma and the
 * running sum in float, and it computes q r in int, which overflows from 2^31
 * cells on; here a_j and a_jk are FP64 for every q r < 2^63 and the sum is
 * exact, as for BIC.  De Campos pruning (enableDeCamposPruning) is not built.
 * Replaces BDeuScoringFunction::lg, calculateScore and calculate
 * (bdeu_scoring_function.cpp:21-35, 69-79, 117-166).
 *
 * kind = ULG_SCORE_FNML: the factorized normalized maximum likelihood score,
 * which has no hyper-parameter.  With r = r_v,
 *   s(v, P) = sum_cells n_jk ln n_jk - sum_j n_j ln n_j
 *           - sum over non-empty configs ln C(r, n_j)
 * where C(r, n) is the normaliser (regret) of the multinomial NML distribution:
 *   C(2, n) = sum_{h=0..n} binom(n, h) (h/n)^h ((n-h)/n)^(n-h)   (1, 2, 2.5, 26/9, ...)
 * summed exactly for n <= 1000 (on the host, in long double, correct to an
 * FP64 ulp) and Szpankowski's three-term approximation
 *   exp(ln(n pi / 2) / 2 + sqrt(8 / (9 n pi)) + (1/12 - 4 / (9 pi)) / n)
 * above, which is the reference's threshold: the approximation lies 5.5e-7
 * above the exact sum at n = 1001, so a configuration's regret steps by that
 * much between n_j = 1000 and 1001.  C(k, n) = C(k-1, n) + n / (k-2) C(k-2, n)
 * runs in FP64 on the ratio C(k, n) / C(k-1, n) and in log space
 * (csrc/disc_fnml.h).  The regrets of the loaded columns' arities live in a
 * device table of fixed-point integers, built by the first fNML call after
 * ulg_disc_load (fnml_regret_kernel) and kept until the next load of either
 * kind: ulg_get_info("fnml_table_bytes") is its size, 0 while there is none.
 * (distinct arities >= 2) x (N + 1) > 2^28 entries returns
 * ULG_ERR_UNSUPPORTED.  Every term -- the n ln n terms and each regret -- is
 * rounded once to a fixed-point integer (scale 2^-shift, a function of N and
 * the largest arity), the integer sum is rounded to float once: bit-identical
 * on the dense and sparse counting paths, across calls and for any grid.
 * Everything else is as for BIC and BDeu: the store rule, 0 for a variable of
 * arity 1, 1 and never stored for a violating set, ULG_ERR_UNSUPPORTED from
 * 2^63 cells or above ULG_MAX_PARENTS_GPU parents, time_limit_ms, option
 * "disc_prune" and every ulg_get_info value; there is no BIC parent limit
 * (score_main.cpp:300-306 applies it to "bic" only).
 * Two departures from the reference: it runs the recurrence on float values
 * and sums the regrets in float, which turn infinite once C(r, n) passes
 * 3.4e38 (r = 60, n = 1000: ln C = 117.5) -- here FP64 and log space, finite
 * for every r <= 255 and N < 2^31; and below n = 1001 it reads 12-digit
 * literals rounded to float where this is the exact sum.
 * Replaces fNMLScoringFunction's calculateScore, calculate and regret
 * (fnml_scoring_function.cpp:17-74) and the table of
 * fnml_scoring_function.h:300-340. */
int ulg_disc_score(ulg_ctx *ctx, int kind, const int *vars, int nv, const uint64_t *candidates,
                   int max_parents, int64_t *total_stored, int64_t *total_scored);
/* The equivalent sample size of ULG_SCORE_BDEU: sticky, default 1.0, kept
 * across ulg_disc_load; nothing but BDeu reads it.  ess must be finite with
 * 1e-6 <= ess <= 1e6; anything else is ULG_ERR_ARG and leaves the previous
 * value. */
int ulg_disc_set_ess(ulg_ctx *ctx, double ess);
/* calculateScore(vars[i], parents[i]) for arbitrary pairs: the value above (of
 * either kind) without the store rule (a violating set gives 1). */
int ulg_disc_score_sets(ulg_ctx *ctx, int kind, int64_t count, const int *vars,
                        const uint64_t *parents, float *scores);
/* diagnostics: out[i] = ln C(arity, first + i), i < count, as ULG_SCORE_FNML
 * uses it: the device table's fixed-point entries converted back.  Builds the
 * table if need be.  ULG_ERR_ARG for an arity that no loaded column has or a
 * range that leaves 0 .. N; ULG_ERR_STATE without discrete data. */
int ulg_disc_regret(ulg_ctx *ctx, int arity, int64_t first, int64_t count, double *out);
/* diagnostics: the dense contingency table of one (variable, parent set).
 * Cell index = sum_p code_p base_p + code_v q, parents in ascending variable
 * order, the first with base 1, q = prod r_p.  *ncells = q r_v;
 * ULG_ERR_ARG if cap is smaller. */
int ulg_disc_counts(ulg_ctx *ctx, int var, uint64_t parents, int32_t *counts, int64_t cap, int64_t *ncells);

/* ---- BGe scoring of the continuous data (no reference counterpart) ---- */
/* The Bayesian Gaussian equivalent score (Geiger & Heckerman 2002; corrected
 * form of Kuipers, Moffa & Heckerman 2014): the continuous counterpart of BDeu,
 * a marginal likelihood instead of cBIC's penalty with its free lambda, and
 * score-equivalent.  It reads what ulg_cbic_load holds -- columns normalised to
 * zero mean and unit sample variance (N - 1), G = Z'Z on the device -- and
 * ignores lambda.  Prior: mean 0 (the sample mean of the normalised data),
 * alpha_mu > 0, alpha_w > n + 1, T = t I with
 * t = alpha_mu (alpha_w - n - 1) / (alpha_mu + 1), R = G + t I.  For |P| = l
 * and A_l = (N + alpha_w - n + l + 1) / 2:
 *   s(v, P) = c_l - 1/2 ln det R[P,P] - A_l ln sigma
 *   sigma   = R[v,v] - R[v,P] R[P,P]^-1 R[P,v]
 *   c_l     = lgamma(A_l) - lgamma((alpha_w - n + l + 1) / 2) - (N / 2) ln pi
 *             + 1/2 ln(alpha_mu / (N + alpha_mu)) + ((alpha_w - n + 2 l + 1) / 2) ln t
 * sigma is the last pivot of the Cholesky factorisation of R[Q,Q], Q = P + {v}
 * with v last, det R[P,P] the product of the pivots before it (1 for no
 * parent).  Everything runs in FP64 and is rounded to float once; c_l and A_l
 * are computed on the host once per call (csrc/bge.h).  One device function
 * computes the value (csrc/bge_dev.h: parents in ascending variable order, t
 * added to each diagonal entry as it is read, every multiply-add an fma), so a
 * pair's value is the same bits from ulg_bge_score and ulg_bge_score_sets, in
 * every call and for any grid.
 * The store rule departs from score_calculator.cpp:59,111 (the empty set iff
 * < 1, any other set iff < 0): BGe is a log density, positive as soon as the
 * residual variance of normalised data falls below about 0.06 (duplicated or
 * near-deterministic columns), so every finite value is stored, the empty set
 * included, and there is no dominance test.  A set that touches a constant
 * column (NaN in G) or whose pivot comes out <= 0 gives NaN and is never
 * stored.  A set that violates ulg_cbic_set_constraints is not evaluated and
 * never stored; ulg_bge_score_sets returns NaN for it.  Costs (-score) may
 * therefore be negative; the "%f" round trip, the best-score tables and the
 * searches take either sign.
 *
 * ulg_bge_set_prior: sticky, default (1, 0), kept across loads.  alpha_w = 0
 * means n + alpha_mu + 1 at scoring time.  ULG_ERR_ARG (and the previous prior
 * stays) outside 1e-3 <= alpha_mu <= 1e3, for a non-finite value, or for
 * 0 != alpha_w <= n + 1 or alpha_w > n + 1e6 against the n loaded at the time
 * (0 without data); the scoring calls check again against their n. */
int ulg_bge_set_prior(ulg_ctx *ctx, double alpha_mu, double alpha_w);
/* ulg_disc_score's arguments and counts: the lists replace the context's
 * (ulg_cbic_fetch, ulg_pss_format, ulg_search_from_scores read them), ordered
 * by (|set|, set value); max_parents < 1 or > n - 1 means n - 1; up to
 * ULG_MAX_PARENTS_GPU parents (ULG_ERR_UNSUPPORTED above); time_limit_ms is
 * checked after each complete layer ("out_of_time",
 * "highest_completed_layer"); *total_scored counts every set of the completed
 * layers, sum over the variables of C(m, <= k).  A refused call leaves the
 * previous lists.  One launch per layer (bge_layer_kernel), one lane per set;
 * layers of 1 .. ULG_UNROLLED_PARENTS_GPU parents run fully unrolled.
 * Option "bge_prune" (0/1, default 0, sticky; only this call reads it): 1 runs
 * ulg_disc_score's prune pass (disc_prune_kernel, unchanged) over the BGe slot
 * table: a stored set goes iff a kept proper subset scores at least as well
 * within 2 FLT_EPSILON.  ulg_get_info("bge_pruned") then gives the sets
 * removed (0 with the option off).  ULG_ERR_STATE without continuous data (no
 * load yet, or after ulg_disc_load). */
int ulg_bge_score(ulg_ctx *ctx, const int *vars, int nv, const uint64_t *candidates, int max_parents,
                  int64_t *total_stored, int64_t *total_scored);
/* s(vars[i], parents[i]) for arbitrary pairs (the variable's own bit is
 * ignored), without the store rule: NaN for a constant column, a pivot <= 0 or
 * a violating set.  At most ULG_MAX_PARENTS_GPU parents per set.  The context's
 * lists stay as they are. */
int ulg_bge_score_sets(ulg_ctx *ctx, int64_t count, const int *vars, const uint64_t *parents, float *scores);

/* ---- discrete skeleton: G^2 tests and MMPC (no reference counterpart) ---- */
/* ln of the chi-square survival function: ln P(chi2_dof >= x), pure host FP64,
 * no context.  x <= 0 gives 0.  Computed in log space (the series of the lower
 * tail below x/2 = dof/2 + 1, a Lentz continued fraction of the upper tail
 * above), so it stays finite where the probability underflows; valid for dof
 * up to 32768 and x up to 1e7.  dof = 2 gives -x/2. */
double ulg_chi2_log_sf(double x, double dof);
/* The raw statistics of count conditional-independence tests of xs[i] and
 * ts[i] given the variables in conds[i] (a mask) on the loaded value codes,
 * whether the MMPC below would call them reliable or not:
 *   cells[i] = q r_x r_t, q = prod_{s in conds} r_s;  dof[i] = (r_x - 1)(r_t - 1) q
 *   (both saturate at INT64_MAX);
 *   g2[i] = 2 [sum n_xtz ln n_xtz + sum n_z ln n_z - sum n_xz ln n_xz - sum n_tz ln n_tz],
 *   clamped at 0, empty cells contributing nothing; NaN where cells > 32768 (the
 *   table is counted in a 128 KB LDS histogram).
 * Each n ln n term is accumulated as a fixed-point integer (as ulg_disc_score's),
 * so g2 does not depend on scheduling, on the other tests of the call or on
 * their order.  ULG_ERR_ARG for x = t, for x or t in conds and for an index or
 * a mask bit out of range; ULG_ERR_STATE without discrete data.  The context's
 * lists stay as they are. */
int ulg_disc_g2(ulg_ctx *ctx, int64_t count, const int *xs, const int *ts, const uint64_t *conds,
                double *g2, int64_t *dof, int64_t *cells);
/* ulg_mmpc for the value codes of ulg_disc_load: MMPC with G^2 tests, rows as
 * ulg_mmpc returns them.  A test (X, T | S) is performed iff N >= min_per_cell
 * cells and cells <= 32768 (the heuristic power rule; a test not performed
 * contributes nothing, a pair whose marginal test is not performed is never a
 * candidate); its association is -ln p = -ulg_chi2_log_sf(G^2, dof), 0 for
 * dof = 0; X and T are independent given S iff that is <= -ln alpha.  Rounds,
 * tie-breaks and the AND rule as ulg_mmpc; max_cond < 0 or > 24 means 24; a
 * candidate set of more than 24 is ULG_ERR_UNSUPPORTED.  One launch per round,
 * one workgroup per test.  Exact rules: csrc/disc_mmpc.hip.  ULG_ERR_ARG for
 * alpha outside (0, 1) or min_per_cell < 1, ULG_ERR_STATE without discrete
 * data; the context's lists stay as they are.  ulg_get_info("disc_mmpc_tests")
 * and ("disc_mmpc_skipped") count the last call's tests performed and left out. */
int ulg_disc_mmpc(ulg_ctx *ctx, double alpha, int max_cond, int min_per_cell, uint64_t *rows);

/* The .pss "%f" + atof round trip the A* input goes through
 * (score_main.cpp:191, score_cache.cpp:151), computed exactly on the
 * device: cost = float(-1 * strtod(printf("%f", score))). */
int ulg_quantize_costs(ulg_ctx *ctx, const float *scores, float *costs,
                       int64_t count);

/* ---- the .pss score-cache text (score_main.cpp:173-203,383-400) -------- */
/* Formats the lists of the last ulg_cbic_score (every variable scored) as
 * the .pss file the reference's score command writes: `header` verbatim
 * (the META block and its blank line), then for each variable in index
 * order "VAR <name>", "META arity=<a>", one line per stored set -- the
 * score as glibc "%f" prints it, a space, each parent's name followed by a
 * space -- and a blank line.  The text is formatted on the GPU; *text points
 * to a context-owned host buffer of *len bytes (NUL-terminated), valid until
 * the next format call or ulg_destroy. */
int ulg_pss_format(ulg_ctx *ctx, const char *header, const char *const *names,
                   const int *arity, const char **text, int64_t *len);
/* Same for host lists (offsets[n+1], sets, scores; variable v owns
 * [offsets[v], offsets[v+1]) ), e.g. after the multi-GPU exchange. */
int ulg_pss_format_lists(ulg_ctx *ctx, int n, const int64_t *offsets,
                         const uint64_t *sets, const float *scores,
                         const char *header, const char *const *names,
                         const int *arity, const char **text, int64_t *len);

/* ---- search side (best-score tables, pattern database, A*) ------------ */
/* Load per-variable parent-set lists (file order within each variable;
 * costs = A* costs, i.e. -1 * atof(score), score_cache.cpp:151) and build
 * the best-score lattice tables on the device.  Duplicate sets within a
 * variable must already be merged (ScoreCache::putScore semantics). */
int ulg_search_load(ulg_ctx *ctx, int n, const int64_t *offsets,
                    const uint64_t *sets, const float *costs);
/* Same from the lists the last ulg_cbic_score produced in this context
 * (every variable must have been scored); costs go through the device
 * "%f" round trip (ulg_quantize_costs), lists stay on the device. */
int ulg_search_from_scores(ulg_ctx *ctx);
/* Same from per-variable lists of .pss scores (not yet costs) in variable
 * order -- what the multi-GPU exchange hands every rank (one
 * all-gather of the per-variable lists, then local tables).  offsets[n+1] is
 * a host array (variable v owns [offsets[v], offsets[v+1]) of sets/scores);
 * device_ptrs = 1: sets and scores are device pointers on this context's GPU
 * (e.g. the all-gather's output tensor), 0: host pointers.  Scores go
 * through the device "%f" round trip like ulg_search_from_scores. */
int ulg_search_load_scores(ulg_ctx *ctx, int n, const int64_t *offsets,
                           const uint64_t *sets, const float *scores,
                           int device_ptrs);
/* SparseParentList::getScore / getParents for count (variable, S) pairs:
 * the cost of the first (cost, file-order) stored set that is a subset of
 * S, or FLT_MAX if none; parents[i] gets that set (0 if none). */
int ulg_bestscore_query(ulg_ctx *ctx, int64_t count, const int *vars,
                        const uint64_t *S, float *costs, uint64_t *parents);
/* StaticPatternDatabase with pd_count groups over scc (and ancestors);
 * static_pattern_database.cpp:82-247.  astar() builds it over all
 * variables with no ancestors. */
int ulg_pdb_build(ulg_ctx *ctx, int pd_count, uint64_t ancestors,
                  uint64_t scc);
/* StaticPatternDatabase::h for count subnetworks S. */
int ulg_pdb_query(ulg_ctx *ctx, int64_t count, const uint64_t *S, float *h,
                  int *complete);
/* Read-back of one variable's best-score table as the device holds it (for
 * tests; the searches never call it): *support = D_var, the union of var's
 * stored sets inside the tables' scope, *count = 2^|D_var|, and costs[i] =
 * the table's cost for the S with pext(S, D_var) = i, FLT_MAX where no stored
 * set fits.  costs == NULL or cap == 0 returns support and count only.
 * *count = 0 for a variable that has no table (the sharded sweep's tables
 * cover its own variables only).  ULG_ERR_STATE when no tables are built
 * (no lists, or the budget refused them), ULG_ERR_ARG for a bad var or a
 * cap below *count. */
int ulg_bestscore_table(ulg_ctx *ctx, int var, uint64_t *support, float *costs,
                        int64_t cap, int64_t *count);
/* Read-back of one pattern-database group from the device array (for tests):
 * *mask = the group's variables (0 for an empty group), *count = 2^|mask|,
 * values[i] = pd[R] for the R inside mask with pext(R, mask) = i.  values ==
 * NULL or cap == 0 returns mask and count only.  ULG_ERR_STATE without a
 * pattern database, ULG_ERR_ARG for a group outside 0..pd_count-1 or a cap
 * below *count. */
int ulg_pdb_table(ulg_ctx *ctx, int group, uint64_t *mask, float *values,
                  int64_t cap, int64_t *count);

#define ULG_ASTAR_EXACT 0 /* the reference's pop order: bit-exact DAG */
#define ULG_ASTAR_GPU 1   /* layer-synchronous GPU order-graph search */
/* astar() (astar_main.cpp:548-644): static PDB(pd_count) over all
 * variables, one search per connected component of the skeleton
 * (edges = n skeleton rows, bit j of row i = edge i-j, or NULL for no
 * skeleton).  Outputs what netFile.csv holds -- vpar[v] = parent set of v
 * (bit i set iff i -> v) -- the total ordering, the goal cost (g of the
 * goal node) and the number of expanded nodes; net_text (if non-NULL)
 * receives the netFile text.  Components are processed in order and each
 * overwrites the outputs, as the reference does. */
int ulg_astar(ulg_ctx *ctx, const uint64_t *edges, int pd_count, int mode,
              uint64_t *vpar, int *order, float *goal_cost, int64_t *expanded,
              char *net_text, int64_t net_cap);
/* astar() with the -p / -s options (astar_main.cpp:590-644, UAI '14): the
 * heuristic is built over (ancestors, scc); each skeleton component (all
 * variables without a skeleton) is searched from the root `ancestors` to
 * ancestors | component.  ulg_astar = ancestors 0, scc all.  Ancestors must
 * not overlap scc; the GPU mode takes no ancestors. */
int ulg_astar_scc(ulg_ctx *ctx, const uint64_t *edges, int pd_count, int mode,
                  uint64_t ancestors, uint64_t scc, uint64_t *vpar, int *order,
                  float *goal_cost, int64_t *expanded, char *net_text,
                  int64_t net_cap);

/* triplet_astar's astar() (astar/triplet_astar.cpp:991-1622): for every
 * variable i and pair of its skeleton neighbours, an exact-order A* with
 * re-opening (run_astar_on_one_scc, :285-674) over the union of the three
 * clusters (skipped above 26 variables, :837-844; one search per distinct
 * cluster -- the result depends on the cluster only), v-structure and
 * undirected-edge bookkeeping (process_triple, :811-989), the
 * unfaithful-edge fixpoint (:1256-1290) and Meek rules 2-4 (:1297-1478).
 * directed_graph (n*n ints, row-major) receives what netFile.csv holds:
 * [i*n+j] = 1 iff the MEC has i -> j (both set = undirected).  edges as in
 * ulg_astar (NULL = no skeleton: every row is the full set, self included).
 * stats (optional, 3 entries): A* runs requested, distinct clusters
 * searched, nodes expanded. */
int ulg_triplet_astar(ulg_ctx *ctx, const uint64_t *edges, int pd_count,
                      int *directed_graph, int64_t *stats);

/* Multi-GPU triplet_astar (distinct clusters are independent A*
 * problems).  The per-cluster results live in a memo on the context, valid
 * for the loaded lists and one pd_count; ulg_triplet_astar reads and fills
 * it, so its stats count only the searches that call made.
 *   ulg_triplet_clusters: the distinct clusters (<= 26 variables) of the
 *     driver's first sweep on the initial skeleton (triplet_astar.cpp:
 *     1148-1204), in first-request order, no searching; *count = how many
 *     (fails with ULG_ERR_ARG if cap is too small and nonzero).
 *   ulg_triplet_solve: the re-opening exact-order A* (:285-674) of each
 *     cluster into the memo; parents (optional, nc*n) receives each cluster
 *     DAG's parent sets.  stats as ulg_triplet_astar.
 *   ulg_triplet_memo_put: seed the memo with other ranks' results.
 * Sharded over ranks, the clusters are solved once each and gathered; every
 * rank then runs ulg_triplet_astar with a full memo and gets the same MEC a
 * single GPU would (a result depends on its cluster only). */
int ulg_triplet_clusters(ulg_ctx *ctx, const uint64_t *edges, uint64_t *clusters,
                         int64_t cap, int64_t *count);
int ulg_triplet_solve(ulg_ctx *ctx, const uint64_t *clusters, int64_t nc,
                      int pd_count, uint64_t *parents, int64_t *stats);
int ulg_triplet_memo_put(ulg_ctx *ctx, const uint64_t *clusters, int64_t nc,
                         int pd_count, const uint64_t *parents);

/* ---- order-graph sweep with variable-sharded tables ----------
 * Replaces run_astar_on_one_scc (astar_main.cpp:216-546) for a full skeleton
 * when one GPU cannot hold every variable's best-score lattice (n >= 31: at
 * n = 32, 32 x 2^31 x 4 B = 275 GB).  Every rank holds every variable's
 * parent-set lists (after the list all-gather) but builds the tables and
 * sweep slices of its own variables only.  Layer by layer (1..n):
 *   ulg_sweep_shard_layer writes, for each of the layer's C(n, layer) nodes
 *     in colex order, this rank's best candidate over the leaves it owns as
 *     a key (ordered cost << 8 | leaf position; 0xFFFFFFFFFF = none) into
 *     keys_dev (device memory, int64-compatible: every key is < 2^40);
 *   the caller MIN-all-reduces keys_dev over the ranks (one RCCL all-reduce
 *     per layer: the smallest cost, then the smallest leaf position -- the
 *     single-GPU sweep's first-strict-minimum rule);
 *   ulg_sweep_shard_commit turns the reduced keys into the layer's g and
 *     leaf bytes (every rank holds all of them).
 * ulg_sweep_shard_end reconstructs the DAG as ULG_ASTAR_GPU does; the result
 * equals the single-GPU ulg_astar(..., ULG_ASTAR_GPU, ...) on a full skeleton
 * bit for bit.  *max_layer_nodes = the largest C(n, layer) (size keys_dev for
 * it).  NaN costs are not supported (their key order differs from the
 * single-GPU float compare). */
int ulg_sweep_shard_begin(ulg_ctx *ctx, uint64_t own, int64_t *max_layer_nodes);
int ulg_sweep_shard_layer(ulg_ctx *ctx, int layer, uint64_t *keys_dev);
int ulg_sweep_shard_commit(ulg_ctx *ctx, int layer, const uint64_t *keys_dev);
int ulg_sweep_shard_end(ulg_ctx *ctx, uint64_t *vpar, int *order, float *goal_cost,
                        int64_t *expanded);
/* Read-only view of a finished sweep: the leaf bytes of the last component
 * ulg_astar(..., ULG_ASTAR_GPU, ...) searched on this context, or of the
 * last ulg_sweep_shard_end, whichever ran later -- one byte per node of the
 * component's 2^m lattice, layers 0..m in order and colex rank (over the
 * component's variables in ascending order) within a layer.  The byte is the
 * position j, among the node's elements in ascending order, of the leaf its
 * cost came through (the first strict minimum), 255 for a node no admissible
 * predecessor reaches; the layer-0 byte is not written by the sweep.
 * *count = 2^m; cap = 0 only asks for it, a smaller nonzero cap is
 * ULG_ERR_ARG.  ULG_ERR_STATE if no sweep has finished (the buffers are
 * rewritten by the next GPU search or ulg_sweep_shard_begin).  No kernel
 * runs: one device-to-host copy. */
int ulg_sweep_leaves(ulg_ctx *ctx, uint8_t *out, int64_t cap, int64_t *count);

/* ---- exact model averaging over the order lattice (no reference counterpart) ----
 * What a Bayesian score (BDeu, BGe: log marginal likelihoods) is for beyond the
 * single best DAG: the posterior probability of every stored parent set, the
 * n x n matrix of edge posteriors and ln Z, by the sum-product form of the
 * lattice recursions the searches run in min-plus form (Koivisto & Sood 2004;
 * Koivisto 2006).  No sampling: the sums are exact.
 *
 * Input: per-variable lists (offsets[n+1], sets, scores), ulg_search_load_scores'
 * layout.  Scores are natural-log float32 values of either sign.  V = {0..n-1};
 * a stored set P of v has weight w_v(P) = exp(s_v(P)), an absent set weight 0.
 * The model is the ORDER-MODULAR prior: the pair (linear order <, DAG G whose
 * every parent set precedes its child in <) has weight prod_v w_v(Pa_v).  It
 * is NOT uniform over DAGs: a DAG counts once per linear extension, so DAGs
 * with many topological orders weigh more than under a flat structure prior.
 * All in FP64 log space (a table holds ln of the quantity, -inf for 0):
 *   alpha_v(S) = sum_{stored P subset of S} w_v(P),  S subset of V\{v}
 *                2^(n-1) entries per variable; index of S = S with bit v
 *                squeezed out (subset-sum transform of the scattered list)
 *   f(0) = 1,  f(S) = sum_{v in S} f(S\v) alpha_v(S\v);     Z = f(V)
 *   b(0) = 1,  b(T) = sum_{v in T} alpha_v(V\T) b(T\v)      (v first of T, its
 *                predecessors exactly V\T);                  b(V) = Z as well
 *   g_v(S) = f(S) b(V\S\{v}),   gamma_v(P) = sum_{S superset of P, S subset of V\{v}} g_v(S)
 *   p(Pa_v = P) = w_v(P) gamma_v(P) / Z   for every stored P
 *   p(u -> v)   = sum_{stored P containing u} p(Pa_v = P)
 * f and b are indexed by the mask itself.
 * Log space: logaddexp(a, b) = max + log1p(exp(-|a - b|)); -inf when both are
 * -inf (inf - inf is never formed); the maximum unchanged when the gap exceeds
 * 38 nats (exp(-38) < 2^-54: below half an ulp of any maximum of magnitude
 * >= 1/2, and an absolute 5.6e-17 below that) -- one device function
 * (csrc/posterior_dev.h) that every kernel uses.  Every output is a fixed
 * expression tree of its inputs: the sweeps' sums run over v ascending, the
 * transforms take bit 0 upward, the per-variable and per-edge sums take the
 * maximum first (order-free) and then add in an order fixed by the list alone
 * (entry i goes to lane i mod 256, lanes add their entries ascending, then a
 * fixed binary tree over the lanes).  No floating-point atomics: the results
 * are bit-identical across calls, contexts and launch geometry.
 * set_logpost[i] = s_i + ln gamma_v(P_i) - L_v with L_v the log of the sum of
 * w gamma over v's own stored sets.  L_v = ln Z in exact arithmetic
 * (sum_S g_v(S) alpha_v(S) = Z for every v) and differs from the forward
 * sweep's ln Z by rounding only; normalising by it makes a variable's stored
 * sets sum to 1 to the last bit the sum allows, and gives the only set of a
 * variable exactly 0.0.  If Z = 0 (e.g. a variable with an empty list) the
 * call succeeds with *log_z = -inf, every set_logpost -inf and every edge 0.
 *
 * ulg_posterior: offsets is a host array; device_ptrs = 1: sets and scores are
 * device pointers on this context's GPU, 0: host pointers.  Outputs are host
 * pointers: edge[u*n+v] = p(u -> v), diagonal 0; set_logpost (one per list
 * entry, in list order) may be NULL.
 * ulg_posterior_from_scores: the lists of the last scoring call of any kind
 * (ulg_cbic_score*, ulg_disc_score, ulg_bge_score; a pending async call is
 * collected first), scores as they are -- not the "%f" costs.  That call must
 * have scored every variable once; its vars may name them in any order (the
 * lists are put in index order here, as ulg_search_from_scores does).  A call
 * that scored only some variables, or one twice, is ULG_ERR_STATE.
 * set_logpost is in variable index order, each variable's sets in their stored
 * order.
 * Lists pruned by dominance (cBIC's store rule, "disc_prune", "bge_prune")
 * give the posterior over the pruned family only: Z is then a lower bound of
 * the full sum, not the full average.
 * ulg_posterior_table (tests, in the manner of ulg_bestscore_table): one table
 * of the last successful posterior call.  which = 0: ln alpha_var, 1: ln f,
 * 2: ln b, 3: ln gamma_var.  *count = 2^(n-1) for 0 and 3, 2^n for 1 and 2 (var
 * is ignored); cap = 0 asks for the count only, a smaller nonzero cap is
 * ULG_ERR_ARG.  The gamma tables are kept on request: with option
 * "posterior_keep" 1 at the time of the call all n stay on the device; with 0
 * (the default) one table is reused variable after variable and which = 3 is
 * ULG_ERR_STATE.  ULG_ERR_STATE without a successful posterior call.
 * Errors: ULG_ERR_ARG for n < 1, offsets not ascending, a set with its own
 * variable's bit or a bit >= n, a duplicate set within a variable, a NaN or
 * infinite score (sets and scores are checked on the device, by the pass that
 * scatters them); ULG_ERR_UNSUPPORTED for n > 28 or when tables and lists do not
 * fit the free device memory -- decided before anything is allocated, the
 * message names the bytes needed.  Tables: 8 B x (n 2^(n-1) + 2 x 2^n + G 2^(n-1)),
 * G = 1 gamma table, n with "posterior_keep" (n = 25: 4.0 GB, n = 28: 35 GB);
 * ulg_get_info("posterior_bytes") gives that figure for the last successful
 * call.  Neither call touches the context's lists, the search tables, the
 * pattern database or the .pss state. */
int ulg_posterior(ulg_ctx *ctx, int n, const int64_t *offsets, const uint64_t *sets,
                  const float *scores, int device_ptrs, double *log_z, double *edge,
                  double *set_logpost);
int ulg_posterior_from_scores(ulg_ctx *ctx, double *log_z, double *edge, double *set_logpost);
int ulg_posterior_table(ulg_ctx *ctx, int which, int var, double *out, int64_t cap, int64_t *count);

/* Sampling: independent (linear order, DAG) draws from the same order-modular
 * posterior, for the features that do not factor over one parent set (paths,
 * Markov blankets, v-structures, whole DAGs): any feature is a sample mean,
 * another structure prior an importance weight.  Backward sampling through the
 * forward table of the last successful ulg_posterior* call of the context
 * (its lists, ln alpha_v and ln f stay on the device): exact i.i.d. draws, no
 * MCMC and no burn-in.  A sample walks from S = V down to the empty set; the
 * step at |S| = l has position i = l - 1 and makes two choices:
 *   1. sink:        v in S with probability f(S\v) alpha_v(S\v) / f(S)
 *   2. parent set:  a stored P subset of S\v of v with probability
 *                   w_v(P) / alpha_v(S\v);  then S <- S\v.
 * v is the variable at position i of the order.  The law of the pair is the
 * order-modular posterior above, so p(Pa_v = P) under it is what set_logpost
 * reports.
 * Every choice is made in integers, as the discrete scorer's fixed-point sums
 * are: no choice depends on a summation order or on the launch geometry.
 *   weights  sink candidates: v in S ascending,
 *              x_v = (ln f(S\v) + ln alpha_v(S\v)) - ln f(S), in FP64 in that
 *              order; set candidates: v's list entries in list order,
 *              x_i = (double) s_i - ln alpha_v(S\v) for P_i subset of S\v, an
 *              entry that is not compatible has weight 0.
 *              q = 0 for x = -inf, else q = (uint64) floor(exp(x) 2^52).
 *   pick     T = sum of q (about 2^52: it never overflows); t = the high 64
 *              bits of U T for a 64-bit draw U; the choice is the first
 *              candidate j with C_j > t, C the running integer sum.  A
 *              candidate of weight 0 is never chosen.  Each step's
 *              probabilities are within (number of candidates) 2^-52 of the
 *              exact ones (the floors), beyond what exp's rounding moves x.
 *   draws    Philox4x32-10 with key (lo32(seed), hi32(seed)) and counter
 *              (lo32(k), hi32(k), i, 0) gives (w0 .. w3); k = the global
 *              sample index, i the step's position; U_sink = w0 | w1 << 32,
 *              U_set = w2 | w3 << 32.  Sample k depends on (tables, lists,
 *              seed, k) alone: a range may be split over calls at will.
 * One definition of all three (csrc/posterior_sample_dev.h) serves every path.
 * ulg_posterior_sample: samples first .. first + count - 1.  Outputs are host
 * pointers: parents[k*n + v] = the parent mask of v in sample first + k;
 * order[k*n + i] = the variable at position i, 0 first (may be NULL);
 * log_weight[k] = sum over v ascending of (double) s_v(Pa_v) (may be NULL).
 * count = 0 succeeds and writes nothing, and does no device work; the checks
 * of first and of the state come before it (ULG_ERR_STATE without a successful
 * posterior call also for count = 0), the look at ln Z after it.
 * ulg_posterior_sample_u (tests, in the manner of ulg_posterior_table): the
 * same kernel with the draws read, not generated: u[(k*n + i)*2] is U_sink and
 * u[(k*n + i)*2 + 1] U_set of step position i of sample k (host pointer).
 * Errors: ULG_ERR_STATE without a successful posterior call on the context, or
 * when its ln Z = -inf; ULG_ERR_ARG for a negative first or count or a NULL
 * parents (or u) with count > 0; ULG_ERR_UNSUPPORTED, decided before anything
 * is allocated, when the call's device buffers (8 n bytes per sample, n more
 * with order, 8 more with log_weight, 16 n more for u) do not fit the free
 * device memory.  The buffers are kept from one sampling call to the next and
 * freed by the next ulg_posterior* call before it sizes its tables.  Neither
 * call changes the tables (ulg_posterior_table), the
 * context's lists (ulg_cbic_fetch) or the search state. */
int ulg_posterior_sample(ulg_ctx *ctx, uint64_t seed, int64_t first, int64_t count,
                         uint64_t *parents, uint8_t *order, double *log_weight);
int ulg_posterior_sample_u(ulg_ctx *ctx, int64_t count, const uint64_t *u, uint64_t *parents,
                           uint8_t *order, double *log_weight);

/* The importance weight that turns those samples into estimates under the
 * prior uniform over DAGs: the law of a sampled DAG is ext(G) prod_v w_v(Pa_v)
 * / Z, ext(G) its number of linear extensions (topological orders), so a
 * sample weighted by 1 / ext(G) stands for prod_v w_v(Pa_v) alone (Ellis &
 * Wong 2008).  ulg_dag_linear_extensions counts ext(G) exactly for each of
 * `count` DAGs by the recursion over the subset lattice
 *   c(0) = 1,  c(S) = sum over v in S with Pa_v subset of S\v of c(S\v),
 *   ext(G) = c(V):
 * c(S) is the number of orderings of S in which every member's parents come
 * first, 0 when S is not closed under parents; hence ext = 0 for a graph with
 * a directed cycle, which is an answer and not an error.  ext <= n! < 2^98:
 * the count is a 128-bit unsigned integer, ext_lo[k] + 2^64 ext_hi[k], and the
 * device adds in two 64-bit words with carry (csrc/linext_dev.h), so every
 * output is the exact integer whatever the launch geometry or the batching.
 * parents[k*n + v] = the parent mask of v in DAG k, the layout
 * ulg_posterior_sample writes.  All pointers are host pointers; ext_hi and
 * log_ext may be NULL.  log_ext[k] = (double) logl((long double) hi 2^64 +
 * (long double) lo), formed on the host from the exact words; -inf for 0.
 * The call needs no loaded data, lists or posterior state and changes none:
 * ulg_cbic_fetch, ulg_posterior_table and a following ulg_posterior_sample
 * give what they gave before.
 * Device memory: 16 * 2^n bytes of table per DAG (n = 20: 16 MB, 25: 512 MB,
 * 28: 4 GB) plus 4 n + 16 for its masks and result.  The DAGs are processed
 * in batches: as many per batch as 2^30 bytes of tables hold (1023 at n = 16,
 * 63 at n = 20, one from n = 25 on) within seven eighths of the free device
 * memory, one at least; and at most "linext_batch" of them when that option
 * is positive.  More per batch buys nothing once a launch fills the card, and
 * a large allocation costs more than the count.  ulg_get_info
 * ("linext_batches") gives the batches of the last call (0 for count = 0).
 * The buffers are the call's own and are freed when it returns.
 * Errors: ULG_ERR_ARG for n < 1, a negative count, a NULL parents or ext_lo
 * with count > 0, a mask with the variable's own bit or a bit >= n (every
 * mask is checked before any device work; nothing is written);
 * ULG_ERR_UNSUPPORTED for n > 28, or when one DAG's table does not fit the
 * free device memory, decided before anything is allocated.  count = 0
 * succeeds without device work. */
int ulg_dag_linear_extensions(ulg_ctx *ctx, int n, int64_t count, const uint64_t *parents,
                              uint64_t *ext_lo, uint64_t *ext_hi, double *log_ext);

/* What the samples are for: the features that do not factor over one parent
 * set, as posterior sample means.  ulg_dag_features reduces a batch of `count`
 * DAGs (parents[k*n + v] = the parent mask of v in DAG k, the layout above) to
 * tables of exact integer sums over the ACYCLIC graphs G_k of the batch, each
 * graph weighted by the integer q_k = weight[k] (weight NULL: every q_k = 1):
 *   edge[u*n + v]       sum of q_k over the G_k with u in Pa_v
 *   ancestor[u*n + v]   ... with a directed path of at least one edge from u
 *                       to v (diagonal 0)
 *   blanket[u*n + v]    ... with u != v a parent, a child or a parent of a
 *                       child of v (symmetric)
 *   compelled[u*n + v]  ... with u in Pa_v and u -> v directed in the
 *                       essential graph (CPDAG) of G_k: every DAG with G_k's
 *                       skeleton and v-structures has the edge in this
 *                       direction.  For a score-equivalent score (BGe, BDeu)
 *                       the data cannot tell the members of such a class
 *                       apart, so this, not edge, is the directed statement
 *                       the data supports.
 *   vstruct[(v*n + u)*n + w], u < w   ... with u -> v <- w and u, w not
 *                       adjacent; every other entry 0
 *   total               sum of q_k over the acyclic graphs
 *   cyclic              the number (not the weight) of graphs with a directed
 *                       cycle.  Such a graph contributes to nothing else: an
 *                       answer, not an error.
 * A caller divides by total.  The essential graph starts from the edges that
 * take part in a v-structure and is closed under Meek's rules R1-R3 (R4 is
 * not needed from a DAG's own v-structures); csrc/dagfeat_dev.h states the
 * rules row by row and host/dagfeat_check.cpp runs them against the
 * definition.  One wave64 per DAG, lane v holding row v; the sums are 64-bit
 * integer adds, so every output is the same to the bit whatever the launch
 * geometry, the batching or the order of the atomics.
 * All pointers are host pointers.  Each of edge, ancestor, blanket, compelled
 * (n*n values) and vstruct (n*n*n) may be NULL: what is not asked for is not
 * computed.  cyclic may be NULL; total may not.
 * n <= 63: the call needs no lattice, so the sampler's n <= 28 does not bind
 * it.  The call needs no loaded data, lists or posterior state and changes
 * none.  Its device buffers (8 n bytes per DAG in chunks of at most 2^28
 * bytes, 8 per weight, 8 (4 n^2 + n^3 + 2) of tables) are its own and are
 * freed when it returns.  Option "dagfeat_grid" sets the workgroups of its
 * launches; ulg_get_info("dagfeat_grid") gives those of the last call.
 * Errors: ULG_ERR_ARG for n < 1, a negative count, a NULL parents with
 * count > 0, a NULL total, a mask with the variable's own bit or a bit >= n,
 * weights that sum to 2^63 or more (every mask and the sum are checked on the
 * host before any device work; nothing is written); ULG_ERR_UNSUPPORTED for
 * n > 63.  count = 0 succeeds without device work and zero-fills the outputs
 * that were given. */
int ulg_dag_features(ulg_ctx *ctx, int n, int64_t count, const uint64_t *parents,
                     const uint64_t *weight, uint64_t *edge, uint64_t *ancestor,
                     uint64_t *blanket, uint64_t *compelled, uint64_t *vstruct,
                     uint64_t *total, int64_t *cyclic);

/* Order MCMC (Friedman & Koller 2003): the same posterior past the lattice's
 * n <= 28.  A Metropolis-Hastings chain over linear orders whose stationary
 * law is the order marginal of the model above,
 *   p(<) proportional to prod_v A_v(pred_<(v)),  A_v(U) = sum_{stored P subset of U} w_v(P),
 * and, given an order, the sampler's second step: P with probability
 * w_v(P) / A_v(U).  A record is then an (order, DAG) pair from the
 * order-modular posterior in ulg_posterior_sample's layout, approximately and
 * with correlation along a chain -- what R-hat and the acceptance rate are
 * read for -- where ulg_posterior_sample's draws are exact and independent.
 * No table: memory is the lists plus O(n) per chain, 1 <= n <= 63.
 * Input: per-variable lists (offsets[n+1], sets, scores), ulg_posterior's
 * layout and validation (device_ptrs as there).
 *   order term  for variable v with predecessor set U, a_v(U) = ln A_v(U), a
 *              fixed function of (v's list, U) made in integers:
 *              m = the maximum of (double) s_i over the compatible entries
 *              (P_i subset of U); none: a = -inf.  q_i = floor(exp((double) s_i
 *              - m) 2^52) for a compatible entry (the sampler's weight,
 *              csrc/posterior_sample_dev.h), 0 otherwise.  T = sum q_i as an
 *              exact 128-bit integer, two 64-bit words with carry
 *              (csrc/linext_dev.h's add): more than 4096 near-maximal entries
 *              pass 2^64.  y = ldexp((double) T_hi, 12) + ldexp((double) T_lo,
 *              -52), a = m + log(y).  A single compatible entry gives exactly
 *              (double) s.  Integer sums have no order: a term does not
 *              depend on lanes, waves or grid.
 *   draws      Philox4x32-10 as above, key (lo32(seed), hi32(seed)), counter
 *              (lo32(t), hi32(t), c, d): c the chain, t the global step index
 *              (steps are 1, 2, ...), d a domain.
 *              initial order (none given): t = 0.  From the identity, for
 *                p = n-1 down to 1: the draw with d = p, r = mulhi32(w0, p+1)
 *                (the high 32 bits of the product), positions p and r swapped.
 *              move of step t: d = 0.  i = mulhi32(w0, n), j' = mulhi32(w1,
 *                n-1), j = j' + (j' >= i); U_acc = w2 | w3 << 32.  The
 *                proposal swaps positions i and j (symmetric).  n = 1: nothing
 *                is proposed, the step counts as rejected.
 *              parent set of position p of a record at step t: d = 1 + p,
 *                U_set = w0 | w1 << 32.
 *   acceptance lo = min(i, j), hi = max(i, j); the terms of positions lo..hi
 *              are recomputed as a'_p.  delta = (sum_{p = lo..hi ascending}
 *              a'_p) - (sum_{p = lo..hi ascending} a_p), FP64 in that order.
 *              Rejected if any a'_p = -inf (delta is then -inf); else
 *              accepted if delta >= 0; else iff (U_acc >> 12) <
 *              floor(exp(delta) 2^52).
 *   records    after every step t with t mod thin = 0 a chain records its
 *              order, log_score = sum_{p ascending} a_p (the full sum) and,
 *              if asked, a DAG: for the variable v at each position p,
 *              x_i = (double) s_i - a_p over v's entries in list order, 0 for
 *              an incompatible one, q = floor(exp(x_i) 2^52), then the
 *              sampler's pick with U_set.  log_weight = sum over v ascending
 *              of (double) s_v(Pa_v).  Record r (0-based within the call) of
 *              chain c has index idx = r chains + c: order[idx n + p],
 *              log_score[idx], parents[idx n + v], log_weight[idx].
 * Hence chain c depends on (lists, seed, c, its initial order) alone -- not
 * on the number of chains, the launch geometry (option "mcmc_waves"), the
 * steps per launch ("mcmc_launch_steps") or how steps are split over calls:
 * run(a); run(b) equals run(a + b) bit for bit, records included (whether a
 * record is taken depends on the global t).
 * ulg_order_mcmc_begin copies the lists to the device, checks them there,
 * sets every chain's order (init_order: chains*n bytes, row c = chain c's
 * order, position 0 first; NULL: the shuffle above) and terms, step = 0.
 * ulg_order_mcmc_begin_from_scores: the lists of the last scoring call, as
 * ulg_posterior_from_scores takes them.
 * ulg_order_mcmc_run advances every chain by `steps`.  With t0 the steps done
 * before the call, *records = floor((t0 + steps) / thin) - floor(t0 / thin)
 * records per chain; the caller sizes order (records chains n bytes),
 * log_score and log_weight (records chains doubles) and parents (records
 * chains n masks) by it (t0: ulg_order_mcmc_state).  accepted[c] = chain c's
 * accepted moves since begin.  trace_delta / trace_accept (tests): delta and
 * the decision (1 accepted) of step t at [(t - t0 - 1) chains + c], steps x
 * chains entries; for n = 1 delta reads -inf.  Every output is a host
 * pointer and may be NULL (what is not asked for is not computed; log_weight
 * without parents is ULG_ERR_ARG).
 * ulg_order_mcmc_state: order (chains n bytes), terms (chains n doubles,
 * terms[c n + p] = a of position p) and *step as they stand; each may be NULL.
 * ulg_order_score: terms[k n + p] = a of position p of order k (orders: count
 * n bytes, each a permutation) on the lists of the last begin -- the same
 * device function, the same bits.
 * The state -- the lists' device copy and per chain the order, terms and
 * accepted count, a struct of its own beside the model averaging's -- is kept
 * until the next begin; a ulg_posterior* call frees it before it sizes its
 * tables, as it frees the sampler's buffers.  Every begin ends the chains of
 * the one before, a refused begin too, whatever it is refused for: after it
 * run, state and score are ULG_ERR_STATE until a begin succeeds (a refused run
 * or score leaves the chains as they were).  None of these calls touches the
 * posterior tables, the context's lists or the search state.
 * Errors: ULG_ERR_UNSUPPORTED for n > 63, and, decided before anything is
 * allocated, when the buffers (lists 12 B per entry and 16 B per entry for
 * the duplicate check, 9 n + 8 B per chain; a run's records and traces) do
 * not fit the free device memory.  ULG_ERR_ARG for n < 1, chains outside
 * 1..2^20, offsets not ascending, a set with its own variable's bit or a bit
 * >= n, a duplicate set, a NaN or infinite score, an init_order (or orders)
 * row that is not a permutation, a chain whose initial order has a -inf term
 * (an order of probability 0; the message names the chain), steps < 0,
 * thin < 1.  ULG_ERR_STATE for run, state or score without a successful
 * begin before it. */
int ulg_order_mcmc_begin(ulg_ctx *ctx, int n, const int64_t *offsets, const uint64_t *sets,
                         const float *scores, int device_ptrs, int64_t chains, uint64_t seed,
                         const uint8_t *init_order);
int ulg_order_mcmc_begin_from_scores(ulg_ctx *ctx, int64_t chains, uint64_t seed,
                                     const uint8_t *init_order);
int ulg_order_mcmc_run(ulg_ctx *ctx, int64_t steps, int64_t thin, uint8_t *order,
                       double *log_score, uint64_t *parents, double *log_weight,
                       int64_t *accepted, double *trace_delta, uint8_t *trace_accept,
                       int64_t *records);
int ulg_order_mcmc_state(ulg_ctx *ctx, uint8_t *order, double *terms, int64_t *step);
int ulg_order_score(ulg_ctx *ctx, int64_t count, const uint8_t *orders, double *terms);

/* Rao-Blackwellised edge posteriors of given orders (Friedman & Koller's
 * estimator): given an order <, the edge posterior has a closed form over the
 * very entries the order's term scans,
 *   p(u -> v | <) = sum_{stored P subset of pred(v), u in P} w_v(P) / A_v(pred(v)),
 * and its mean over orders recorded by ulg_order_mcmc_run estimates
 * p(u -> v | D) of the same order-modular posterior with a variance that is
 * never above that of the sampled DAGs' 0/1 indicator.  It does not mend a
 * chain that has not mixed.  On the lists of the last successful
 * ulg_order_mcmc_begin*, as ulg_order_score.
 *   orders     count n bytes, each row a permutation, position 0 first.
 *   edge       groups n n values; order k adds into group k mod groups at
 *              [g n n + u n + v].  groups = 1: the batch sum; groups = chains
 *              on ulg_order_mcmc_run's record layout (idx = r chains + c):
 *              per-chain sums; groups = count: a matrix per order.
 *   zero       (may be NULL) the number of orders with a term of -inf (an
 *              order of probability 0).  Such an order adds nothing to any
 *              table: an answer, not an error.
 *   edge term  one order's contribution.  For position p, v = order[p], U the
 *              predecessors: m, the compatible entries, q_i = floor(exp((double)
 *              s_i - m) 2^52) and T = sum q_i exactly as in the order term
 *              above.  For u in U, N_u = sum of q_i over the compatible
 *              entries with u in P_i, an exact 128-bit integer (two words with
 *              carry).  y(X) = ldexp((double) X_hi, 12) + ldexp((double) X_lo,
 *              -52), the order term's conversion.  g(u -> v) = (uint64)
 *              floor(ldexp(y(N_u) / y(T), 40)): FP64, one IEEE division.
 *              Hence g <= 2^40, g = 2^40 when every compatible entry of
 *              positive weight holds u (N_u = T; beyond that only where y
 *              rounds N_u and T to one double), g = 0 for u outside U and on
 *              the diagonal.  A group's value is the 64-bit integer sum of
 *              its orders' g.
 * Every output is therefore the same bits whatever the lanes, waves, grid
 * (option "edges_grid"), batching or the split of `count` over calls: the sum
 * of two calls' tables equals one call's.  A caller divides by 2^40 (orders in
 * the group - its zero orders).
 * Errors: ULG_ERR_STATE without a successful begin.  ULG_ERR_ARG for
 * count < 0, count > 2^22 (a sum stays below 2^62), groups < 1 or groups >
 * max(count, 1), NULL orders with count > 0, NULL edge, a row that is not a
 * permutation: checked on the host before any device work, nothing is
 * written.  ULG_ERR_UNSUPPORTED, decided before anything is allocated, when
 * the call's buffers (count (n + 1) + 8 groups n^2 + n bytes) do not fit
 * the free device memory.  count = 0 zero-fills the tables and succeeds.  The
 * device buffers are the call's own and freed when it returns; it touches
 * neither the chains, the posterior tables nor the context's lists. */
int ulg_order_edges(ulg_ctx *ctx, int64_t count, const uint8_t *orders, int64_t groups,
                    uint64_t *edge, int64_t *zero);

/* ---- tuning knobs -------------------------------------------------------
 * "score_variant" (1, 49, 65, 113, 241; default 241): bit 0 = fully
 * unrolled presence gather (layers <= 6), bit 4 = two-pass layers (the
 * scoring kernel settles every set it can without a walk and queues the rest
 * for a dense walk kernel with the hi-cover prune), bit 5 = that walk
 * bit-sliced (64 x K sets per wave), bit 6 = subset maxima (a per-slot table
 * of the largest stored value below each set settles sets with 2L-3L reads
 * before the rest are compacted for the 2^(L+1) presence gathers), bit 7 =
 * the sets the two-level rules leave to the walk compacted once more before
 * the rest of their gathers (round 6).  1 and 65 are one-pass (every set
 * decided in its lane).  All variants store identical lists.
 * "walk_bucket" (0 or 1; default 1, round 6): the layer-5 and layer-6 walk
 * launches of the two-pass variants with subset maxima (113, 241) walk their
 * queue sorted by walk key (which of the walk's first-level nodes a set may
 * expand): sets with one key share more of their union walk (C3 layer 6
 * without variable 0: its longest wave 811 -> ~465 union points, the
 * launch's union points 3x fewer).  Identical lists either way.
 * "walk_small_sets" (>= 0, default 200000): a layer-6 launch of fewer sets
 * walks one set per lane instead of four (the small launches of 4- and
 * 8-rank shares end with their longest walk wave; walk_bucket 0 only).
 * "walk_k6" (1, 2, 4 or 8; default 4): sets per lane of the other layer-6
 * walk launches: more sets share one walk of their union tree (less work per
 * set, longer waves).  4 gives the shortest single call; with several calls
 * in flight on one GPU (bench.py's slots) 8 gives the most sets per second
 * (C3: 10.17e9 against 9.80e9, single call 0.91 against 0.89 ms).
 * "table_budget_kb" (KiB; default 0 = half the free HBM): memory for the dense
 * best-score tables (16 B per entry incl. the host cost copy).  Lists whose
 * tables over all variables exceed it (e.g. n = 32 with a full skeleton) are
 * searched with tables built per skeleton component / triplet cluster, and
 * lookups outside the current tables scan the lists on the device -- same
 * answers, less memory.
 * "score_streams" (1..4, default 3): variable groups scored on concurrent
 * streams; "score_small_layers" (0..8, default 4): layers up to this size run
 * one one-pass launch per phase over all variables on one stream (they are
 * latency-bound), larger ones the two-pass form per group; "score_fused"
 * (0..4, default 3): layers up to this size (and up to score_small_layers)
 * run in ONE launch, a workgroup of 1024 threads per variable taking its
 * layers and phases in order with a barrier between them (score_variant 113
 * and 241 only, and not under time_limit_ms, whose budget is checked after every
 * layer; lists identical either way; C3 layers 1-3: 40 us against 54 us
 * for six launches, layer 4 in it 340 us: too many sets for one workgroup).
 * "score_unrank_lut" (0..2^31-1, default 2^20): the layer launches of 4 to 8
 * parents read each set's members from a table rank -> set of C(U, l) 32-bit
 * masks per (candidates U <= 32, members l), filled once per context the
 * first time a call needs it and shared by every variable, layer and call;
 * the value is the largest such table in entries, 0 = every lane computes
 * the mapping as before.  Lists and scores are bit-identical either way.
 * "score_lds_image" (0/1, default 1): every block of a layer launch (the
 * unfused layers up to 8 parents) fills its LDS constants -- Gram matrix,
 * binomials, work prefixes, unrank offsets, slab offsets, metadata, candidate
 * lists -- from one image per launch that the host packs in the LDS layout
 * (the Gram matrix from a host copy taken at ulg_cbic_load), in 16-byte
 * pieces whose loads are all in flight at once; 0 = from the separate arrays,
 * one loop each, as before.  The images are uploaded only when their bytes
 * change.  Lists and scores are bit-identical either way; ulg_get_info
 * "lds_image_bytes" reads the bytes of the last call's images.
 * "score_narrow" (0/1, default 1): a layer launch of 5 or 6 parents of the
 * default variant (241) whose every set mask, rank, launch-local index and
 * table slot fits 32 bits runs the narrow form of the layer kernel, which
 * carries them in 32-bit registers: every variable of the call has at most 32
 * candidates, the launch's sets plus one block fit 32 bits and the table has
 * fewer than 2^30 slots.  Any other launch, and every launch under 0, runs
 * the 64-bit kernel.  Lists and scores are bit-identical either way;
 * ulg_get_info "narrow_launches" counts the last call's narrow launches.
 * "disc_dense_cells" (1..32768, default 16384): a discrete set whose
 * contingency table has at most this many cells is counted in an int32 LDS
 * histogram; larger tables are counted in a hash table of their non-empty
 * cells (in LDS when 4N slots fit, else in a per-workgroup HBM slab).  Both
 * give bit-identical values.
 * "disc_prune" (0/1, default 0): ulg_disc_score drops every set that a kept
 * proper subset dominates (the reference's prune(); see ulg_disc_score).
 * "bge_prune" (0/1, default 0): the same pass for ulg_bge_score.
 * "posterior_keep" (0/1, default 0): ulg_posterior* keep every variable's
 * gamma table for ulg_posterior_table instead of reusing one (n - 1 more
 * tables of 2^(n-1) doubles); the outputs are bit-identical either way.
 * "linext_batch" (>= 0, default 0): ulg_dag_linear_extensions processes at
 * most this many DAGs per batch; 0 = as many as fit (the rule there).  The
 * counts are the same integers either way.
 * "dagfeat_grid" (0..65536, default 0): the workgroups (of four waves, a DAG
 * per wave at a time) of ulg_dag_features' launches; 0 = one per four DAGs,
 * at most 2048.  The tables are the same integers either way.
 * "mcmc_waves" (1, 2, 4 or 8; default 4): the waves of the workgroup that
 * runs one chain of ulg_order_mcmc_run; they share the positions a move
 * affects.  "mcmc_launch_steps" (>= 1, default 4096): the steps one launch of
 * it runs at most; the host loops launches over the chains' device state, so
 * no launch is unbounded.  Neither changes a bit of any output.
 * "edges_grid" (0..65536, default 0): the workgroups (of four waves, an
 * (order, position) pair per wave at a time) of ulg_order_edges' launches;
 * 0 = one per four pairs, at most 65536.  The tables are the same integers
 * either way.
 * "time_limit_ms" (default 0 = none): the reference's -r running-time budget
 * (score: per calculateScores call, score_calculator.cpp:33-52,78,91; astar:
 * a watchdog over the search, astar_main.cpp:135-138,266,696-706).  The GPU
 * scorer checks it after every complete layer (it synchronises the scoring
 * streams there, so only set it when a budget is wanted) and keeps the layers
 * finished so far -- the reference stops mid-layer, at a point that depends
 * on its clock; the exact-order A* checks it every 4096 pops and stops
 * without a goal for that component, as the reference's loop does.
 * "sweep_table" (0/1, default 1): the GPU search (ULG_ASTAR_GPU) on a
 * component without a skeleton filter first lays the component's successor
 * costs out in its own (variable, layer, colex) order (m 2^(m-1) floats,
 * cached until the tables change) when that fits the free HBM; 0 reads the
 * binary-indexed lattice per predecessor instead; 2 uses the slices with
 * 64-bit index arithmetic (1 = 32-bit).
 * "wide_prune" (0/1, default 1): the wide-layer walks skip absent nodes
 * below which no present key reaches -ts (hi-cover tables per variable);
 * "wide_reduced" (0/1, default 1): they skip the recursion's re-tests that
 * cannot change its state (each expanded node costs O(m) tests, not O(m^2));
 * "wide_lds" (0/1/2, default 1): walks longer than 2^6 steps are replayed by
 * one workgroup each with their skip / hi bitsets in LDS (2^q <= 2^20 local
 * subsets; the hi bitset in HBM above 2^19); 2 replays every walk that way.
 * "wide_pool" (0/1/2, default 2): with score_streams > 1 the wide layers run
 * variable by variable on score_streams host threads, largest candidate set
 * first (0: every group's part of a layer together, the slowest group
 * holding the next layer; 1: always by variable; 2: by variable when the
 * wide variables' candidate counts span at least 2).
 * "wide_host" (iterations, default 1024, 0 = never): an LDS replay still
 * walking after that many iterations stops and is replayed from the start on
 * a host thread over the same bitsets (one wave issues at most one
 * instruction every 4 cycles; a host core runs the same sequential walk tens
 * of times faster); "wide_host_max" (default 4096): only launches of at
 * most this many LDS replays hand over; "wide_host_first" (default 0): launches
 * of at most this many replays go to the host whole, without the LDS phase;
 * "wide_host_q" (0..32, default 0 = off): ... as do launches of at most 128
 * replays whose local bits q reach this; "wide_host_threads" (1..64,
 * default 16): host threads for those replays.
 * All variants compute identical results; the knob exists for A/B timing. */
int ulg_set_option(ulg_ctx *ctx, const char *name, int64_t value);
/* Read-back.  Every option name of ulg_set_option gives that option as it
 * stands (its default, or the last value a ulg_set_option accepted).
 * "device_bytes_live" / "pinned_bytes_live": the bytes of device memory and
 * of pinned host memory that the library's buffers hold at this moment --
 * process-wide, every live context's together, the asking one's included; a
 * destroyed context has given all of its bytes back (the exact search's
 * host row table, an anonymous mapping, is not counted).
 * Per-call state: "out_of_time" (1 if the last ulg_cbic_score,
 * ulg_astar* or ulg_triplet_astar ran out of time_limit_ms), "highest_completed_layer" (the
 * reference's ScoreCalculator::highestCompletedLayer of the last scoring call,
 * score_calculator.h:45), "exact_cycles" / "exact_instructions" /
 * "exact_cache_misses" (the last exact-order A*'s user-space host counters on
 * the calling thread, perf_event_open; -1 where the host does not grant
 * them), "disc_dense_sets" / "disc_sparse_sets" (sets of the last ulg_disc_score
 * counted on each path), "disc_pruned" (sets its prune pass removed, option
 * "disc_prune"), "bge_pruned" (likewise for the last ulg_bge_score, option
 * "bge_prune"), "fnml_table_bytes" (the ULG_SCORE_FNML regret table of the
 * loaded data; 0 until an fNML call builds it and after every load),
 * "disc_mmpc_tests" / "disc_mmpc_skipped" (G^2 tests the last
 * ulg_disc_mmpc performed / left out by its reliability rule),
 * "posterior_bytes" (the device bytes of the last successful ulg_posterior*
 * call's tables, by the formula there; 0 before any),
 * "linext_batches" (batches the last ulg_dag_linear_extensions ran, option
 * "linext_batch"),
 * "dagfeat_grid" (the workgroups the last ulg_dag_features launched, 0 when
 * it launched nothing: under this one name the read-back is the last call's
 * grid, not the option of the same name that asks for it),
 * "edges_grid" (likewise the workgroups the last ulg_order_edges launched, 0
 * when it launched nothing),
 * "unrank_lut_entries" (entries of the unrank tables the context holds),
 * "lds_image_bytes" (bytes of the last scoring call's launch images),
 * "narrow_launches" (layer launches of the last ulg_cbic_score that ran the
 * narrow form, option "score_narrow"),
 * "score_graph_captures" (scoring calls of the context that captured a launch
 * graph anew, option "score_graph"; a call that replays the held graph does
 * not count),
 * "score_error_word" (the last scoring call's device error word: 0,
 * or bit 0 a wide walk over its cap, bit 1 a walk-queue segment overflow,
 * bit 2 a walk entry naming a slot past the call's table -- any nonzero
 * word also made that call return a nonzero status). */
int ulg_get_info(ulg_ctx *ctx, const char *name, int64_t *value);

/* ---- profiling (per-kernel HIP-event timing on the context stream) ---- */
int ulg_profile_enable(ulg_ctx *ctx, int on);
/* Average duration (ms) and launch count of kernels whose name matches
 * `name` exactly, since the last reset.  Returns ULG_ERR_ARG if none. */
int ulg_profile_get(ulg_ctx *ctx, const char *name, double *avg_ms,
                    int64_t *count, double *total_ms);
/* Writes a newline-separated "name count total_ms" listing into buf. */
int ulg_profile_dump(ulg_ctx *ctx, char *buf, int64_t cap);
int ulg_profile_reset(ulg_ctx *ctx);
/* Time only the kernels named in the comma-separated list (NULL or "" = all):
 * each timed kernel costs two event records on the host, which the small
 * launches of a scoring call notice. */
int ulg_profile_select(ulg_ctx *ctx, const char *names);

/* ---- diagnostics (tests only; no reference counterpart) ---- */
/* One host pattern-database build in the form the triplet look-ahead pool
 * uses (StaticPatternDatabase, static_pattern_database.cpp:82-247, over
 * `cluster`), with the pool's cancel flag preset when cancel_preset != 0.
 * out[4]: built, cancelled, entries built, entries equal to the device PDB's. */
int ulg_diag_pdb_host(ulg_ctx *ctx, uint64_t cluster, int pd_count, int cancel_preset, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif
