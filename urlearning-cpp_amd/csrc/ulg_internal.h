// ulg_internal.h -- shared host-side state of the MI355X URLearning path.
#pragma once

#include <mutex>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <cstring>
#include <set>
#include <vector>

#include "../../include/ulg.h"
#include "bge.h"         // BgeConsts
#include "dev_buf.h"     // DevBuf, PinnedBuf, ensure, upload, Mirror
#include "options.h"     // Options
#include "score_plan.h"  // kMaxVars, kMaxL, kWideMax, kBinomK, binom64, ScoreLists, CbicPlan

namespace ulg {

constexpr uint32_t kAbsentBits = 0xFFFFFFFFu;  // "not in the FloatMap" sentinel (a NaN payload)

struct SearchState;
struct PssState;
struct PosteriorState;
struct OrderMcmcState;

struct ProfRec {
    std::string name;
    hipEvent_t start, stop;
    bool graph = false;  // recorded by a captured graph (its events stay with the graph)
};

// The context's streams and events.  A base of ulg_ctx, so that they are
// destroyed after every member of it (~ulg_ctx, ulg_ctx.cpp).
struct CtxStreams {
    hipStream_t stream = nullptr;
    std::vector<hipStream_t> aux_streams;  // created on first use
    std::vector<hipEvent_t> sync_events;
    std::vector<hipEvent_t> event_pool;
    CtxStreams() = default;
    CtxStreams(const CtxStreams &) = delete;
    CtxStreams &operator=(const CtxStreams &) = delete;
    ~CtxStreams();
};

}  // namespace ulg

struct ulg_ctx : ulg::CtxStreams {
    int device = 0;
    std::string err;
    ulg::Options opt;  // ulg_set_option (options.h)
    ~ulg_ctx();

    // ---- data (BIC_OLS ctor) ----
    int n = 0;
    int64_t N = 0;
    int npad = 0;
    double lambda = 0.0;
    bool loaded = false;
    ulg::DevBuf<double> raw, z, gram, partials, colstat;
    // lambda ln(N) as the device computes it (penalty_kernel at ulg_cbic_load):
    // the BIC penalty per parent, passed to every scoring kernel
    double pen = 0.0;
    ulg::DevBuf<double> d_pen;

    // ---- scoring state ----
    ulg::ScoreLists lists;  // the scoring call being prepared (published into the fields below when it is launched)
    ulg::CbicPlan plan;     // ... and ulg_cbic_score's plan for it; both keep their vectors' capacity across calls
    int nv = 0;
    int kmax = 0;
    std::vector<int> vars;
    std::vector<int> m;           // candidate count per batch variable
    std::vector<uint64_t> tbl_off;  // [nv][kmax+2] flattened prefix of table slots
    int64_t total_slots = 0;
    int64_t total_stored = 0;
    int64_t total_scored = 0;
    bool scored = false;
    int out_of_time = 0;           // the last scoring call or search ran out of its budget
    int completed_layer = -1;      // highest fully scored layer of the last scoring call
    hipGraph_t graph = nullptr;    // the captured scoring launches, its instance, its key
    hipGraphExec_t gexec = nullptr;
    std::vector<uint64_t> gkey;
    std::vector<ulg::ProfRec> gprof;  // profiling events inside the graph
    ulg::DevBuf<float> table;
    ulg::DevBuf<float> d_hsub;    // score_variant bit 6: subset maxima, table layout
    // unrank tables (score_plan.h LutCache): the tables, the cache's index of
    // them, and the call's per-launch offsets
    ulg::LutCache lut_cache;
    ulg::DevBuf<uint32_t> d_lut;
    ulg::DevBuf<int32_t> d_lutoff;
    ulg::Mirror mir_lutoff;
    // launch images (score_plan.h CbicPlan::build_images): the layer launches'
    // LDS constants packed per launch, and the host copy of the Gram matrix
    // they are built from (taken at ulg_cbic_load, replaced by every load)
    std::vector<double> h_gram;
    ulg::DevBuf<unsigned char> d_image;
    ulg::Mirror mir_image;
    ulg::DevBuf<uint64_t> d_tbl_off, d_work, d_blk;
    ulg::DevBuf<uint8_t> d_cand;  // [nv][64] compact index -> variable
    ulg::DevBuf<int> d_meta;      // [nv][4]: var, m, var0in, pad
    ulg::DevBuf<uint32_t> d_binom;
    ulg::DevBuf<uint64_t> d_binom64;              // [64][64] unclamped C(a, b) for the wide layers
    ulg::DevBuf<uint64_t> d_wqueue;               // wide layers: sets left for the walk
    ulg::DevBuf<uint64_t> d_wbits;                // wide layers: per-walk checked bitsets
    ulg::DevBuf<unsigned long long> d_stats;      // wide walks: statistics (ULG_WALK_STATS diagnostics)
    ulg::DevBuf<uint64_t> d_dump;
    ulg::DevBuf<uint64_t> d_queue;                // score_variant bit 4: undecided lanes
    ulg::DevBuf<uint32_t> d_qaux, d_qsidx, d_qoffs;  // walk_bucket: key/rank, sorted index, key bases
    ulg::DevBuf<uint8_t> d_qkey;                            // walk_bucket: each queue entry's walk key
    ulg::DevBuf<unsigned long long> d_qseg;       // ... their per-segment counters (score_plan.h kSegBlocks)
    ulg::DevBuf<unsigned long long> d_qcount;
    ulg::DevBuf<uint64_t> d_workg;                // per stream-group work prefixes
    ulg::DevBuf<uint64_t> d_vwork;                // per-variable work prefixes of the wide-layer pool
    ulg::DevBuf<uint32_t> d_hq;                   // per stream group: replays handed to the host
    ulg::DevBuf<unsigned int> d_hqc;
    ulg::DevBuf<float> d_hmax;      // wide walks: hi-cover tables (subset max of the present keys), then the present keys
    uint64_t hmax_half = 0;         // entries of each half of d_hmax
    ulg::DevBuf<uint64_t> d_hoff;   // [nv] table offsets, ~0 = no table
    ulg::DevBuf<int> d_hmeta;       // per stream group: launch variables and tile / block prefixes
    ulg::DevBuf<unsigned long long> d_scount;  // per stream group: long wide walks handed to the LDS kernel
    ulg::PinnedBuf<unsigned long long> wide_pinned;  // pinned queue / long-walk counts of the wide stages
    std::vector<unsigned long long> wide_host;
    ulg::Mirror mir_tbl_off, mir_work, mir_cand, mir_meta, mir_workg, mir_hoff, mir_vwork, mir_cons;
    ulg::DevBuf<uint64_t> out_sets;
    ulg::DevBuf<float> out_scores;
    ulg::DevBuf<int64_t> out_offsets;
    // ulg_cbic_score_async: the stored count lands here when the launches
    // finish; ulg_cbic_score_finish (or any later scorer call) collects it
    ulg::PinnedBuf<unsigned long long> async_pinned;  // [stored count, error word] of the last call
    unsigned long long last_err_word = 0;        // the last scoring call's error word (kErr* bits)
    bool async_pending = false;
    int64_t graph_captures = 0;                  // scoring calls that captured a new graph (ulg_get_info)
    ulg::DevBuf<float> qbuf_in, qbuf_out;
    ulg::DevBuf<uint64_t> d_sets_in;              // ulg_cbic_score_sets: (variable, parent mask) pairs

    // ---- parent-set constraints (ulg_cbic_set_constraints) ----
    std::vector<int> cons_var;                    // one entry per alternative: its variable,
    std::vector<uint64_t> cons_req, cons_forb;    // required and forbidden parents (variable masks)
    ulg::DevBuf<uint64_t> d_cons_var;             // by variable, variable masks (ulg_cbic_score_sets)
    ulg::DevBuf<uint64_t> d_cons;                 // the scoring call's table: by call index, compact masks
    int cons_call_words = 0;                      // its words (0: the call runs the unconstrained kernels)

    // ---- discrete data and scorer (disc.hip) ----
    // The context holds discrete data iff disc_loaded && !loaded: ulg_cbic_load
    // sets `loaded`, ulg_disc_load clears it.
    bool disc_loaded = false;
    std::vector<int> disc_arity;                  // [n]
    int64_t disc_path_sets[2] = {0, 0};           // last ulg_disc_score: sets on the dense / sparse path
    ulg::DevBuf<uint8_t> d_codes;                 // [n][N] value codes, column-major
    ulg::DevBuf<uint64_t> d_disc_meta;            // slot prefixes [nv * S + 1], then item prefixes [S][nv + 1]
    ulg::DevBuf<uint8_t> d_disc_cand;             // [nv][64] compact index -> variable
    ulg::DevBuf<int> d_disc_vm;                   // [nv][2]: variable, candidate count
    ulg::DevBuf<float> d_disc_table;              // per table slot: the stored value, or absent
    ulg::DevBuf<unsigned long long> d_disc_blk;   // compaction: stored sets per block, then their prefix
    ulg::DevBuf<uint64_t> d_disc_sets;            // per table slot: the set's variable mask
    ulg::DevBuf<unsigned long long> d_disc_slab;  // sparse path: per-workgroup hash tables
    ulg::DevBuf<unsigned long long> d_disc_word;  // [error word, dense sets, sparse sets, stored, pruned]
    double disc_ess = 1.0;                        // ulg_disc_set_ess: BDeu's equivalent sample size (sticky)
    int64_t disc_pruned = 0;                      // sets the last ulg_disc_score's prune pass dropped
    ulg::DevBuf<float> d_disc_best;               // ... per table slot: the best kept score among the set and its subsets
    ulg::DevBuf<int32_t> d_disc_counts;           // ulg_disc_counts' table
    // ---- BGe (bge.hip): the continuous data's Bayesian score, over the slot table above ----
    double bge_alpha_mu = 1.0, bge_alpha_w = 0.0; // ulg_bge_set_prior (sticky; alpha_w 0 = n + alpha_mu + 1)
    ulg::BgeConsts bge_k;                         // the last call's t, c_l and A_l (the upload's source)
    ulg::DevBuf<double> d_bge_tab;                // [64]: c_l, A_l
    int64_t bge_pruned = 0;                       // sets the last ulg_bge_score's prune pass dropped
    // ---- discrete G^2 tests and MMPC (disc_mmpc.hip) ----
    ulg::DevBuf<uint64_t> d_g2_tests;             // per test: (x, t), conditioning mask
    ulg::DevBuf<unsigned long long> d_g2_out;     // per test: the fixed-point sum
    int64_t disc_mmpc_stat[2] = {0, 0};           // last ulg_disc_mmpc: tests performed / skipped

    // ---- search side (best-score tables, pattern database, A*) ----
    ulg::SearchState *search = nullptr;
    int64_t exact_pmu[3] = {-1, -1, -1};  // last exact A*: user-space cycles, instructions, cache misses (-1: n/a)

    // ---- .pss text formatting (pss.hip) ----
    ulg::PssState *pss = nullptr;

    // ---- exact model averaging (posterior.hip): its lists and tables, apart from everything above ----
    ulg::PosteriorState *posterior = nullptr;
    int64_t posterior_bytes = 0;  // ulg_get_info("posterior_bytes"): the last successful call's tables
    int64_t linext_batches = 0;   // ulg_get_info("linext_batches"): batches of the last ulg_dag_linear_extensions (linext.hip)
    int64_t dagfeat_grid = 0;     // ulg_get_info("dagfeat_grid"): workgroups of the last ulg_dag_features' first launch (dagfeat.hip)

    // ---- order MCMC (order_mcmc.hip): its lists and chains, apart from the model averaging's ----
    ulg::OrderMcmcState *mcmc = nullptr;
    int64_t edges_grid = 0;       // ulg_get_info("edges_grid"): workgroups the last ulg_order_edges launched (order_edges.hip)

    // ---- profiling ----
    bool prof = false;
    std::vector<ulg::ProfRec> pending;
    std::set<std::string> prof_only;  // ulg_profile_select: time only these kernels
    std::mutex mu;  // err / pending: the wide scoring layers use one host thread per stream group
    std::map<std::string, std::vector<double>> prof_ms;

    // ---- fNML (ULG_SCORE_FNML, disc.hip) ----
    // The regret table of the loaded discrete data, built by the first fNML
    // call after ulg_disc_load, dropped by every load (fnml_drop).
    ulg::DevBuf<long long> d_fnml;                // per distinct arity >= 2, ascending: fix(ln C(r, n)), n = 0 .. N
    ulg::DevBuf<double> d_fnml_c2;                // C(2, n), n = 0 .. 1000, from the host
    bool fnml_built = false;
    int64_t fnml_bytes = 0;                       // ulg_get_info("fnml_table_bytes")
};

namespace ulg {

// error helpers -----------------------------------------------------------
int set_err(ulg_ctx *c, int code, const std::string &msg);

#define ULG_HIP(ctx, expr)                                                          \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess)                                                       \
            return ::ulg::set_err((ctx), ULG_ERR_HIP,                               \
                                  std::string(#expr " failed: ") + hipGetErrorString(e_)); \
    } while (0)

// profiling: bracket a launch with events when enabled
void prof_begin(ulg_ctx *c, const char *name);
void prof_end(ulg_ctx *c);
void prof_begin_s(ulg_ctx *c, const char *name, hipStream_t stream);
void prof_end_s(ulg_ctx *c, hipStream_t stream);
void prof_collect(ulg_ctx *c);  // after a stream sync
void graph_reset(ulg_ctx *c);   // drop the captured scoring graph (cbic.hip)
void pss_delete(ulg_ctx *c);   // delete the context's PssState (pss.hip, where the type is complete)
void posterior_delete(ulg_ctx *c);  // ... and its PosteriorState (posterior.hip)
void order_mcmc_delete(ulg_ctx *c);  // ... and its OrderMcmcState (order_mcmc.hip)

// binomial table C(a, b), a < 64, b < kBinomK, clamped to uint32
const std::vector<uint32_t> &host_binom();
// C(a, b) for a, b < 64 (saturating at 2^64 - 1), [a * 64 + b]
const std::vector<uint64_t> &host_binom64();

// A load of either kind: the regret table of the previous records goes.
inline void fnml_drop(ulg_ctx *c) {
    c->d_fnml.reset();
    c->fnml_built = false;
    c->fnml_bytes = 0;
}

// An async scoring call's launches still own the buffers and the lists: every
// entry point that reads or replaces them collects that call first.
inline int finish_pending(ulg_ctx *c) {
    return c->async_pending ? ulg_cbic_score_finish(c, nullptr, nullptr) : ULG_OK;
}
// ScoreLists::build's refusal as the status and message of ABI function `who`
inline int lists_error(ulg_ctx *c, const char *who, ScoreLists::Status st) {
    return set_err(c, st == ScoreLists::kTooWide ? ULG_ERR_UNSUPPORTED : ULG_ERR_ARG,
                   std::string(who) + ScoreLists::status_text(st));
}
// A launched scoring call's lists become the context's (ulg_cbic_fetch, the
// search and the .pss writer read them); completed_layer names its last layer.
inline void publish(ulg_ctx *c, const ScoreLists &ls, int64_t stored, bool async_pending) {
    c->nv = ls.nv;
    c->kmax = ls.kmax;
    c->vars = ls.vars;
    c->m = ls.mv;
    c->tbl_off = ls.toff;
    c->total_slots = (int64_t)ls.total_slots;
    c->total_stored = stored;
    c->total_scored = ls.scored_up_to(c->completed_layer);
    c->scored = true;
    c->async_pending = async_pending;
}

}  // namespace ulg
