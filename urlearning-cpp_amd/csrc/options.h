// options.h -- the context's options (ulg_set_option): one struct that holds
// them with their defaults, one table that names them and says what each
// accepts.  Host-only.  A new option is a member of Options and a row of
// kOptionRows; ulg_set_option and ulg_get_info pick it up from there.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

namespace ulg {

constexpr int64_t kLutDefaultCap = 1 << 20;  // entries of the largest unrank table (profiles/r15/README.md)
constexpr uint64_t kLutMaxTotal = 0x7fffffffull;  // unrank table offsets are int32, -1 = none

struct Options {
    // ---- cBIC scorer ----
    int64_t score_streams = 3;       // scorer variable groups on concurrent streams
    int64_t score_small_layers = 4;  // layers <= this run one-pass on one stream (two-pass variants)
    int64_t score_fused = 3;         // ... and layers <= this (<= small layers) in one launch, a workgroup per variable
    int64_t score_unrank_lut = kLutDefaultCap;  // largest unrank table in entries (score_plan.h LutCache), 0: none
    int64_t score_lds_image = 1;     // the layer launches fill LDS from a packed image (score_plan.h build_images)
    int64_t score_narrow = 1;        // layer launches whose every mask fits 32 bits run the narrow kernels (score_plan.h narrow_fits)
    int64_t score_variant = 241;
    int64_t score_graph = 1;         // scoring call: replay the captured launch sequence
    int64_t score_xcd = 1;           // scoring kernels: contiguous runs of sets per XCD
    int64_t walk_k6 = 4;             // sets per lane of the layer-6 walk launches (1, 2, 4 or 8)
    int64_t walk_bucket = 1;         // layers 5, 6: walk the queue sorted by walk key (walk_bucket_kernel)
    int64_t walk_small_sets = 200000;  // layer-6 launches below this many sets walk one set per lane
    int64_t wide_host_iters = 1024;  // "wide_host": LDS replays past this many iterations finish on host threads (0: never)
    int64_t wide_host_max = 4096;    // ... in launches of at most this many LDS replays
    int64_t wide_host_first = 0;     // launches of at most this many replays go to the host whole
    int64_t wide_host_q = 0;         // ... as do launches of <= 128 replays with q >= this (0: off)
    int64_t wide_host_threads = 16;  // host threads per wide-layer launch for those replays
    int64_t wide_pool = 2;           // wide layers variable by variable on score_streams host threads (2: auto)
    int64_t wide_lds = 1;            // wide walks: long ones replayed with their bitsets in LDS
    int64_t wide_reduced = 1;        // wide walks: skip the recursion's no-op re-tests
    int64_t wide_prune = 1;          // wide walks: skip absent nodes whose subsets hold no key >= -ts
    // ---- search ----
    int64_t sweep_xcd = 1;           // GPU sweep launches: contiguous runs of nodes per XCD
    int64_t sweep_table = 1;         // GPU sweep: successor costs in the sweep's (layer, colex) order
    int64_t time_limit_ms = 0;       // -r: wall-clock budget per scoring call / search (0 = none)
    int64_t table_budget_kb = 0;     // best-score table budget in KiB (0 = half the free HBM)
    // ---- discrete scorer ----
    int64_t disc_dense_cells = 16384;  // tables up to this many cells are counted in LDS
    int64_t disc_prune = 0;          // ulg_disc_score: drop dominated sets (the reference's prune())
    // ---- BGe scorer ----
    int64_t bge_prune = 0;           // ulg_bge_score: the same pass over the BGe slot table
    // ---- exact model averaging ----
    int64_t posterior_keep = 0;      // ulg_posterior*: keep every variable's gamma table for ulg_posterior_table
    // ---- linear extensions ----
    int64_t linext_batch = 0;        // ulg_dag_linear_extensions: at most this many DAGs per batch (0: as many as fit)
    // ---- structural features ----
    int64_t dagfeat_grid = 0;        // ulg_dag_features: workgroups of its launches (0: the default rule)
    // ---- order MCMC ----
    int64_t mcmc_waves = 4;          // ulg_order_mcmc_run: waves of the workgroup that runs one chain
    int64_t mcmc_launch_steps = 4096;  // ... and the steps of one launch at most
    int64_t edges_grid = 0;          // ulg_order_edges: workgroups of its launches (0: the default rule)
};

// What an option accepts: lo..hi, or (nlist > 0) one of list[0 .. nlist).
struct OptionRow {
    const char *name;
    int64_t Options::*field;
    int64_t lo, hi;
    int nlist;
    int64_t list[5];
    const char *text;  // the refusal reads "<name> must be <text>"
};

constexpr int64_t kOptMax = INT64_MAX;
constexpr OptionRow kOptionRows[] = {
    {"score_streams", &Options::score_streams, 1, 4, 0, {}, "1..4"},
    {"score_small_layers", &Options::score_small_layers, 0, 8, 0, {}, "0..8"},  // ULG_UNROLLED_PARENTS_GPU
    {"score_fused", &Options::score_fused, 0, 4, 0, {}, "0..4"},
    {"score_unrank_lut", &Options::score_unrank_lut, 0, (int64_t)kLutMaxTotal, 0, {}, "0..2^31-1"},
    {"score_lds_image", &Options::score_lds_image, 0, 1, 0, {}, "0 or 1"},
    {"score_narrow", &Options::score_narrow, 0, 1, 0, {}, "0 or 1"},
    {"score_variant", &Options::score_variant, 0, 0, 5, {1, 49, 65, 113, 241}, "1, 49, 65, 113 or 241"},
    {"score_graph", &Options::score_graph, 0, 1, 0, {}, "0 or 1"},
    {"score_xcd", &Options::score_xcd, 0, 1, 0, {}, "0 or 1"},
    {"sweep_xcd", &Options::sweep_xcd, 0, 1, 0, {}, "0 or 1"},
    {"sweep_table", &Options::sweep_table, 0, 2, 0, {}, "0, 1 or 2"},
    {"time_limit_ms", &Options::time_limit_ms, 0, kOptMax, 0, {}, ">= 0"},
    {"table_budget_kb", &Options::table_budget_kb, 0, kOptMax, 0, {}, ">= 0"},
    {"walk_k6", &Options::walk_k6, 0, 0, 4, {1, 2, 4, 8}, "1, 2, 4 or 8"},
    {"walk_bucket", &Options::walk_bucket, 0, 1, 0, {}, "0 or 1"},
    {"walk_small_sets", &Options::walk_small_sets, 0, kOptMax, 0, {}, ">= 0"},
    {"wide_host", &Options::wide_host_iters, 0, kOptMax, 0, {}, ">= 0"},
    {"wide_host_max", &Options::wide_host_max, 0, kOptMax, 0, {}, ">= 0"},
    {"wide_host_first", &Options::wide_host_first, 0, kOptMax, 0, {}, ">= 0"},
    {"wide_host_q", &Options::wide_host_q, 0, 32, 0, {}, "0..32"},
    {"wide_host_threads", &Options::wide_host_threads, 1, 64, 0, {}, "1..64"},
    {"wide_pool", &Options::wide_pool, 0, 2, 0, {}, "0, 1 or 2"},
    {"wide_lds", &Options::wide_lds, 0, 2, 0, {}, "0, 1 or 2"},
    {"wide_reduced", &Options::wide_reduced, 0, 1, 0, {}, "0 or 1"},
    {"wide_prune", &Options::wide_prune, 0, 1, 0, {}, "0 or 1"},
    {"disc_dense_cells", &Options::disc_dense_cells, 1, 32768, 0, {}, "1..32768"},
    {"disc_prune", &Options::disc_prune, 0, 1, 0, {}, "0 or 1"},
    {"bge_prune", &Options::bge_prune, 0, 1, 0, {}, "0 or 1"},
    {"posterior_keep", &Options::posterior_keep, 0, 1, 0, {}, "0 or 1"},
    {"linext_batch", &Options::linext_batch, 0, kOptMax, 0, {}, ">= 0"},
    {"dagfeat_grid", &Options::dagfeat_grid, 0, 65536, 0, {}, "0..65536"},
    {"mcmc_waves", &Options::mcmc_waves, 0, 0, 4, {1, 2, 4, 8}, "1, 2, 4 or 8"},
    {"mcmc_launch_steps", &Options::mcmc_launch_steps, 1, kOptMax, 0, {}, ">= 1"},
    {"edges_grid", &Options::edges_grid, 0, 65536, 0, {}, "0..65536"},
};

inline const OptionRow *option_row(const char *name) {
    for (const OptionRow &r : kOptionRows)
        if (std::strcmp(r.name, name) == 0) return &r;
    return nullptr;
}

// false, with *err set, for an unknown name or a value the row refuses
inline bool options_set(Options &o, const char *name, int64_t value, std::string *err) {
    const OptionRow *r = option_row(name);
    if (!r) {
        if (err) *err = std::string("unknown option: ") + name;
        return false;
    }
    bool ok = r->nlist == 0 && value >= r->lo && value <= r->hi;
    for (int i = 0; i < r->nlist; ++i) ok = ok || value == r->list[i];
    if (!ok) {
        if (err) *err = std::string(r->name) + " must be " + r->text;
        return false;
    }
    o.*r->field = value;
    return true;
}

inline bool options_get(const Options &o, const char *name, int64_t *value) {
    const OptionRow *r = option_row(name);
    if (r) *value = o.*r->field;
    return r != nullptr;
}

}  // namespace ulg
