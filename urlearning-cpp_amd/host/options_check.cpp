// options_check -- the option table of csrc/options.h against a record of
// what ulg_set_option accepted, refused and defaulted to before the table
// existed.  The record below is data of this program: it was read from the 26
// hand-written blocks the table replaced and is not derived from the table
// (score_narrow, bge_prune, posterior_keep, linext_batch, dagfeat_grid,
// mcmc_waves, mcmc_launch_steps and edges_grid, added since, are recorded the
// same way).
// Built with AddressSanitizer + UBSan by `make sanitize` (tests/test_sanitize.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/options.h"

using namespace ulg;

namespace {

long g_checks = 0;
const char *g_case = "";

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        ++g_checks;                                                                                         \
        if (!(cond)) {                                                                                      \
            std::fprintf(stderr, "options_check: %s:%d: %s fails for %s\n", __FILE__, __LINE__, #cond, g_case); \
            std::exit(1);                                                                                   \
        }                                                                                                   \
    } while (0)

constexpr int64_t kNoMax = INT64_MAX;  // ">= 0": no upper bound

struct Want {
    const char *name;
    std::vector<int64_t> list;  // accepted values; empty: lo..hi
    int64_t lo, hi;
    int64_t def;
    const char *text;  // "<name> must be <text>"
};

const std::vector<Want> kWant = {
    {"score_streams", {}, 1, 4, 3, "1..4"},
    {"score_small_layers", {}, 0, 8, 4, "0..8"},
    {"score_fused", {}, 0, 4, 3, "0..4"},
    {"score_unrank_lut", {}, 0, 2147483647, 1 << 20, "0..2^31-1"},
    {"score_lds_image", {0, 1}, 0, 0, 1, "0 or 1"},
    {"score_narrow", {0, 1}, 0, 0, 1, "0 or 1"},
    {"score_variant", {1, 49, 65, 113, 241}, 0, 0, 241, "1, 49, 65, 113 or 241"},
    {"score_graph", {0, 1}, 0, 0, 1, "0 or 1"},
    {"score_xcd", {0, 1}, 0, 0, 1, "0 or 1"},
    {"sweep_xcd", {0, 1}, 0, 0, 1, "0 or 1"},
    {"sweep_table", {}, 0, 2, 1, "0, 1 or 2"},
    {"time_limit_ms", {}, 0, kNoMax, 0, ">= 0"},
    {"table_budget_kb", {}, 0, kNoMax, 0, ">= 0"},
    {"walk_k6", {1, 2, 4, 8}, 0, 0, 4, "1, 2, 4 or 8"},
    {"walk_bucket", {0, 1}, 0, 0, 1, "0 or 1"},
    {"walk_small_sets", {}, 0, kNoMax, 200000, ">= 0"},
    {"wide_host", {}, 0, kNoMax, 1024, ">= 0"},
    {"wide_host_max", {}, 0, kNoMax, 4096, ">= 0"},
    {"wide_host_first", {}, 0, kNoMax, 0, ">= 0"},
    {"wide_host_q", {}, 0, 32, 0, "0..32"},
    {"wide_host_threads", {}, 1, 64, 16, "1..64"},
    {"wide_pool", {}, 0, 2, 2, "0, 1 or 2"},
    {"wide_lds", {}, 0, 2, 1, "0, 1 or 2"},
    {"wide_reduced", {0, 1}, 0, 0, 1, "0 or 1"},
    {"wide_prune", {0, 1}, 0, 0, 1, "0 or 1"},
    {"disc_dense_cells", {}, 1, 32768, 16384, "1..32768"},
    {"disc_prune", {0, 1}, 0, 0, 0, "0 or 1"},
    {"bge_prune", {0, 1}, 0, 0, 0, "0 or 1"},
    {"posterior_keep", {0, 1}, 0, 0, 0, "0 or 1"},
    {"linext_batch", {}, 0, kNoMax, 0, ">= 0"},
    {"dagfeat_grid", {}, 0, 65536, 0, "0..65536"},
    {"mcmc_waves", {1, 2, 4, 8}, 0, 0, 4, "1, 2, 4 or 8"},
    {"mcmc_launch_steps", {}, 1, kNoMax, 4096, ">= 1"},
    {"edges_grid", {}, 0, 65536, 0, "0..65536"},
};

bool accepted(const Want &w, int64_t v) {
    if (w.list.empty()) return v >= w.lo && v <= w.hi;
    for (int64_t x : w.list)
        if (x == v) return true;
    return false;
}

// the value is refused with the exact message and nothing changes
void check_refused(const Want &w, int64_t v) {
    Options o;
    int64_t before = -1, after = -1;
    std::string err;
    CHECK(options_get(o, w.name, &before));
    CHECK(!options_set(o, w.name, v, &err));
    CHECK(err == std::string(w.name) + " must be " + w.text);
    CHECK(options_get(o, w.name, &after) && after == before);
    CHECK(!options_set(o, w.name, v, nullptr));  // the message is optional
}

// the value is accepted, reads back, and no other option moves
void check_accepted(const Want &w, int64_t v) {
    Options o;
    std::string err = "untouched";
    int64_t got = -1;
    CHECK(options_set(o, w.name, v, &err) && err == "untouched");
    CHECK(options_get(o, w.name, &got) && got == v);
    for (const Want &other : kWant)
        if (std::strcmp(other.name, w.name) != 0) CHECK(options_get(o, other.name, &got) && got == other.def);
}

}  // namespace

int main() {
    CHECK(kWant.size() == 34);
    CHECK(sizeof(kOptionRows) / sizeof(kOptionRows[0]) == kWant.size());
    CHECK(sizeof(Options) == kWant.size() * sizeof(int64_t));  // one member per option, nothing else
    // names: unique on both sides, and the same ones
    for (size_t i = 0; i < kWant.size(); ++i) {
        g_case = kWant[i].name;
        int in_table = 0;
        for (const OptionRow &r : kOptionRows) in_table += std::strcmp(r.name, kWant[i].name) == 0;
        CHECK(in_table == 1);
        for (size_t j = i + 1; j < kWant.size(); ++j) CHECK(std::strcmp(kWant[i].name, kWant[j].name) != 0);
    }
    // no two rows share a member
    for (const OptionRow &a : kOptionRows)
        for (const OptionRow &b : kOptionRows) {
            g_case = a.name;
            CHECK(&a == &b || a.field != b.field);
        }
    for (const Want &w : kWant) {
        g_case = w.name;
        Options o;
        int64_t got = -1;
        CHECK(options_get(o, w.name, &got) && got == w.def);
        CHECK(accepted(w, w.def));
        const bool bounded = !w.list.empty() || w.hi != kNoMax;
        if (w.list.empty()) {
            check_accepted(w, w.lo);
            check_refused(w, w.lo - 1);
            if (bounded) {
                check_accepted(w, w.hi);
                check_refused(w, w.hi + 1);
                check_accepted(w, w.lo + (w.hi - w.lo) / 2);
            } else {
                check_accepted(w, kNoMax);
                check_accepted(w, (1ll << 32) + 1);
            }
        } else {
            for (int64_t v : w.list) check_accepted(w, v);
            check_refused(w, w.list.front() - 1);
            check_refused(w, w.list.back() + 1);
            // every value in a gap between two listed ones
            for (int64_t v = w.list.front(); v < w.list.back(); ++v)
                if (!accepted(w, v)) check_refused(w, v);
        }
        check_refused(w, -1);
        check_refused(w, INT64_MIN);
        if (bounded) {
            // no silent narrowing: these are 1 and 0 as 32-bit values
            check_refused(w, (1ll << 32) + 1);
            check_refused(w, 1ll << 32);
            check_refused(w, kNoMax);
        }
    }
    g_case = "score_variant / walk_k6";
    check_refused(kWant[6], 2);
    check_refused(kWant[13], 3);
    // an unknown name
    g_case = "unknown";
    {
        Options o;
        std::string err;
        int64_t got = 77;
        CHECK(!options_set(o, "no_such_option", 1, &err) && err == "unknown option: no_such_option");
        CHECK(!options_set(o, "", 1, &err) && err == "unknown option: ");
        CHECK(!options_set(o, "wide_host_iters", 1, &err) && err == "unknown option: wide_host_iters");  // the field's name
        CHECK(!options_get(o, "no_such_option", &got) && got == 77);
        CHECK(!options_get(o, "out_of_time", &got) && got == 77);  // an info name, not an option
    }
    std::printf("options_check ok: %ld checks\n", g_checks);
    return 0;
}
