// mmpc -- writes the skeleton file the reference's score / astar /
// triplet_astar take with -k (README.md:16 expects it from an MMPC run
// outside the package; format read by Skeleton::read_matrix_file,
// base/skeleton.cpp:19-105): an n x n 0/1 matrix, row i column j = 1 iff
// edge i-j.  The data go through the same loader as `score` (mlpack/Armadillo
// csv semantics), the Gram matrix is built on the GPU (MFMA f64) and every
// Fisher-z test runs on the GPU (ulg_mmpc).
//
//   mmpc <in.csv> <skeleton.csv> [--alpha 0.05] [--max-cond K] [--diagonal]
//
// --discrete reads the file as `score -f BIC` does (load_discrete_csv, with
// -s / -d as there) and runs MMPC with G^2 tests on the value codes
// (ulg_disc_mmpc; --min-per-cell is its reliability rule):
//
//   mmpc --discrete -s <in.csv> <skeleton.csv> [--alpha 0.05] [--max-cond K] [--min-per-cell 5]
//
// --diagonal also sets the diagonal, as the README's all-ones example does
// (it changes triplet_astar's degenerate triples, tests/golden/README.md).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/ulg.h"
#include "cli_common.h"
#include "io.h"

static bool write_skeleton(const ulgcli::Args &args, const std::vector<uint64_t> &rows, int n, int &edges) {
    std::string text;
    edges = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const bool e = ((rows[i] >> j) & 1ull) || (i == j && args.has("diagonal"));
            edges += (j > i) && ((rows[i] >> j) & 1ull);
            text += e ? '1' : '0';
            text += (j == n - 1) ? '\n' : ',';
        }
    if (!ulgio::write_text(args.get("output"), text)) {
        std::fprintf(stderr, "mmpc: cannot write '%s'\n", args.get("output").c_str());
        return false;
    }
    return true;
}

// --discrete: the value codes of `score -f BIC`, G^2 tests (ulg_disc_mmpc)
static int discrete_main(const ulgcli::Args &args, double alpha, int max_cond) {
    const int min_per_cell = std::atoi(args.get("min-per-cell").c_str());
    if (min_per_cell < 1) {
        std::fprintf(stderr, "mmpc: --min-per-cell must be at least 1\n");
        return 2;
    }
    if (!(alpha > 0.0 && alpha < 1.0)) {
        std::fprintf(stderr, "mmpc: --alpha must lie in (0, 1)\n");
        return 2;
    }
    const char delim = args.get("delimiter").empty() ? ',' : args.get("delimiter")[0];
    ulgio::DiscreteData dd;
    std::string derr;
    if (!ulgio::load_discrete_csv(args.get("input"), delim, args.has("hasHeader"), dd, derr)) {
        std::fprintf(stderr, "mmpc: %s\n", derr.c_str());
        return 1;
    }
    const int n = (int)dd.names.size();
    const int64_t N = dd.num_records;
    if (n < 1 || n > 63 || N < 2) {
        std::fprintf(stderr, "mmpc: '%s' must have 1..63 columns and at least 2 records\n", args.get("input").c_str());
        return 1;
    }
    const int dev = std::atoi(args.get("device").c_str());
    ulg_ctx *ctx = nullptr;
    if (ulg_create(&dev, 1, &ctx) != ULG_OK) {
        std::fprintf(stderr, "mmpc: no usable HIP device %d\n", dev);
        return 1;
    }
    const double t0 = ulgcli::now_s();
    std::vector<uint64_t> rows(n, 0);
    int rc = ulg_disc_load(ctx, dd.codes.data(), N, n, dd.arity.data());
    if (rc == ULG_OK) rc = ulg_disc_mmpc(ctx, alpha, max_cond, min_per_cell, rows.data());
    const double t1 = ulgcli::now_s();
    if (rc != ULG_OK) {
        std::fprintf(stderr, "mmpc: %s\n", ulg_last_error(ctx));
        ulg_destroy(ctx);
        return 1;
    }
    int64_t tests = 0, skipped = 0;
    ulg_get_info(ctx, "disc_mmpc_tests", &tests);
    ulg_get_info(ctx, "disc_mmpc_skipped", &skipped);
    ulg_destroy(ctx);
    int edges = 0;
    if (!write_skeleton(args, rows, n, edges)) return 1;
    std::printf("MMPC (MI355X): n=%d N=%lld alpha=%g edges=%d, G^2 tests %lld (skipped %lld), upload + tests %.3f s\n", n,
                (long long)N, alpha, edges, (long long)tests, (long long)skipped, t1 - t0);
    return 0;
}

int main(int argc, char **argv) {
    ulgcli::Args args(
        {
            {"", "alpha", true, "0.05", "Significance level of the Fisher-z tests"},
            {"", "max-cond", true, "-1", "Largest conditioning set (-1: no cap below 24)"},
            {"", "diagonal", false, "", "Set the diagonal of the skeleton matrix"},
            {"", "discrete", false, "", "Discrete data: G^2 tests on the value codes instead of Fisher-z"},
            {"s", "hasHeader", false, "", "With --discrete: the first line of the input file gives the variable names."},
            {"d", "delimiter", true, ",", "With --discrete: the delimiter of the input file."},
            {"", "min-per-cell", true, "5", "With --discrete: a test needs this many records per table cell"},
            {"", "device", true, "0", "HIP device to use."},
            {"h", "help", false, "", "Show this help message."},
        },
        {"input", "output"});
    std::string err;
    if (!args.parse(argc, argv, err)) {
        std::fprintf(stderr, "mmpc: %s\n", err.c_str());
        return 2;
    }
    if (args.has("help") || argc == 1 || !args.has("input") || !args.has("output")) {
        args.usage(argv[0], "MMPC skeleton for the score/astar/triplet_astar -k option.  Example usage: mmpc data.csv skeleton.csv");
        return args.has("help") || argc == 1 ? 0 : 2;
    }
    const double alpha = std::atof(args.get("alpha").c_str());
    const int max_cond = std::atoi(args.get("max-cond").c_str());
    const bool discrete = args.has("discrete");
    if (!discrete && (args.has("hasHeader") || args.has("delimiter") || args.has("min-per-cell"))) {
        std::fprintf(stderr, "mmpc: -s, -d and --min-per-cell belong to --discrete\n");
        return 2;
    }
    if (discrete) return discrete_main(args, alpha, max_cond);
    std::vector<double> data;
    int64_t N = 0;
    int n = 0;
    if (!ulgio::load_numeric_csv(args.get("input"), data, N, n) || n < 1 || n > 63) {
        std::fprintf(stderr, "mmpc: cannot load '%s' (1..63 columns)\n", args.get("input").c_str());
        return 1;
    }
    const int dev = std::atoi(args.get("device").c_str());
    ulg_ctx *ctx = nullptr;
    if (ulg_create(&dev, 1, &ctx) != ULG_OK) {
        std::fprintf(stderr, "mmpc: no usable HIP device %d\n", dev);
        return 1;
    }
    const double t0 = ulgcli::now_s();
    std::vector<uint64_t> rows(n, 0);
    int rc = ulg_cbic_load(ctx, data.data(), N, n, 0.0);
    if (rc == ULG_OK) rc = ulg_mmpc(ctx, alpha, max_cond, rows.data());
    const double t1 = ulgcli::now_s();
    if (rc != ULG_OK) {
        std::fprintf(stderr, "mmpc: %s\n", ulg_last_error(ctx));
        ulg_destroy(ctx);
        return 1;
    }
    ulg_destroy(ctx);
    int edges = 0;
    if (!write_skeleton(args, rows, n, edges)) return 1;
    std::printf("MMPC (MI355X): n=%d N=%lld alpha=%g edges=%d, Gram + tests %.3f s\n", n, (long long)N, alpha, edges,
                t1 - t0);
    return 0;
}
