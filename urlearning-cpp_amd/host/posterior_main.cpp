// posterior -- exact model averaging over a .pss on the MI355X path
// (ulg_posterior, include/ulg.h): ln Z, the matrix of edge posteriors and the
// posterior of every stored parent set, under the order-modular prior (a DAG
// counts once per linear extension; not uniform over DAGs).
//
//   posterior scores.pss [-o edges.csv] [-s sets.txt] [-d device]
//
// The .pss is read as astar reads it (read_pss); scores = -costs, taken as
// natural-log weights, so the file should come from a Bayesian score
// (score --bge, --bdeu).  Lists pruned by dominance (cBIC's store rule,
// --prune) give the posterior over the pruned family only: Z is then a lower
// bound of the full sum.  Prints "ln Z = <value>".  -o writes the edge matrix,
// n rows of n comma-separated "%.6f" values, row u column v = p(u -> v);
// without -o it goes to standard output after the ln Z line.  -s writes one
// line per stored set, in the file's order: "<name>: <posterior %.6f> <parent
// names ...>".  Exit status: 0, 1 for a file or device error, 2 for a bad
// command line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/ulg.h"
#include "cli_common.h"
#include "io.h"

int main(int argc, char **argv) {
    ulgcli::Args args(
        {
            {"h", "help", false, "", "Show this help message."},
            {"o", "edges", true, "", "Write the edge posteriors here (csv, row u column v = p(u -> v))."},
            {"s", "sets", true, "", "Write the posterior of every stored parent set here."},
            {"d", "device", true, "0", "The GPU to use."},
        },
        {"scoreFile"});
    std::string err;
    if (!args.parse(argc, argv, err)) {
        std::fprintf(stderr, "posterior: %s\n", err.c_str());
        return 2;
    }
    if (args.has("help") || argc == 1 || !args.has("scoreFile")) {
        args.usage(argv[0],
                   "Posterior edge and parent-set probabilities by exact model averaging (order-modular prior) on an MI355X.  "
                   "Example usage: posterior iris.pss -o iris_edges.csv");
        return args.has("help") || argc == 1 ? 0 : 2;
    }
    ulgio::PssData p;
    if (!ulgio::read_pss(args.get("scoreFile"), p, err)) {
        std::fprintf(stderr, "posterior: %s\n", err.c_str());
        return 1;
    }
    const int n = (int)p.names.size();
    if (n < 1) {
        std::fprintf(stderr, "posterior: no variables in '%s'\n", args.get("scoreFile").c_str());
        return 1;
    }
    std::vector<float> scores(p.costs.size());
    for (size_t i = 0; i < scores.size(); ++i) scores[i] = -p.costs[i];
    if (p.sets.empty()) {  // the call takes no null lists
        p.sets.push_back(0);
        scores.push_back(0.0f);
    }
    const int dev = std::atoi(args.get("device").c_str());
    ulg_ctx *ctx = nullptr;
    if (ulg_create(&dev, 1, &ctx) != ULG_OK) {
        std::fprintf(stderr, "posterior: no usable HIP device %d\n", dev);
        return 1;
    }
    double log_z = 0.0;
    std::vector<double> edge((size_t)n * n), lp(scores.size());
    if (ulg_posterior(ctx, n, p.offsets.data(), p.sets.data(), scores.data(), 0, &log_z, edge.data(), lp.data()) != ULG_OK) {
        std::fprintf(stderr, "posterior: %s\n", ulg_last_error(ctx));
        ulg_destroy(ctx);
        return 1;
    }
    ulg_destroy(ctx);
    std::printf("ln Z = %.10f\n", log_z);
    std::string text;
    char buf[64];
    for (int u = 0; u < n; ++u)
        for (int v = 0; v < n; ++v) {
            std::snprintf(buf, sizeof buf, "%.6f%s", edge[(size_t)u * n + v], v + 1 < n ? "," : "\n");
            text += buf;
        }
    if (!args.has("edges")) {
        std::fputs(text.c_str(), stdout);
    } else if (!ulgio::write_text(args.get("edges"), text)) {
        std::fprintf(stderr, "posterior: cannot write '%s'\n", args.get("edges").c_str());
        return 1;
    }
    if (args.has("sets")) {
        text.clear();
        for (int v = 0; v < n; ++v)
            for (int64_t i = p.offsets[v]; i < p.offsets[v + 1]; ++i) {
                std::snprintf(buf, sizeof buf, ": %.6f", std::exp(lp[(size_t)i]));
                text += p.names[v] + buf;
                for (int u = 0; u < n; ++u)
                    if ((p.sets[(size_t)i] >> u) & 1ull) text += " " + p.names[u];
                text += "\n";
            }
        if (!ulgio::write_text(args.get("sets"), text)) {
            std::fprintf(stderr, "posterior: cannot write '%s'\n", args.get("sets").c_str());
            return 1;
        }
    }
    return 0;
}
