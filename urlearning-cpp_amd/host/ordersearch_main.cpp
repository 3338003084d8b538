// ordersearch -- the best network an order-space tabu search finds on a .pss
// score cache, for up to 63 variables (ulg_order_search_*; contract:
// include/ulg.h, "Order search").  Past n ~ 30, where astar's tables end, this
// is the tool that names a DAG; it is a heuristic and proves no optimality.
//
//   ordersearch <in.pss> [-n netFile] [--searches C] [--steps T] [--tenure K]
//               [--patience P] [--seed S] [-r] [--tables]
//               [--window W [--window-stride s] [--window-sweeps K] [--rounds R]]
//
// The .pss is read as astar reads it (read_pss); scores = -costs.  netFile and
// netFile.csv are astar's: "Var v, parents .." lines in the best order, and
// the 0/1 matrix with row v, column u = 1 for u -> v.  One line is printed.
// The defaults -- 256 searches, 20 n^2 steps, tenure n / 2, patience 4 n -- are
// untuned starting points.
//
// --window W re-optimises the C best orders by exact windows of W positions
// (ulg_order_window) after the run and reports those; with --rounds R the
// searches begin again from the re-optimised orders (seed + round), run --steps
// more and are re-optimised again, R times in all.  A second line is printed.
// Without --window the tool's output is what it was before the option existed.
//
// --tables searches over the dense candidate-set tables (option
// "search_tables"): the same searches bit for bit, for lists whose every
// variable has at most 26 candidate parents.  Without the flag nothing changes.
#include <chrono>
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
            {"n", "netFile", true, "", "The file to which the best network found is written (and netFile.csv, its 0/1 matrix)."},
            {"", "searches", true, "", "The number of independent searches, 1..1048576 (default 256, untuned)."},
            {"", "steps", true, "", "Steps of every search (default 20 n^2, untuned)."},
            {"", "tenure", true, "", "Steps a swapped pair stays tabu, 0..1048576 (default n / 2, untuned)."},
            {"", "patience", true, "", "Steps without a new best before a search is kicked off its best order (default 4 n, untuned)."},
            {"", "seed", true, "0", "The seed of the initial orders and the kicks."},
            {"r", "random", false, "", "Take the seed from the clock instead."},
            {"", "tables", false, "", "Search over dense candidate-set tables (at most 26 candidate parents per variable; untuned)."},
            {"", "window", true, "", "Re-optimise the best orders by exact windows of this many positions, 2..12 (default: none)."},
            {"", "window-stride", true, "", "Positions between two window starts, 1..window (default window / 2, untuned)."},
            {"", "window-sweeps", true, "", "Sweeps of a re-optimisation at most (default 64, untuned)."},
            {"", "rounds", true, "", "Rounds of search and re-optimisation (default 1, untuned); needs --window."},
            {"d", "device", true, "0", "The GPU to use."},
            {"h", "help", false, "", "Show this help message."},
        },
        {"scoreFile"});
    std::string err;
    if (!args.parse(argc, argv, err)) {
        std::fprintf(stderr, "ordersearch: %s\n", err.c_str());
        return 2;
    }
    if (args.has("help") || argc == 1 || !args.has("scoreFile")) {
        args.usage(argv[0],
                   "Learn a Bayesian network of up to 63 variables by tabu search over variable orders on an MI355X: the best "
                   "network found, not a proven optimum.  Example usage: ordersearch big.pss -n big_net");
        return args.has("help") || argc == 1 ? 0 : 2;
    }
    ulgio::PssData p;
    if (!ulgio::read_pss(args.get("scoreFile"), p, err)) {
        std::fprintf(stderr, "ordersearch: %s\n", err.c_str());
        return 1;
    }
    const int n = (int)p.names.size();
    if (n < 1) {
        std::fprintf(stderr, "ordersearch: no variables in '%s'\n", args.get("scoreFile").c_str());
        return 1;
    }
    auto number = [&](const char *name, long long def) { return args.get(name).empty() ? def : std::atoll(args.get(name).c_str()); };
    const int64_t C = number("searches", 256), steps = number("steps", 20ll * n * n), tenure = number("tenure", n / 2),
                  patience = number("patience", 4ll * n);
    uint64_t seed = std::strtoull(args.get("seed").c_str(), nullptr, 10);
    if (args.has("random")) seed = (uint64_t)std::chrono::system_clock::now().time_since_epoch().count();
    if (C < 1 || steps < 0) {
        std::fprintf(stderr, "ordersearch: --searches must be >= 1 and --steps >= 0\n");
        return 2;
    }
    const bool windowed = args.has("window");
    const int width = (int)number("window", 0), wstride = (int)number("window-stride", 0);
    const int64_t wsweeps = number("window-sweeps", 64), rounds = number("rounds", 1);
    if (rounds < 1 || (!windowed && (args.has("window-stride") || args.has("window-sweeps") || args.has("rounds")))) {
        std::fprintf(stderr, "ordersearch: --rounds must be >= 1; it, --window-stride and --window-sweeps need --window\n");
        return 2;
    }
    std::vector<float> scores(p.costs.size());
    for (size_t i = 0; i < scores.size(); ++i) scores[i] = -p.costs[i];
    const int dev = std::atoi(args.get("device").c_str());
    ulg_ctx *ctx = nullptr;
    if (ulg_create(&dev, 1, &ctx) != ULG_OK) {
        std::fprintf(stderr, "ordersearch: no usable HIP device %d\n", dev);
        return 1;
    }
    if (args.has("tables") && ulg_set_option(ctx, "search_tables", 1) != ULG_OK) {
        std::fprintf(stderr, "ordersearch: %s\n", ulg_last_error(ctx));
        ulg_destroy(ctx);
        return 1;
    }
    const double t0 = ulgcli::now_s();
    std::vector<double> best((size_t)C);
    std::vector<uint8_t> order((size_t)C * n);
    std::vector<uint64_t> parents((size_t)C * n);
    std::vector<int64_t> moves((size_t)C), kicks((size_t)C);
    auto fail = [&]() {
        std::fprintf(stderr, "ordersearch: %s\n", ulg_last_error(ctx));
        ulg_destroy(ctx);
        return 1;
    };
    if (ulg_order_search_begin(ctx, n, p.offsets.data(), p.sets.data(), scores.data(), 0, C, seed, tenure, patience, nullptr) != ULG_OK ||
        ulg_order_search_run(ctx, steps, best.data(), order.data(), parents.data(), moves.data(), kicks.data(), nullptr, nullptr) !=
            ULG_OK)
        return fail();
    // --window: the best orders re-optimised, and with --rounds searched on from there
    double window_s = 0, before = 0;
    int64_t improved_windows = 0, improved_searches = 0;
    if (windowed) {
        std::vector<int64_t> accepted((size_t)C), m((size_t)C), k((size_t)C);
        std::vector<char> improved((size_t)C, 0);
        for (int64_t r = 0; r < rounds; ++r) {
            if (r > 0) {
                if (ulg_order_search_begin(ctx, n, p.offsets.data(), p.sets.data(), scores.data(), 0, C, seed + (uint64_t)r, tenure, patience,
                                           order.data()) != ULG_OK ||
                    ulg_order_search_run(ctx, steps, best.data(), order.data(), nullptr, m.data(), k.data(), nullptr, nullptr) != ULG_OK)
                    return fail();
                for (int64_t c = 0; c < C; ++c) moves[c] += m[c], kicks[c] += k[c];
            }
            before = best[0];
            for (int64_t c = 1; c < C; ++c) before = best[c] > before ? best[c] : before;
            const double w0 = ulgcli::now_s();
            if (ulg_order_window(ctx, C, order.data(), width, wstride, wsweeps, nullptr, best.data(), parents.data(), accepted.data(),
                                 nullptr) != ULG_OK)
                return fail();
            window_s += ulgcli::now_s() - w0;
            for (int64_t c = 0; c < C; ++c) improved_windows += accepted[c], improved[c] = improved[c] || accepted[c] > 0;
        }
        for (int64_t c = 0; c < C; ++c) improved_searches += improved[c];
    }
    const double t1 = ulgcli::now_s();
    ulg_destroy(ctx);
    int64_t at = 0, same = 0, all_moves = 0, all_kicks = 0;
    for (int64_t c = 0; c < C; ++c) {
        if (best[c] > best[at]) at = c;  // the least search among equals
        all_moves += moves[c], all_kicks += kicks[c];
    }
    for (int64_t c = 0; c < C; ++c) same += best[c] == best[at];
    std::printf("best score = %.6f, search %lld, %lld of %lld searches share it, %lld moves, %lld kicks\n", best[at], (long long)at,
                (long long)same, (long long)C, (long long)all_moves, (long long)all_kicks);
    if (windowed)
        std::printf("window %d: %lld windows improved in %lld of %lld searches, best score before = %.6f\n", width,
                    (long long)improved_windows, (long long)improved_searches, (long long)C, before);
    char wmetrics[96] = "";
    if (windowed) std::snprintf(wmetrics, sizeof wmetrics, ", \"window\": %d, \"window_s\": %.6f", width, window_s);
    std::fprintf(stderr,
                 "ulg_metrics {\"tool\": \"ordersearch\", \"n\": %d, \"searches\": %lld, \"steps\": %lld, \"seed\": %llu, "
                 "\"best_score\": %.6f, \"search_s\": %.6f%s}\n",
                 n, (long long)C, (long long)steps, (unsigned long long)seed, best[at], t1 - t0, wmetrics);
    const std::string net = args.get("netFile");
    if (!net.empty()) {
        const std::vector<uint64_t> vpar(parents.begin() + at * n, parents.begin() + (at + 1) * n);
        std::string txt = "NumVars " + std::to_string(n) + "\n";  // astar's layout
        for (int q = 0; q < n; ++q) {
            const int v = order[at * n + q];
            txt += "Var " + std::to_string(v + 1) + ", parents";
            for (int i = 0; i < n; ++i)
                if ((vpar[v] >> i) & 1ull) txt += ", " + std::to_string(i + 1);
            txt += "\n";
        }
        if (!ulgio::write_text(net, txt) || !ulgio::write_net_csv(net + ".csv", vpar, n)) {
            std::fprintf(stderr, "ordersearch: cannot write '%s'\n", net.c_str());
            return 1;
        }
    }
    return 0;
}
