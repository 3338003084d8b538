// score -- the reference's score command line (score/score_main.cpp) on the
// MI355X path: the input CSV is read on the host, every parent set is scored
// by libulg.so on one GPU, and the .pss score cache is written in the
// reference's exact text format.
//
//   score <in.csv> <out.pss> [-f BIC] [--prune] [-k skeleton] [-c constraints] [-p k] [-s] [-d ,]
//   score <in.csv> <out.pss> --bdeu [-e ESS] [--prune] [-k skeleton] [-c constraints] [-p k] [-s] [-d ,]
//   score <in.csv> <out.pss> --fnml [--prune] [-k skeleton] [-c constraints] [-p k] [-s] [-d ,]
//   score <in.csv> <out.pss> -f cBIC --lambda L [-k skeleton] [-c constraints] [-p k] [-s] [-d ,]
//   score <in.csv> <out.pss> --bge [--alpha-mu A] [--alpha-w W] [--prune] [-k skeleton] [-c constraints] [-p k] [-r s] [-s] [-d ,]
//
// -f BIC (the default, as in the reference) is the discrete score: the tokens
// of each column are its values (load_discrete_csv), the parent limit is
// min(-p, (int) log(2N / log N)) (score_main.cpp:300-304) and --lambda is
// ignored.  -f cBIC reads the columns as numbers.  --bdeu is the discrete
// BDeu score (the reference's -f BDeu -e ESS; -f BDeu itself keeps being
// refused, as it was before BDeu was built): same reader, equivalent sample
// size -e (default 1, 1e-6 .. 1e6), "META score_type = bdeu", and no parent
// limit besides -p, since the reference applies log(2N / log N) to "bic" only
// (score_main.cpp:300-304) -- without -p every subset of the candidates is
// scored.  --fnml is the discrete fNML score (the reference's -f fNML; -f fNML
// itself keeps being refused): same reader, no parameter, "META score_type =
// fnml", no parent limit besides -p either; it does not go with --bdeu or
// -f cBIC.  --enableDeCamposPruning is not built for a discrete score
// (experimental in the reference).  Options that only matter for the
// reference's AD-tree or its other paths (-m, -w, -a, -o) are accepted; -e
// feeds the "META ess" header line as in score_main.cpp:388 whatever the score.
//
// --prune (-f BIC, --bdeu and --fnml) applies the reference's end-of-scoring prune()
// (score_calculator.cpp:137-197; its call is commented out in
// score_main.cpp:166-171 because it "might not work with continuous case") on
// the GPU: a parent set goes when a kept proper subset scores at least as well
// (within 2 FLT_EPSILON).  The .pss then holds the kept sets only, stdout gains
// "Size before pruning" / "Size after pruning" and the metrics line "pruned".
// -f cBIC refuses it: its store rule already tests dominance.
//
// --bge is the Bayesian score of the continuous data (ulg_bge_score; the
// reference has none): the columns are read as numbers, as for -f cBIC, the
// prior is --alpha-mu (default 1, 1e-3 .. 1e3) and --alpha-w (default 0 =
// n + alpha_mu + 1; otherwise above n + 1), "META score_type = bge", --lambda
// is ignored, and every finite value is written, positive ones included.
// --prune applies.  It does not go with --bdeu, --fnml, -f cBIC or
// --enableDeCamposPruning; -f BGe keeps being refused like every -f but BIC
// and cBIC.
#include <cmath>
#include <cctype>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/ulg.h"
#include "cli_common.h"
#include "io.h"

int main(int argc, char **argv) {
    using ulgcli::Opt;
    ulgcli::Args args(
        {
            {"d", "delimiter", true, ",", "The delimiter of the input file."},
            {"l", "lambda", true, "0.5", "The lambda (BIC penalty weight)."},
            {"a", "adaptive", false, "", "Use adaptive Lasso (not on this path)."},
            {"w", "scoreType", true, "1", "which score (not on this path)"},
            {"c", "constraints", true, "", "The file specifying constraints on the scores."},
            {"k", "skeleton", true, "", "The file specifying the skeleton superstructure"},
            {"m", "rMin", true, "5", "The minimum number of records in the AD-tree nodes (no effect: the counts are exact)."},
            {"f", "function", true, "BIC", "The scoring function to use (BIC or cBIC)."},
            {"e", "ess", true, "1", "The equivalent sample size of --bdeu, 1e-6 to 1e6 (always written to META ess)."},
            {"p", "maxParents", true, "0", "The maximum number of parents for any variable. A value less than 1 means no limit."},
            {"t", "threads", true, "1", "Host threads in the reference; the GPU scores every variable at once."},
            {"r", "time", true, "-1", "The maximum amount of time (s) to use for each variable (every variable is scored at once: the budget of the whole call, checked after each layer). A value less than 1 means no limit."},
            {"s", "hasHeader", false, "", "Add this flag if the first line of the input file gives the variable names."},
            {"o", "doNotPrune", false, "", "No effect (the reference's pruning is disabled, score_main.cpp:167-171; --prune runs it for -f BIC)."},
            {"", "prune", false, "", "Drop every parent set that a kept proper subset dominates (the reference's prune(); -f BIC, --bdeu, --fnml and --bge)."},
            {"", "bdeu", false, "", "Score with BDeu (the reference's -f BDeu) and equivalent sample size -e. There is no BIC parent limit: without -p every subset of the candidates is scored."},
            {"", "fnml", false, "", "Score with fNML (the reference's -f fNML). It has no parameter and no BIC parent limit: without -p every subset of the candidates is scored."},
            {"", "bge", false, "", "Score continuous data with BGe, the Bayesian Gaussian equivalent score (prior: --alpha-mu, --alpha-w). Every finite value is stored; --lambda is ignored."},
            {"", "alpha-mu", true, "1", "The prior's alpha_mu of --bge, 1e-3 to 1e3."},
            {"", "alpha-w", true, "0", "The prior's alpha_w of --bge: above n + 1, at most n + 1e6; 0 means n + alpha_mu + 1."},
            {"", "enableDeCamposPruning", false, "", "No effect for cBIC; refused for BIC, --bdeu and --fnml."},
            {"", "device", true, "0", "HIP device to use."},
            {"h", "help", false, "", "Show this help message."},
        },
        {"input", "output"});
    std::string err;
    if (!args.parse(argc, argv, err)) {
        std::fprintf(stderr, "score: %s\n", err.c_str());
        return 2;
    }
    if (args.has("help") || argc == 1 || !args.has("input") || !args.has("output")) {
        args.usage(argv[0], "Compute the scores for a csv file on an MI355X.  Example usage: score iris.csv iris.pss  (discrete BIC), or: score iris.csv iris.pss -f cBIC --lambda 2");
        return args.has("help") || argc == 1 ? 0 : 2;
    }
    std::string sf = args.get("function");
    for (char &ch : sf) ch = (char)std::tolower((unsigned char)ch);
    if (sf != "cbic" && sf != "bic") {
        std::fprintf(stderr, "score: scoring function '%s' is not on this path; use -f cBIC or -f BIC\n",
                     args.get("function").c_str());
        return 2;
    }
    const bool bdeu = args.has("bdeu");
    if (bdeu && sf != "bic") {
        std::fprintf(stderr, "score: --bdeu is a discrete score of its own; it does not go with -f %s\n",
                     args.get("function").c_str());
        return 2;
    }
    // boost::lexical_cast<float>(-e) in the reference; the same float, widened, is what BDeu uses
    const double ess = (double)std::strtof(args.get("ess").c_str(), nullptr);
    if (bdeu && !(ess >= 1e-6 && ess <= 1e6)) {
        std::fprintf(stderr, "score: --bdeu needs 1e-6 <= -e <= 1e6 (got '%s')\n", args.get("ess").c_str());
        return 2;
    }
    const bool fnml = args.has("fnml");
    if (fnml && bdeu) {
        std::fprintf(stderr, "score: --fnml and --bdeu are two scores; give one of them\n");
        return 2;
    }
    if (fnml && sf != "bic") {
        std::fprintf(stderr, "score: --fnml is a discrete score of its own; it does not go with -f %s\n",
                     args.get("function").c_str());
        return 2;
    }
    const bool bge = args.has("bge");
    if (bge && (bdeu || fnml)) {
        std::fprintf(stderr, "score: --bge is the score of continuous data; it does not go with --bdeu or --fnml\n");
        return 2;
    }
    if (bge && sf != "bic") {
        std::fprintf(stderr, "score: --bge is a continuous score of its own; it does not go with -f %s\n",
                     args.get("function").c_str());
        return 2;
    }
    if (bge && args.has("enableDeCamposPruning")) {
        std::fprintf(stderr, "score: --enableDeCamposPruning is not built for --bge\n");
        return 2;
    }
    const double alpha_mu = std::strtod(args.get("alpha-mu").c_str(), nullptr);
    const double alpha_w = std::strtod(args.get("alpha-w").c_str(), nullptr);
    if (bge && !(alpha_mu >= 1e-3 && alpha_mu <= 1e3)) {
        std::fprintf(stderr, "score: --bge needs 1e-3 <= --alpha-mu <= 1e3 (got '%s')\n", args.get("alpha-mu").c_str());
        return 2;
    }
    if (bge && !(alpha_w == 0.0 || (alpha_w > 0.0 && std::isfinite(alpha_w)))) {
        std::fprintf(stderr, "score: --bge needs --alpha-w above n + 1, or 0 for n + alpha_mu + 1 (got '%s')\n",
                     args.get("alpha-w").c_str());
        return 2;
    }
    if (bdeu) sf = "bdeu";
    if (fnml) sf = "fnml";
    if (bge) sf = "bge";
    const bool discrete = !bge && (sf == "bic" || bdeu || fnml);
    if (discrete && args.has("enableDeCamposPruning")) {
        std::fprintf(stderr, "score: --enableDeCamposPruning is not built for -f BIC, --bdeu or --fnml (it is a no-op for -f cBIC)\n");
        return 2;
    }
    const bool prune = args.has("prune");
    if (prune && !discrete && !bge) {
        std::fprintf(stderr, "score: --prune is for -f BIC, --bdeu and --fnml: the store rule of -f cBIC already tests dominance, and the "
                             "reference disabled prune() for the continuous case\n");
        return 2;
    }
    const std::string input = args.get("input"), output = args.get("output");
    const char delim = args.get("delimiter").empty() ? ',' : args.get("delimiter")[0];
    const bool has_header = args.has("hasHeader");
    const double lambda = std::atof(args.get("lambda").c_str());
    int maxp = std::atoi(args.get("maxParents").c_str());

    ulgio::RecordStats rs;
    ulgio::DiscreteData dd;
    std::vector<double> data;
    int64_t N = 0;
    int ncols = 0;
    if (discrete) {
        std::string derr;
        if (!ulgio::load_discrete_csv(input, delim, has_header, dd, derr)) {
            std::fprintf(stderr, "score: %s\n", derr.c_str());
            return 1;
        }
        rs.num_records = dd.num_records;
        rs.names = dd.names;
        rs.arity = dd.arity;
        N = dd.num_records;
        ncols = (int)dd.names.size();
    } else {
        if (!ulgio::record_stats(input, delim, has_header, rs)) {
            std::fprintf(stderr, "score: cannot read '%s'\n", input.c_str());
            return 1;
        }
        if (!ulgio::load_numeric_csv(input, data, N, ncols)) {
            std::fprintf(stderr, "score: cannot load '%s'\n", input.c_str());
            return 1;
        }
    }
    const int n = (int)rs.names.size();
    if (n != ncols || n < 1 || n > 63) {
        std::fprintf(stderr, "score: %d record columns vs %d numeric columns (n must be 1..63)\n", n, ncols);
        return 1;
    }
    if (maxp > n || maxp < 1) maxp = n - 1;  // score_main.cpp:296-298
    if (discrete) {
        // score_main.cpp:300-304; the reference divides by log 1 at N = 1
        if (N < 2) {
            std::fprintf(stderr, "score: %s needs at least 2 records ('%s' has %lld)\n", bdeu ? "--bdeu" : fnml ? "--fnml" : "-f BIC",
                         input.c_str(), (long long)N);
            return 2;
        }
        if (!bdeu && !fnml) {
            const int lim = (int)std::log(2 * (double)N / std::log((double)N));
            if (lim < maxp) maxp = lim;
        }
    }
    // -c: scoring::parseConstraints over the .pss names (score_main.cpp:314-317)
    const std::string cons_file = args.get("constraints");
    ulgio::Constraints cons;
    if (!cons_file.empty()) {
        std::printf("Constraints file: '%s'\n", cons_file.c_str());  // score_main.cpp:270
        std::string cerr_;
        if (!ulgio::read_constraints(cons_file, rs.names, cons, cerr_)) {
            std::fprintf(stderr, "score: %s\n", cerr_.c_str());
            return 1;
        }
    }
    // candidates: 2-hop skeleton neighbourhood; no -k = every variable
    std::vector<uint64_t> cands(n, n >= 64 ? ~0ull : ((1ull << n) - 1ull));
    const std::string skel = args.get("skeleton");
    if (!skel.empty()) {
        std::vector<uint64_t> rows;
        int nv = 0;
        if (ulgio::read_skeleton(skel, n, rows, nv)) {
            for (int v = 0; v < n; ++v) cands[v] = ulgio::candidates(rows, n, v);
        } else {
            // an unreadable -k leaves the default Skeleton(1) whose get_neighbors is {0}
            for (int v = 0; v < n; ++v) cands[v] = 1ull;
        }
    }
    const int dev = std::atoi(args.get("device").c_str());
    ulg_ctx *ctx = nullptr;
    if (ulg_create(&dev, 1, &ctx) != ULG_OK) {
        std::fprintf(stderr, "score: no usable HIP device %d\n", dev);
        return 1;
    }
    const double t0 = ulgcli::now_s();
    int rc = discrete ? ulg_disc_load(ctx, dd.codes.data(), N, n, dd.arity.data())
                      : ulg_cbic_load(ctx, data.data(), N, n, lambda);
    std::vector<int> vars(n);
    for (int v = 0; v < n; ++v) vars[v] = v;
    int64_t stored = 0, scored = 0;
    const int running_time = std::atoi(args.get("time").c_str());
    if (running_time > 0) {
        std::printf("I am using a timer in the calculation function.\n");  // score_calculator.cpp:40
        if (rc == ULG_OK) rc = ulg_set_option(ctx, "time_limit_ms", (int64_t)running_time * 1000);
    }
    if (rc == ULG_OK && !cons.vars.empty())
        rc = ulg_cbic_set_constraints(ctx, (int)cons.vars.size(), cons.vars.data(), cons.required.data(),
                                      cons.forbidden.data());
    if (rc == ULG_OK && prune) rc = ulg_set_option(ctx, bge ? "bge_prune" : "disc_prune", 1);
    if (rc == ULG_OK && bdeu) rc = ulg_disc_set_ess(ctx, ess);
    if (rc == ULG_OK && bge) rc = ulg_bge_set_prior(ctx, alpha_mu, alpha_w);
    if (rc == ULG_OK && bge)
        rc = ulg_bge_score(ctx, vars.data(), n, cands.data(), maxp, &stored, &scored);
    else if (rc == ULG_OK)
        rc = discrete ? ulg_disc_score(ctx, bdeu ? ULG_SCORE_BDEU : fnml ? ULG_SCORE_FNML : ULG_SCORE_BIC, vars.data(), n, cands.data(), maxp, &stored, &scored)
                      : ulg_cbic_score(ctx, vars.data(), n, cands.data(), maxp, &stored, &scored);
    int64_t oot = 0, done_layer = 0, pruned = 0;
    if (rc == ULG_OK && prune) {
        ulg_get_info(ctx, bge ? "bge_pruned" : "disc_pruned", &pruned);
        // score_main.cpp:159,170, once for the whole call
        std::printf("Size before pruning: %lld\nSize after pruning: %lld\n", (long long)(stored + pruned), (long long)stored);
    }
    if (rc == ULG_OK && running_time > 0) {
        ulg_get_info(ctx, "out_of_time", &oot);
        ulg_get_info(ctx, "highest_completed_layer", &done_layer);
        if (oot) std::printf("Out of time\n");  // score_calculator.cpp:28-31
    }
    const double t1 = ulgcli::now_s();
    if (rc != ULG_OK) {
        std::fprintf(stderr, "score: %s\n", ulg_last_error(ctx));
        ulg_destroy(ctx);
        return 1;
    }
    ulgio::PssHeader h;
    h.input_file = input;
    h.num_records = rs.num_records;
    h.parent_limit = maxp;
    h.score_type = sf;
    {
        // boost::lexical_cast<std::string>(float)
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.9g", ess);
        h.ess = buf;
    }
    const std::string header = ulgio::pss_header_text(h);
    std::vector<const char *> cnames(n);
    for (int v = 0; v < n; ++v) cnames[v] = rs.names[v].c_str();
    const char *text = nullptr;
    int64_t len = 0;
    rc = ulg_pss_format(ctx, header.c_str(), cnames.data(), rs.arity.data(), &text, &len);
    const double t2 = ulgcli::now_s();
    if (rc != ULG_OK) {
        std::fprintf(stderr, "score: %s\n", ulg_last_error(ctx));
        ulg_destroy(ctx);
        return 1;
    }
    if (!ulgio::write_bytes(output, text, len)) {
        std::fprintf(stderr, "score: cannot write '%s'\n", output.c_str());
        ulg_destroy(ctx);
        return 1;
    }
    ulg_destroy(ctx);
    const double t3 = ulgcli::now_s();
    std::printf("URLearning (MI355X), Score Calculator: n=%d N=%lld k=%d lambda=%g\n", n, (long long)N, maxp, lambda);
    if (oot) std::printf("Scoring stopped after layer %lld of %d (-r %d s)\n", (long long)done_layer, maxp, running_time);
    std::printf("Parent sets scored: %lld, stored: %lld, GPU scoring %.3f s (%.3g sets/s), GPU .pss format %.3f s, "
                "file write %.3f s (%lld bytes)\n",
                (long long)scored, (long long)stored, t1 - t0, (double)scored / (t1 - t0), t2 - t1, t3 - t2,
                (long long)len);
    char pruned_field[48] = "";
    if (prune) std::snprintf(pruned_field, sizeof pruned_field, ", \"pruned\": %lld", (long long)pruned);
    char ess_field[48] = "";
    if (bdeu) std::snprintf(ess_field, sizeof ess_field, ", \"ess\": %.9g", ess);
    char prior_field[96] = "";
    if (bge) std::snprintf(prior_field, sizeof prior_field, ", \"alpha_mu\": %.9g, \"alpha_w\": %.9g", alpha_mu, alpha_w);
    std::fprintf(stderr,
                 "ulg_metrics {\"tool\": \"score\", \"function\": \"%s\", \"n\": %d, \"N\": %lld, \"k\": %d, \"lambda\": %g, "
                 "\"scored\": %lld, \"stored\": %lld, \"score_s\": %.6f, \"sets_per_s\": %.6g, \"format_s\": %.6f, "
                 "\"write_s\": %.6f, \"bytes\": %lld, \"out_of_time\": %d%s%s%s}\n",
                 sf.c_str(), n, (long long)N, maxp, lambda, (long long)scored, (long long)stored, t1 - t0,
                 (double)scored / (t1 - t0), t2 - t1, t3 - t2, (long long)len, (int)oot, pruned_field, ess_field, prior_field);
    return 0;
}
