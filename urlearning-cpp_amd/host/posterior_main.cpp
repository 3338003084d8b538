// posterior -- exact model averaging over a .pss on the MI355X path
// (ulg_posterior, include/ulg.h): ln Z, the matrix of edge posteriors and the
// posterior of every stored parent set, under the order-modular prior (a DAG
// counts once per linear extension; not uniform over DAGs).
//
//   posterior scores.pss [-o edges.csv] [-s sets.txt] [-d device]
//             [--sample K [--seed S] [-g dags.txt] [--uniform [--uniform-edges FILE]]
//              [--paths FILE] [--blankets FILE] [--compelled FILE] [--vstructs FILE]
//              [--mcmc [--chains C] [--burn B] [--thin T] [--rb-edges FILE]]]
//
// The .pss is read as astar reads it (read_pss); scores = -costs, taken as
// natural-log weights, so the file should come from a Bayesian score
// (score --bge, --bdeu).  Lists pruned by dominance (cBIC's store rule,
// --prune) give the posterior over the pruned family only: Z is then a lower
// bound of the full sum.  Prints "ln Z = <value>".  -o writes the edge matrix,
// n rows of n comma-separated "%.6f" values, row u column v = p(u -> v);
// without -o it goes to standard output after the ln Z line.  -s writes one
// line per stored set, in the file's order: "<name>: <posterior %.6f> <parent
// names ...>".  --sample K draws K independent (order, DAG) pairs from the same
// posterior (ulg_posterior_sample; --seed S, default 0: sample k of a seed is
// the same in every run) and writes one line per sample: "%.6f" of the log
// weight, then "<name><-<parent>,<parent>" for each variable in the sampled
// order, separated by spaces; to the file of -g, else to standard output after
// everything above.  --uniform (with --sample) reweights the samples to the
// prior uniform over DAGs of the stored families: every sample line gains a
// second field after the log weight, the exact number of linear extensions of
// its DAG in decimal (ulg_dag_linear_extensions, per block of 2^16 samples with
// duplicate DAGs removed), and "uniform-prior ESS = %.1f of K" is printed on
// standard output right after the ln Z line: the effective sample size
// (sum r)^2 / sum r^2 of the weights r_k = exp(min log_ext - log_ext_k).
// --uniform-edges FILE (with --uniform) writes sum_k r_k [u in Pa_v^k] / sum_k
// r_k in -o's format.  The minimum is known only after the last block, so the
// counts' logarithms and the parent masks are kept and the sums are formed in a
// second pass over them, in float64 over k ascending: the summation of
// ulg.uniform_prior_edges (urlearning-cpp_amd/ulg.py) term by term.
// --paths, --blankets, --compelled FILE (with --sample) write the sample means
// of the features that do not factor over one parent set, each in -o's
// format: row u column v = the estimate of p(u ~> v) (a directed path), of
// p(u in the Markov blanket of v), and of p(u -> v is compelled: directed in
// the essential graph of the sampled DAG, the directed statement a
// score-equivalent score supports).  --vstructs FILE writes one line
// "<name_u> -> <name_v> <- <name_w> %.6f" per v-structure that occurs, sorted
// by (v, u, w).  All four come from one ulg_dag_features call over all K
// samples: exact integer tables, divided by their total as doubles.  Without
// --uniform every sample weighs 1; with it sample k weighs the integer
// floor(r_k 2^B), B = min(52, 62 - ceil(log2 K)): ulg.uniform_prior_weights
// term by term.
// --mcmc (with --sample) takes the K samples from order MCMC
// (ulg_order_mcmc_*) and not from the exact tables, which end at 28
// variables: no exact call is made and no ln Z line printed; n <= 63.  C chains
// (--chains, default 256) run B steps unrecorded (--burn, default 5000), then
// on until each has R = ceil(K / C) records, one after every step t that is a
// multiple of T (--thin, default 100; t counts from the start, so a chain makes
// T (floor(B / T) + R) steps in all); record r of chain c is sample r C + c and
// the first K are used.  The defaults are untuned starting points: the line
//   order MCMC: C chains, <steps> steps each, acceptance = %.3f, R-hat(log score) = %.3f
// printed in the ln Z line's place is what to read (R-hat: Gelman-Rubin over
// the recorded chains' log scores, ulg.order_rhat term by term; "n/a" for
// fewer than 2 records or chains).  The sample lines, -g, --uniform (its own
// n <= 28 still holds) and the feature files are as above; the edge matrix
// (-o, else standard output) is then the samples' mean edge frequency from
// the same ulg_dag_features call, weighted as the feature files are.  -s has
// no counterpart and is refused with --mcmc.
// --rb-edges FILE (with --mcmc) writes, in -o's format, the Rao-Blackwellised
// edge matrix of the very K orders the run recorded (ulg_order_edges): the mean
// over the orders of the closed form p(u -> v | order), an estimate of the same
// order-modular posterior as -o's sample mean with a variance that is never
// larger; it does not mend a chain that has not mixed (R-hat stays the thing to
// read).  One table per chain (groups = C) when C >= 2, K >= C and the tables
// fit 2^28 bytes, else one table; at most 2^22 samples.  The line
//   Rao-Blackwell edges: K orders, Z of probability 0, largest standard error = %.6f
// follows the order MCMC line: the standard error of the mean across chains
// (ulg.order_edge_posterior term by term), or "standard error not computed"
// with one table, and also with a table per chain when Z > 0: which chain an
// order of probability 0 belongs to is not reported, so the chains' counts
// are not known (a chain never records such an order; Z is then 0).  -o's file is the same with and without it.
// Exit status: 0, 1 for a file or device error, 2 for a bad command line
// (--seed, -g, --uniform, --mcmc or a feature file without --sample,
// --uniform-edges without --uniform, --chains, --burn or --thin without
// --mcmc, --rb-edges without --mcmc or with more than 2^22 samples, -s with
// --mcmc, a K that is not a positive integer, and --thin, --burn and K / C that
// together pass 2^62 steps per chain included).
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ulg.h"
#include "cli_common.h"
#include "io.h"

namespace {

// lo + 2^64 hi in decimal
std::string decimal128(uint64_t lo, uint64_t hi) {
    unsigned __int128 x = ((unsigned __int128)hi << 64) | lo;
    if (x == 0) return "0";
    std::string out;
    for (; x != 0; x /= 10) out.insert(out.begin(), (char)('0' + (int)(x % 10)));
    return out;
}

}  // namespace

int main(int argc, char **argv) {
    ulgcli::Args args(
        {
            {"h", "help", false, "", "Show this help message."},
            {"o", "edges", true, "", "Write the edge posteriors here (csv, row u column v = p(u -> v)); with --mcmc, the "
                                     "samples' mean edge frequencies."},
            {"s", "sets", true, "", "Write the posterior of every stored parent set here."},
            {"d", "device", true, "0", "The GPU to use."},
            {"", "sample", true, "", "Draw this many (order, DAG) samples from the posterior."},
            {"", "seed", true, "", "The samples' seed (with --sample; 0 without it)."},
            {"g", "dags", true, "", "Write the samples here instead of standard output (with --sample)."},
            {"", "uniform", false, "", "Reweight the samples to the prior uniform over DAGs: each sample line gains its DAG's "
                                       "number of linear extensions, and the effective sample size is printed (with --sample)."},
            {"", "uniform-edges", true, "", "Write the reweighted edge posteriors here, in -o's format (with --uniform)."},
            {"", "paths", true, "", "Write the sampled p(u ~> v), a directed path from u to v, here in -o's format (with --sample)."},
            {"", "blankets", true, "", "Write the sampled p(u in the Markov blanket of v) here in -o's format (with --sample)."},
            {"", "compelled", true, "", "Write the sampled p(u -> v is directed in the essential graph) here in -o's format "
                                        "(with --sample)."},
            {"", "vstructs", true, "", "Write the sampled p(u -> v <- w, u and w not adjacent) here, a line per triple that "
                                       "occurs (with --sample)."},
            {"", "mcmc", false, "", "Take the samples from order MCMC instead of the exact tables: up to 63 variables, no ln Z "
                                    "(with --sample; not with -s)."},
            {"", "chains", true, "", "The number of chains, 1..1048576 (with --mcmc; default 256, an untuned starting point: "
                                     "read the R-hat that is printed)."},
            {"", "burn", true, "", "Steps every chain makes before its first record (with --mcmc; default 5000, untuned)."},
            {"", "thin", true, "", "A record after every this many steps (with --mcmc; default 100, untuned)."},
            {"", "rb-edges", true, "", "Write the Rao-Blackwellised edge posteriors of the recorded orders here, in -o's format "
                                       "(with --mcmc; at most 4194304 samples)."},
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
    long long samples = 0;
    unsigned long long seed = 0;
    if (!args.has("sample") && (args.has("seed") || args.has("dags"))) {
        std::fprintf(stderr, "posterior: --seed and -g need --sample\n");
        return 2;
    }
    const bool uniform = args.has("uniform");
    if ((uniform && !args.has("sample")) || (args.has("uniform-edges") && !uniform)) {
        std::fprintf(stderr, "posterior: --uniform needs --sample, --uniform-edges needs --uniform\n");
        return 2;
    }
    const char *const feature_flags[4] = {"paths", "blankets", "compelled", "vstructs"};
    bool features = false;
    for (const char *f : feature_flags) features = features || args.has(f);
    if (features && !args.has("sample")) {
        std::fprintf(stderr, "posterior: --paths, --blankets, --compelled and --vstructs need --sample\n");
        return 2;
    }
    const bool mcmc = args.has("mcmc");
    if (mcmc && (!args.has("sample") || args.has("sets"))) {
        std::fprintf(stderr, "posterior: --mcmc needs --sample and does not go with -s\n");
        return 2;
    }
    if (!mcmc && (args.has("chains") || args.has("burn") || args.has("thin"))) {
        std::fprintf(stderr, "posterior: --chains, --burn and --thin need --mcmc\n");
        return 2;
    }
    const bool rb = args.has("rb-edges");
    if (rb && !mcmc) {
        std::fprintf(stderr, "posterior: --rb-edges needs --mcmc\n");
        return 2;
    }
    long long chains = 256, burn = 5000, thin = 100;
    {
        const struct {
            const char *name;
            long long *value, least, most;
        } ints[3] = {{"chains", &chains, 1, 1 << 20}, {"burn", &burn, 0, 1ll << 40}, {"thin", &thin, 1, 1ll << 40}};
        for (const auto &o : ints) {
            if (!args.has(o.name)) continue;
            const std::string t = args.get(o.name);
            char *end = nullptr;
            errno = 0;
            *o.value = std::strtoll(t.c_str(), &end, 10);
            if (t.empty() || t.find_first_not_of("0123456789") != std::string::npos || errno || *end || *o.value < o.least ||
                *o.value > o.most) {
                std::fprintf(stderr, "posterior: --%s takes an integer %lld..%lld, not '%s'\n", o.name, o.least, o.most, t.c_str());
                return 2;
            }
        }
    }
    if (args.has("sample")) {
        const std::string k = args.get("sample");
        char *end = nullptr;
        errno = 0;
        samples = std::strtoll(k.c_str(), &end, 10);
        if (k.empty() || k.find_first_not_of("0123456789") != std::string::npos || errno || *end || samples < 1) {
            std::fprintf(stderr, "posterior: --sample takes a positive integer, not '%s'\n", k.c_str());
            return 2;
        }
    }
    if (args.has("seed")) {
        const std::string t = args.get("seed");
        char *end = nullptr;
        errno = 0;
        seed = std::strtoull(t.c_str(), &end, 10);
        if (t.empty() || t.find_first_not_of("0123456789") != std::string::npos || errno || *end) {
            std::fprintf(stderr, "posterior: --seed takes an unsigned 64-bit integer, not '%s'\n", t.c_str());
            return 2;
        }
    }
    // --mcmc: every chain makes thin (floor(burn / thin) + ceil(samples / chains)) steps; kept below 2^62
    const long long mcmc_recs = samples / chains + (samples % chains != 0 ? 1 : 0);
    if (mcmc && mcmc_recs > (1ll << 62) / thin - burn / thin) {
        std::fprintf(stderr, "posterior: %lld records per chain at --thin %lld after --burn %lld pass 2^62 steps\n", mcmc_recs, thin, burn);
        return 2;
    }
    if (rb && samples > (1ll << 22)) {
        std::fprintf(stderr, "posterior: --rb-edges takes at most 4194304 samples, not %lld\n", samples);
        return 2;
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
    // --mcmc: every chain's records, sample r * chains + c = record r of chain c; the line that stands for ln Z
    std::vector<uint64_t> m_par;
    std::vector<uint8_t> m_ord;
    std::vector<double> m_lw;
    std::string mcmc_line;
    std::vector<double> rb_mean;  // --rb-edges: the matrix
    if (!mcmc) {
        if (ulg_posterior(ctx, n, p.offsets.data(), p.sets.data(), scores.data(), 0, &log_z, edge.data(), lp.data()) != ULG_OK) {
            std::fprintf(stderr, "posterior: %s\n", ulg_last_error(ctx));
            ulg_destroy(ctx);
            return 1;
        }
    } else {
        const long long recs = mcmc_recs;
        const long long steps = thin * (burn / thin + recs);  // the step of the last record; >= burn + 1, < 2^62 (checked above)
        int64_t got = 0;
        std::vector<double> m_ls;
        std::vector<int64_t> m_acc((size_t)chains);
        try {
            if (recs > (1ll << 46) / (chains * n)) throw std::length_error("records");  // the products below stay far inside size_t
            m_par.resize((size_t)recs * chains * n);
            m_ord.resize((size_t)recs * chains * n);
            m_lw.resize((size_t)recs * chains);
            m_ls.resize((size_t)recs * chains);
        } catch (const std::exception &) {
            std::fprintf(stderr, "posterior: out of memory for %lld records of %lld chains\n", recs, chains);
            ulg_destroy(ctx);
            return 1;
        }
        if (ulg_order_mcmc_begin(ctx, n, p.offsets.data(), p.sets.data(), scores.data(), 0, chains, seed, nullptr) != ULG_OK ||
            ulg_order_mcmc_run(ctx, burn, thin, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ULG_OK ||
            ulg_order_mcmc_run(ctx, steps - burn, thin, m_ord.data(), m_ls.data(), m_par.data(), m_lw.data(), m_acc.data(), nullptr,
                               nullptr, &got) != ULG_OK) {
            std::fprintf(stderr, "posterior: %s\n", ulg_last_error(ctx));
            ulg_destroy(ctx);
            return 1;
        }
        if (got != recs) {
            std::fprintf(stderr, "posterior: %lld records per chain, not %lld\n", (long long)got, recs);
            ulg_destroy(ctx);
            return 1;
        }
        long long accepted = 0;
        for (int64_t a : m_acc) accepted += a;
        // Gelman-Rubin over the (recs, chains) log scores: ulg.order_rhat, every sum over its index ascending
        double rhat = NAN;
        if (recs >= 2 && chains >= 2) {
            const double R = (double)recs, C = (double)chains;
            std::vector<double> mc((size_t)chains, 0.0), ss((size_t)chains, 0.0);
            for (long long r = 0; r < recs; ++r)
                for (long long c = 0; c < chains; ++c) mc[(size_t)c] += m_ls[(size_t)(r * chains + c)];
            for (double &x : mc) x /= R;
            double m = 0.0;
            for (double x : mc) m += x;
            m /= C;
            for (long long r = 0; r < recs; ++r)
                for (long long c = 0; c < chains; ++c) {
                    const double d = m_ls[(size_t)(r * chains + c)] - mc[(size_t)c];
                    ss[(size_t)c] += d * d;
                }
            double W = 0.0, B = 0.0;
            for (double x : ss) W += x / (R - 1);
            W /= C;
            for (double x : mc) B += (x - m) * (x - m);
            B = R * B / (C - 1);
            if (W > 0) rhat = std::sqrt(((R - 1) / R * W + B / R) / W);
        }
        char line[256], rh[32];
        if (std::isnan(rhat)) std::snprintf(rh, sizeof rh, "n/a");
        else std::snprintf(rh, sizeof rh, "%.3f", rhat);
        std::snprintf(line, sizeof line, "order MCMC: %lld chains, %lld steps each, acceptance = %.3f, R-hat(log score) = %s\n", chains,
                      steps, (double)accepted / ((double)chains * (double)steps), rh);
        mcmc_line = line;
        if (rb) {
            // a table per chain where that gives a standard error and fits; sample k = record k / chains of chain k % chains
            const long long groups = chains >= 2 && samples >= chains && 8 * chains * n * n <= (1ll << 28) ? chains : 1;
            std::vector<uint64_t> tab((size_t)groups * n * n);
            int64_t dead = 0;
            if (ulg_order_edges(ctx, samples, m_ord.data(), groups, tab.data(), &dead) != ULG_OK) {
                std::fprintf(stderr, "posterior: %s\n", ulg_last_error(ctx));
                ulg_destroy(ctx);
                return 1;
            }
            if (dead >= samples) {  // a recorded order has a finite term: not reached
                std::fprintf(stderr, "posterior: every recorded order has probability 0\n");
                ulg_destroy(ctx);
                return 1;
            }
            // ulg.order_edge_posterior: the integer sum over the groups, one division; the standard error over g ascending
            const double unit = 1099511627776.0;  // 2^40
            const size_t nn = (size_t)n * n;
            rb_mean.assign(nn, 0.0);
            for (size_t i = 0; i < nn; ++i) {
                uint64_t tot = 0;
                for (long long g = 0; g < groups; ++g) tot += tab[(size_t)g * nn + i];
                rb_mean[i] = (double)tot / (unit * (double)(samples - dead));
            }
            char se_text[64];
            std::snprintf(se_text, sizeof se_text, "standard error not computed");
            if (groups >= 2 && dead == 0) {  // which chain an order of probability 0 belongs to is not reported
                const double G = (double)groups;
                double worst = 0.0;
                for (size_t i = 0; i < nn; ++i) {
                    double mbar = 0.0, ss = 0.0;
                    for (long long g = 0; g < groups; ++g) {
                        const double cnt = (double)(samples / groups + (g < samples % groups ? 1 : 0));
                        mbar += (double)tab[(size_t)g * nn + i] / (unit * cnt);
                    }
                    mbar /= G;
                    for (long long g = 0; g < groups; ++g) {
                        const double cnt = (double)(samples / groups + (g < samples % groups ? 1 : 0));
                        const double d = (double)tab[(size_t)g * nn + i] / (unit * cnt) - mbar;
                        ss += d * d;
                    }
                    worst = std::max(worst, std::sqrt(ss / (G * (G - 1))));
                }
                std::snprintf(se_text, sizeof se_text, "largest standard error = %.6f", worst);
            }
            std::snprintf(line, sizeof line, "Rao-Blackwell edges: %lld orders, %lld of probability 0, %s\n", samples, (long long)dead,
                          se_text);
            mcmc_line += line;
        }
    }
    // the samples' lines, drawn and formatted a block at a time: the host buffers do not grow with K
    std::string sample_text;
    std::vector<double> all_le;      // --uniform: log_ext of every sample, and
    std::vector<uint64_t> all_par;   // its parent masks, for the pass that knows the minimum; also kept for the feature files
    // the feature files: tables of ulg_dag_features over all K samples (ancestor, blanket, compelled: n x n; v-structures: n^3)
    std::vector<uint64_t> f_anc, f_blanket, f_compelled, f_vs, f_edge;  // f_edge: --mcmc's edge matrix
    uint64_t f_total = 0;
    try {
        const long long block = 1 << 16;
        std::vector<uint64_t> s_par;
        std::vector<uint8_t> s_ord;
        std::vector<double> s_lw;
        // --uniform: the block's distinct DAGs and their counts; every sample's log count and masks for the second pass
        std::vector<uint64_t> u_par, u_lo, u_hi;
        std::vector<double> u_le;
        std::vector<size_t> which;
        char num[64];
        for (long long first = 0; first < samples; first += block) {
            const long long cnt = std::min(block, samples - first);
            s_par.resize((size_t)cnt * n);
            s_ord.resize((size_t)cnt * n);
            s_lw.resize((size_t)cnt);
            if (mcmc) {
                std::copy(m_par.begin() + (size_t)first * n, m_par.begin() + (size_t)(first + cnt) * n, s_par.begin());
                std::copy(m_ord.begin() + (size_t)first * n, m_ord.begin() + (size_t)(first + cnt) * n, s_ord.begin());
                std::copy(m_lw.begin() + (size_t)first, m_lw.begin() + (size_t)(first + cnt), s_lw.begin());
            } else if (ulg_posterior_sample(ctx, seed, first, cnt, s_par.data(), s_ord.data(), s_lw.data()) != ULG_OK) {
                std::fprintf(stderr, "posterior: %s\n", ulg_last_error(ctx));
                ulg_destroy(ctx);
                return 1;
            }
            if (uniform) {
                std::map<std::vector<uint64_t>, size_t> seen;
                u_par.clear();
                which.assign((size_t)cnt, 0);
                for (long long k = 0; k < cnt; ++k) {
                    std::vector<uint64_t> row(s_par.begin() + (size_t)k * n, s_par.begin() + (size_t)(k + 1) * n);
                    const auto at = seen.emplace(std::move(row), seen.size());
                    if (at.second) u_par.insert(u_par.end(), at.first->first.begin(), at.first->first.end());
                    which[(size_t)k] = at.first->second;
                }
                const size_t distinct = seen.size();
                u_lo.assign(distinct, 0);
                u_hi.assign(distinct, 0);
                u_le.assign(distinct, 0.0);
                if (ulg_dag_linear_extensions(ctx, n, (int64_t)distinct, u_par.data(), u_lo.data(), u_hi.data(), u_le.data()) !=
                    ULG_OK) {
                    std::fprintf(stderr, "posterior: %s\n", ulg_last_error(ctx));
                    ulg_destroy(ctx);
                    return 1;
                }
                for (long long k = 0; k < cnt; ++k) all_le.push_back(u_le[which[(size_t)k]]);
            }
            if (uniform || features || mcmc) all_par.insert(all_par.end(), s_par.begin(), s_par.end());
            for (long long k = 0; k < cnt; ++k) {
                std::snprintf(num, sizeof num, "%.6f", s_lw[(size_t)k]);
                sample_text += num;
                if (uniform) sample_text += " " + decimal128(u_lo[which[(size_t)k]], u_hi[which[(size_t)k]]);
                for (int i = 0; i < n; ++i) {
                    const int v = s_ord[(size_t)k * n + i];
                    sample_text += " " + p.names[v] + "<-";
                    const uint64_t pa = s_par[(size_t)k * n + v];
                    bool firstp = true;
                    for (int u = 0; u < n; ++u)
                        if ((pa >> u) & 1ull) {
                            sample_text += (firstp ? "" : ",") + p.names[u];
                            firstp = false;
                        }
                }
                sample_text += "\n";
            }
        }
        if (features || mcmc) {
            // --uniform: q_k = floor(exp(min log_ext - log_ext_k) 2^B), ulg.uniform_prior_weights; a count of 0 is
            // refused below, after the ln Z line, as without the feature files
            std::vector<uint64_t> q;
            double least = INFINITY;
            for (double x : all_le) least = std::min(least, x);
            if (uniform && least > -INFINITY) {
                int ceil_log2 = 0;
                while ((1ull << ceil_log2) < (unsigned long long)samples) ++ceil_log2;
                const int bits = std::min(52, 62 - ceil_log2);
                for (double x : all_le) q.push_back((uint64_t)std::floor(std::ldexp(std::exp(least - x), bits)));
            }
            if (!uniform || !q.empty()) {
                if (args.has("paths")) f_anc.resize((size_t)n * n);
                if (args.has("blankets")) f_blanket.resize((size_t)n * n);
                if (args.has("compelled")) f_compelled.resize((size_t)n * n);
                if (args.has("vstructs")) f_vs.resize((size_t)n * n * n);
                if (mcmc) f_edge.resize((size_t)n * n);
                if (ulg_dag_features(ctx, n, samples, all_par.data(), uniform ? q.data() : nullptr, f_edge.empty() ? nullptr : f_edge.data(),
                                     f_anc.empty() ? nullptr : f_anc.data(), f_blanket.empty() ? nullptr : f_blanket.data(),
                                     f_compelled.empty() ? nullptr : f_compelled.data(), f_vs.empty() ? nullptr : f_vs.data(),
                                     &f_total, nullptr) != ULG_OK) {
                    std::fprintf(stderr, "posterior: %s\n", ulg_last_error(ctx));
                    ulg_destroy(ctx);
                    return 1;
                }
            }
        }
    } catch (const std::exception &) {  // bad_alloc, length_error: the text of K lines does not fit
        std::fprintf(stderr, "posterior: out of memory for the lines of %lld samples\n", samples);
        ulg_destroy(ctx);
        return 1;
    }
    ulg_destroy(ctx);
    if (mcmc) std::fputs(mcmc_line.c_str(), stdout);
    else std::printf("ln Z = %.10f\n", log_z);
    std::string text;
    char buf[64];
    if (uniform) {
        // r_k = exp(min log_ext - log_ext_k); every sum in float64 over k ascending (ulg.uniform_prior_edges)
        double least = INFINITY;
        for (double x : all_le) least = std::min(least, x);
        if (!(least > -INFINITY)) {  // a count of 0: not a sampled DAG
            std::fprintf(stderr, "posterior: a sample without a linear extension\n");
            return 1;
        }
        double tot = 0.0, tot2 = 0.0;
        std::vector<double> acc((size_t)n * n, 0.0);
        for (size_t k = 0; k < all_le.size(); ++k) {
            const double r = std::exp(least - all_le[k]);
            tot += r;
            tot2 += r * r;
            for (int v = 0; v < n; ++v)
                for (uint64_t pa = all_par[k * n + v]; pa; pa &= pa - 1) acc[(size_t)__builtin_ctzll(pa) * n + v] += r;
        }
        std::printf("uniform-prior ESS = %.1f of %lld\n", tot * tot / tot2, samples);
        if (args.has("uniform-edges")) {
            for (int u = 0; u < n; ++u)
                for (int v = 0; v < n; ++v) {
                    std::snprintf(buf, sizeof buf, "%.6f%s", acc[(size_t)u * n + v] / tot, v + 1 < n ? "," : "\n");
                    text += buf;
                }
            if (!ulgio::write_text(args.get("uniform-edges"), text)) {
                std::fprintf(stderr, "posterior: cannot write '%s'\n", args.get("uniform-edges").c_str());
                return 1;
            }
            text.clear();
        }
    }
    if (rb) {
        for (int u = 0; u < n; ++u)
            for (int v = 0; v < n; ++v) {
                std::snprintf(buf, sizeof buf, "%.6f%s", rb_mean[(size_t)u * n + v], v + 1 < n ? "," : "\n");
                text += buf;
            }
        if (!ulgio::write_text(args.get("rb-edges"), text)) {
            std::fprintf(stderr, "posterior: cannot write '%s'\n", args.get("rb-edges").c_str());
            return 1;
        }
        text.clear();
    }
    if (mcmc)  // the samples' mean edge frequencies (with --uniform: under its weights)
        for (size_t i = 0; i < f_edge.size(); ++i) edge[i] = (double)f_edge[i] / (double)f_total;
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
    if (features) {
        const double tot = (double)f_total;
        const std::pair<const char *, const std::vector<uint64_t> *> square[3] = {
            {"paths", &f_anc}, {"blankets", &f_blanket}, {"compelled", &f_compelled}};
        for (const auto &t : square) {
            if (!args.has(t.first)) continue;
            text.clear();
            for (int u = 0; u < n; ++u)
                for (int v = 0; v < n; ++v) {
                    std::snprintf(buf, sizeof buf, "%.6f%s", (double)(*t.second)[(size_t)u * n + v] / tot, v + 1 < n ? "," : "\n");
                    text += buf;
                }
            if (!ulgio::write_text(args.get(t.first), text)) {
                std::fprintf(stderr, "posterior: cannot write '%s'\n", args.get(t.first).c_str());
                return 1;
            }
        }
        if (args.has("vstructs")) {
            text.clear();
            for (int v = 0; v < n; ++v)
                for (int u = 0; u < n; ++u)
                    for (int w = u + 1; w < n; ++w) {
                        const uint64_t x = f_vs[((size_t)v * n + u) * n + w];
                        if (!x) continue;
                        std::snprintf(buf, sizeof buf, " %.6f\n", (double)x / tot);
                        text += p.names[u] + " -> " + p.names[v] + " <- " + p.names[w] + buf;
                    }
            if (!ulgio::write_text(args.get("vstructs"), text)) {
                std::fprintf(stderr, "posterior: cannot write '%s'\n", args.get("vstructs").c_str());
                return 1;
            }
        }
    }
    if (samples) {
        text.swap(sample_text);
        if (!args.has("dags")) {
            std::fputs(text.c_str(), stdout);
        } else if (!ulgio::write_text(args.get("dags"), text)) {
            std::fprintf(stderr, "posterior: cannot write '%s'\n", args.get("dags").c_str());
            return 1;
        }
    }
    return 0;
}
