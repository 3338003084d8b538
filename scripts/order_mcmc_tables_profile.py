"""First measurement of the order MCMC over log-sum tables (profiles/r37/order_mcmc_tables.json).

On the three list families of scripts/order_mcmc_profile.py (n = 25 dense, C4-like, C5-like):
1. Rate.  ulg_order_mcmc_run with option "mcmc_tables" beside the same build's list path, 256 and
   1024 chains, in two contexts timed in alternation, REPEATS times each after an untimed call:
   chain-steps per second over the wall clock of a call that ends in a synchronise and lasts
   0.08 s or more (the step count is doubled until it does); median, least, largest.  A family
   the tables refuse (a variable with more than 26 candidate parents) is recorded with the
   refusal's text.
2. Begin.  The wall clock of ulg_order_mcmc_begin with and without the tables' build, alternated
   likewise, K_max and the tables' bytes.
3. Split (n = 25, the command line's defaults: 256 chains, burn 5000, thin 100, 10^4 samples):
   the record phase with the DAG picks and without them, either path; the difference is the
   picks' list scans.
4. Law (n = 20 and 25, the same defaults): acceptance, R-hat of the log score and the largest
   deviation of the samples' edge frequencies from ulg_posterior's exact matrix in standard
   errors, either path.

    python scripts/order_mcmc_tables_profile.py out.json [rate] [split] [law]

With ULG_LIB set to another build's library only the list path is timed (the parent commit's,
for the run-to-run spread).
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "urlearning-cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import order_mcmc_ref as om  # noqa: E402
import posterior_ref as pr  # noqa: E402
import ulg  # noqa: E402
from order_mcmc_profile import c4like  # noqa: E402

REPEATS = 5
LEAST_SECONDS = 0.08
OTHER_BUILD = "ULG_LIB" in os.environ
QUIET = dict(want_order=False, want_score=False, want_parents=False)


def begin(ctx, lists, chains, tables):
    kw = {} if OTHER_BUILD else {"tables": tables}
    t0 = time.perf_counter()
    ctx.order_mcmc_begin(*lists, chains, seed=1, **kw)
    return time.perf_counter() - t0


def open_paths(lists, chains, out):
    """-> {"lists": ctx[, "tables": ctx]}, both begun; a refusal of the tables goes into out."""
    paths = {"lists": ulg.Context(0)}
    begin(paths["lists"], lists, chains, False)
    if not OTHER_BUILD:
        paths["tables"] = ulg.Context(0)
        try:
            begin(paths["tables"], lists, chains, True)
        except ulg.ULGError as e:
            out["tables_refused"] = str(e)
            paths.pop("tables").close()
    return paths


def spread(times, work):
    rates = sorted(work / t for t in times)
    return {"seconds": times, "steps_per_second_median": statistics.median(rates), "least": rates[0], "largest": rates[-1]}


def rate(lists, chains):
    offs = lists[0]
    n = len(offs) - 1
    out = {"n": n, "sets": int(offs[-1]), "chains": chains}
    paths = open_paths(lists, chains, out)
    try:
        if "tables" in paths:
            K = [bin(paths["tables"].order_mcmc_table(v)[0]).count("1") for v in range(n)]
            out["K_max"], out["table_bytes"] = max(K), int(sum(8 << k for k in K))
        out["run"] = {}
        steps = {}
        for k, ctx in paths.items():  # untimed calls: the code object, the caches, and a step count that lasts long enough
            steps[k] = 256
            while True:
                t0 = time.perf_counter()
                ctx.order_mcmc_run(steps[k], 1, **QUIET)
                if time.perf_counter() - t0 >= 1.5 * LEAST_SECONDS or steps[k] >= 1 << 22:
                    break
                steps[k] *= 2
        times = {k: [] for k in paths}
        for _ in range(REPEATS):
            for k, ctx in paths.items():
                t0 = time.perf_counter()
                r = ctx.order_mcmc_run(steps[k], 1, **QUIET)
                times[k].append(time.perf_counter() - t0)
                out.setdefault("acceptance", {})[k] = float(r["accepted"].sum()) / (chains * r["step"])
        for k in paths:
            out["run"][k] = dict(spread(times[k], chains * steps[k]), steps=steps[k])
        if "tables" in paths:
            out["tables_over_lists"] = out["run"]["tables"]["steps_per_second_median"] / out["run"]["lists"]["steps_per_second_median"]
            tb = {"lists": [], "tables": []}
            for _ in range(3):
                tb["lists"].append(begin(paths["lists"], lists, chains, False))
                tb["tables"].append(begin(paths["tables"], lists, chains, True))
            out["begin_seconds"] = tb
    finally:
        for ctx in paths.values():
            ctx.close()
    return out


def sampled(n, K, exact):
    """The command line's default run for K samples on the dense lists of n variables, either path."""
    lists = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
    chains, burn, thin = 256, 5000, 100
    recs = -(-K // chains)
    out = {"n": n, "sets": int(len(lists[1])), "chains": chains, "burn": burn, "thin": thin, "samples": K}
    edge = None
    if exact:
        ctx = ulg.Context(0)
        _, edge, _ = ctx.posterior(*lists, want_sets=False)
        ctx.close()
    paths = open_paths(lists, chains, out)
    try:
        for k, ctx in paths.items():
            t0 = time.perf_counter()
            ctx.order_mcmc_run(burn, thin, **QUIET)
            t_burn = time.perf_counter() - t0
            more = thin * (burn // thin + recs) - burn
            t0 = time.perf_counter()
            r = ctx.order_mcmc_run(more, thin)
            t_rec = time.perf_counter() - t0
            t0 = time.perf_counter()
            ctx.order_mcmc_run(more, thin, want_parents=False)  # the same count of steps and records, no picks
            t_nopick = time.perf_counter() - t0
            res = {"seconds": {"burn": t_burn, "records_with_picks": t_rec, "records_without_picks": t_nopick,
                               "picks": t_rec - t_nopick},
                   "acceptance": float(r["accepted"].sum()) / (chains * r["step"]), "rhat_log_score": ulg.order_rhat(r["log_score"])}
            if edge is not None:
                par = r["parents"].reshape(-1, n)[:K]
                freq = np.array([[float((((par[:, v] >> np.uint64(u)) & np.uint64(1)) == 1).mean()) for v in range(n)] for u in range(n)])
                se = np.sqrt(np.maximum(edge * (1 - edge), 0) / K)
                with np.errstate(divide="ignore", invalid="ignore"):
                    z = np.where(se > 0, np.abs(freq - edge) / se, 0.0)
                res["largest_edge_deviation_in_standard_errors"] = float(z.max())
                res["largest_edge_deviation"] = float(np.abs(freq - edge).max())
            out[k] = res
    finally:
        for ctx in paths.values():
            ctx.close()
    return out


def main():
    out, want = sys.argv[1], sys.argv[2:] or ["rate", "split", "law"]
    res = {"repeats": REPEATS, "other_build": OTHER_BUILD}

    def save(key, name, value):
        res.setdefault(key, {})[name] = value
        print(json.dumps({key: {name: value}}), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)

    if "rate" in want:
        families = {"n25": lambda: pr.make_lists(25, "dense", 2525, max_parents=4), "c4like": c4like,
                    "c5like": lambda: om.make_lists(32, 3232, max_parents=3).triple()}
        for name, make in families.items():
            lists = make()
            for chains in (256, 1024):
                save("rate", f"{name}-{chains}", rate(lists, chains))
    if "law" in want and not OTHER_BUILD:
        for n in (20, 25):
            save("law", f"n{n}", sampled(n, 10000, True))  # n = 25's seconds are the split as well
    elif "split" in want:
        save("split", "n25", sampled(25, 10000, False))


if __name__ == "__main__":
    main()
