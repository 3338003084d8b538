"""First measurement of ulg_order_edges (profiles/r31/order_edges.json).

1. Price.  On the three families of lists of scripts/order_mcmc_profile.py
   (n25, c4like, c5like): the ulg_order_mcmc_run at the defaults (256 chains,
   burn 5000, thin 100) that records --orders orders, then on those orders
   ulg_order_edges (groups = chains) and ulg_order_score, the kernel that makes
   the same scan for the term alone: wall clock of each call (host checks,
   copies and the synchronise included), the kernels' own time from the
   context's profiler, the ratios, and list entries visited per second.  An
   entry is visited once per (order, position) whose variable lists it (both
   kernels read it twice, for the maximum and for the sum): orders x the number
   of list entries.  Beside them edges_grid's sweep on n25.
2. What it buys.  At n = 20 and 25 (the posterior probe's lists), defaults and
   --orders samples: the largest deviation from ulg_posterior's exact matrix of
   the sample mean (the 0/1 indicator of the recorded DAGs) and of the
   Rao-Blackwellised matrix, absolute and in standard errors.  Two standard
   errors each: of independent draws, sqrt(p (1 - p) / K) (which these are not;
   the README's earlier figures), and across the 256 chains (of the per-chain
   means; for both estimators from the same run).

    python scripts/order_edges_profile.py out.json [--orders 10000]
"""
import argparse
import json
import os
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

CHAINS, BURN, THIN = 256, 5000, 100


def record(ctx, lists, K, want_parents=False):
    """The CLI's run at the defaults -> (orders (K, n), the run's dict, seconds of begin + burn + records)."""
    offs, sets, scores = lists
    n = len(offs) - 1
    recs = -(-K // CHAINS)
    t0 = time.perf_counter()
    ctx.order_mcmc_begin(offs, sets, scores, CHAINS, seed=1)
    ctx.order_mcmc_run(BURN, THIN, want_order=False, want_score=False, want_parents=False)
    r = ctx.order_mcmc_run(THIN * (BURN // THIN + recs) - BURN, THIN, want_parents=want_parents, want_weight=False)
    return r["order"].reshape(-1, n)[:K], r, time.perf_counter() - t0


def timed(fn, reps=3):
    out, times = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


def kernel_ms(ctx, fn, names):
    ctx.profile(True)
    ctx.profile_reset()
    fn()
    ms = {k: ctx.profile_get(k)["total_ms"] for k in names}
    ctx.profile(False)
    return ms


def price(ctx, lists, K):
    offs = lists[0]
    n, total = len(offs) - 1, int(offs[-1])
    orders, r, t_run = record(ctx, lists, K)
    ctx.order_edges(orders[:64], groups=1)  # untimed: the code objects
    ctx.order_score(orders[:64])
    (tab, zero), t_edges = timed(lambda: ctx.order_edges(orders, groups=CHAINS))
    _, t_score = timed(lambda: ctx.order_score(orders))
    out = {"n": n, "sets": total, "orders": int(len(orders)), "zero": int(zero), "steps_each": int(r["step"]),
           "seconds": {"mcmc_begin_burn_records": t_run, "order_edges": t_edges, "order_score": t_score},
           "edges_over_score_wall": min(t_edges) / min(t_score), "edges_over_run_wall": min(t_edges) / t_run,
           "entries_visited": len(orders) * total, "entries_per_second_edges_wall": len(orders) * total / min(t_edges),
           "edges_grid": ctx.info("edges_grid")}
    ms = kernel_ms(ctx, lambda: ctx.order_edges(orders, groups=CHAINS), ("edges_empty", "edges_flag", "edges_scatter"))
    ms.update(kernel_ms(ctx, lambda: ctx.order_score(orders), ("mcmc_score",)))
    out["kernel_ms"] = ms
    out["scatter_over_score_kernel"] = ms["edges_scatter"] / ms["mcmc_score"]
    out["entries_per_second_scatter_kernel"] = len(orders) * total / (ms["edges_scatter"] * 1e-3)
    return out, orders


def grid_sweep(ctx, orders):
    sweep = {}
    for grid in (256, 1024, 4096, 16384, 65536, 0):
        ctx.set_option("edges_grid", grid)
        _, t = timed(lambda: ctx.order_edges(orders, groups=CHAINS))
        sweep[str(grid)] = {"seconds": t, "launched": ctx.info("edges_grid")}
    ctx.set_option("edges_grid", 0)
    return sweep


def quality(ctx, n, K):
    lists = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
    _, exact, _ = ctx.posterior(*lists, want_sets=False)
    orders, r, _ = record(ctx, lists, K, want_parents=True)
    par = r["parents"].reshape(-1, n)[:K]
    tab, zero = ctx.order_edges(orders, groups=CHAINS)
    counts = [len(range(g, K, CHAINS)) for g in range(CHAINS)]
    rb, rb_se = ulg.order_edge_posterior(tab, counts)
    ind = ((par[:, None, :] >> np.arange(n, dtype=np.uint64)[None, :, None]) & np.uint64(1)).astype(np.float64)  # [k, u, v]
    freq = ind.mean(axis=0)
    per_chain = np.stack([ind[g::CHAINS].mean(axis=0) for g in range(CHAINS)])
    freq_se = per_chain.std(axis=0, ddof=1) / np.sqrt(CHAINS)
    iid = np.sqrt(np.maximum(exact * (1 - exact), 0) / K)

    def worst(est, se):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.where(se > 0, np.abs(est - exact) / se, 0.0).max())

    return {"n": n, "sets": int(lists[0][-1]), "samples": K, "zero": int(zero), "rhat_log_score": ulg.order_rhat(r["log_score"]),
            "sample_mean": {"largest_deviation": float(np.abs(freq - exact).max()), "in_iid_standard_errors": worst(freq, iid),
                            "in_between_chain_standard_errors": worst(freq, freq_se), "largest_between_chain_standard_error": float(freq_se.max()),
                            "sum_of_squared_deviations": float(((freq - exact) ** 2).sum())},
            "rao_blackwell": {"largest_deviation": float(np.abs(rb - exact).max()), "in_iid_standard_errors": worst(rb, iid),
                              "in_between_chain_standard_errors": worst(rb, rb_se), "largest_between_chain_standard_error": float(rb_se.max()),
                              "sum_of_squared_deviations": float(((rb - exact) ** 2).sum())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--orders", type=int, default=10000)
    ap.add_argument("--quality-ns", default="20,25")
    a = ap.parse_args()
    res = {"defaults": {"chains": CHAINS, "burn": BURN, "thin": THIN}, "price": {}, "quality": {}}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    ctx = ulg.Context(0)
    families = {"n25": pr.make_lists(25, "dense", 2525, max_parents=4), "c4like": c4like(),
                "c5like": om.make_lists(32, 3232, max_parents=3).triple()}
    for name, lists in families.items():
        res["price"][name], orders = price(ctx, lists, a.orders)
        print(json.dumps({name: res["price"][name]}), flush=True)
        save()
        if name == "n25":
            res["edges_grid_sweep_n25"] = grid_sweep(ctx, orders)
            print(json.dumps(res["edges_grid_sweep_n25"]), flush=True)
            save()
    for n in [int(x) for x in a.quality_ns.split(",") if x]:
        res["quality"][f"n{n}"] = quality(ctx, n, a.orders)
        print(json.dumps({f"n{n}": res["quality"][f"n{n}"]}), flush=True)
        save()
    ctx.close()


if __name__ == "__main__":
    main()
