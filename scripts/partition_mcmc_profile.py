"""First measurement of the partition MCMC (profiles/r33/partition_mcmc.json).

1. Rate.  ulg_partition_mcmc_run and ulg_order_mcmc_run of the same build without
   records on the three list families of scripts/order_mcmc_profile.py, 256 and
   1024 chains, default "mcmc_waves": chain-steps per second over the wall clock
   of a call that ends in a synchronise.  The two are timed in alternation,
   REPEATS times each after an untimed call; median, least and largest are kept.
   Beside it the mean |D| of the proposed moves (the variables whose term a
   move recomputes; a no-op counts 0) over 8 chains' steps after 500, made on
   the host from the recorded states by tests/partition_mcmc_ref.py.
2. What the command line's defaults deliver at n = 20 and 25: 256 chains, burn
   5000, thin 100, 10000 samples: acceptance, mean parts, R-hat, wall clock, and
   the largest deviation of the samples' edge frequencies from the exact
   sampler's uniform-prior estimate (ulg.uniform_prior_edges over 100000
   order-modular samples reweighted by 1 / ext, with its ESS).

    python scripts/partition_mcmc_profile.py out.json
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
import partition_mcmc_ref as pm  # noqa: E402
import posterior_ref as pr  # noqa: E402
import ulg  # noqa: E402
from order_mcmc_profile import c4like  # noqa: E402

REPEATS = 5


def spread(times, work):
    rates = sorted(work / t for t in times)
    return {"seconds": times, "steps_per_second_median": statistics.median(rates), "least": rates[0], "largest": rates[-1]}


def rate(lists, chains, steps):
    offs, sets, scores = lists
    part, order = ulg.Context(0), ulg.Context(0)
    try:
        part.partition_mcmc_begin(offs, sets, scores, chains, seed=1)
        order.order_mcmc_begin(offs, sets, scores, chains, seed=1)
        pk = dict(want_part=False, want_score=False, want_parents=False)
        ok = dict(want_order=False, want_score=False, want_parents=False)
        part.partition_mcmc_run(500, 1, **pk)  # untimed: the code object, the caches, and away from the empty DAG
        order.order_mcmc_run(500, 1, **ok)
        tp, to = [], []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            r = part.partition_mcmc_run(steps, 1, **pk)
            tp.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            order.order_mcmc_run(steps, 1, **ok)
            to.append(time.perf_counter() - t0)
        out = {"chains": chains, "steps": steps, "partition": spread(tp, chains * steps), "order": spread(to, chains * steps),
               "partition_acceptance": float(r["accepted"].sum()) / (chains * r["step"])}
    finally:
        part.close()
        order.close()
    return out


def mean_touched(lists, steps=300):
    """The mean |D| of the proposals of 8 chains' steps 501 .. 500 + steps, from the recorded states."""
    offs, sets, scores = lists
    n = len(offs) - 1
    ctx = ulg.Context(0)
    try:
        ctx.partition_mcmc_begin(offs, sets, scores, 8, seed=1)
        ctx.partition_mcmc_run(500, 500, want_score=False, want_parents=False)
        before = ctx.partition_mcmc_state()[0]
        rec = ctx.partition_mcmc_run(steps, 1, want_score=False, want_parents=False)["part"]
    finally:
        ctx.close()
    sizes = []
    for c in range(8):
        state = before[c]
        for s in range(steps):
            t = 501 + s
            parts = pm.from_part_of([int(p) for p in state])
            w = [int(x[0]) for x in om._draw(1, t, [c], 0)]
            x = [int(y[0]) for y in om._draw(1, t, [c], pm.AUX)]
            _, new, _, _ = pm.propose(w, x[2] | (x[3] << 32), parts, n)
            old = pm.pairs(parts, n)
            sizes.append(0 if new is None else sum(a != b for a, b in zip(old, pm.pairs(new, n))))
            state = rec[s, c]
    return float(np.mean(sizes))


def quality(n, K=10000, exact_K=100000):
    offs, sets, scores = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
    chains, burn, thin = 256, 5000, 100
    recs = -(-K // chains)
    ctx = ulg.Context(0)
    try:
        ctx.posterior(offs, sets, scores, want_sets=False)
        par = ctx.posterior_sample(exact_K, seed=1, want_order=False, want_weight=False)[0]
        _, log_ext = ctx.dag_linear_extensions(par)
        exact, ess = ulg.uniform_prior_edges(par, log_ext)
        t0 = time.perf_counter()
        ctx.partition_mcmc_begin(offs, sets, scores, chains, seed=1)
        ctx.partition_mcmc_run(burn, thin, want_part=False, want_score=False, want_parents=False)
        r = ctx.partition_mcmc_run(thin * (burn // thin + recs) - burn, thin)
        wall = time.perf_counter() - t0
    finally:
        ctx.close()
    mine = r["parents"].reshape(-1, n)[:K]
    freq = np.array([[float((((mine[:, v] >> np.uint64(u)) & np.uint64(1)) == 1).mean()) for v in range(n)] for u in range(n)])
    return {"n": n, "sets": int(len(sets)), "chains": chains, "burn": burn, "thin": thin, "samples": K, "steps_each": int(r["step"]),
            "acceptance": float(r["accepted"].sum()) / (chains * r["step"]), "mean_parts": float(r["parts"].mean()),
            "rhat_log_score": ulg.order_rhat(r["log_score"]), "seconds_begin_burn_records": wall,
            "exact_sampler": {"samples": exact_K, "uniform_prior_ess": float(ess)},
            "largest_edge_deviation_from_uniform_edges": float(np.abs(freq - exact).max())}


def main():
    out = sys.argv[1]
    res = {"repeats": REPEATS, "rate": {}, "quality": {}}
    families = {"n25": (pr.make_lists(25, "dense", 2525, max_parents=4), 200), "c5like": (om.make_lists(32, 3232, max_parents=3).triple(), 400),
                "c4like": (c4like(), 4000)}
    for name, (lists, steps) in families.items():
        res["rate"][name] = {"n": len(lists[0]) - 1, "sets": int(lists[0][-1]), "mean_touched_variables_per_step": mean_touched(lists),
                             "order_touched_positions_per_step": (len(lists[0]) + 3) / 3, "runs": [rate(lists, c, steps) for c in (256, 1024)]}
        print(json.dumps({name: res["rate"][name]}), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    for n in (20, 25):
        res["quality"][f"n{n}"] = quality(n)
        print(json.dumps(res["quality"][f"n{n}"]), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
