"""First measurement of the order MCMC (profiles/r30/order_mcmc.json).

1. Rate.  ulg_order_mcmc_run without records on three families of lists, for
   256 and 1024 chains and every "mcmc_waves": steps per second (all chains'
   steps over the wall clock of the call, which ends in a synchronise) and list
   entries visited per second.  An entry is visited once per recomputed term
   (the kernel reads it twice, for the maximum and for the sum): a step visits
   the lists of positions lo .. hi, (n + 4) / 3 of them on average, so entries
   per step = (n + 4) / 3 x the mean list length (exact for equal lists).
     n25      every subset of at most 4 of the other 24 variables (the
              posterior probe's lists, scripts/posterior_profile.py)
     c4like   n = 30, each variable with 3 .. 9 candidate parents and every
              subset of them (a sparse skeleton's lists, as config C4's)
     c5like   n = 32, every subset of at most 3 of the other 31 (a full
              skeleton's lists, as config C5's at k = 3)
   Baseline: tests/order_mcmc_ref.py's numpy restatement on the same n25 lists.
2. What the defaults deliver.  At n = 20 and 25 (the probe's lists): 256 chains,
   burn 5000, thin 100, --quality-samples samples; the largest deviation of the
   samples' edge frequencies from ulg_posterior's exact matrix in standard
   errors sqrt(p (1 - p) / K) (of independent draws, which these are not), with
   R-hat and the acceptance rate; and the wall clock of those calls beside the
   exact path's posterior + sample calls on the same context.

    python scripts/order_mcmc_profile.py out.json [--quality-samples 10000]
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "urlearning-cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import order_mcmc_ref as om  # noqa: E402
import posterior_ref as pr  # noqa: E402
import ulg  # noqa: E402


def c4like(seed=3030):
    rng = np.random.default_rng(seed)
    n = 30
    offs, sets, scores = [0], [], []
    for v in range(n):
        cand = rng.choice([u for u in range(n) if u != v], size=int(rng.integers(3, 10)), replace=False)
        mine = [sum(1 << int(u) for u in c) for r in range(len(cand) + 1) for c in itertools.combinations(cand, r)]
        sets += mine
        scores += list(rng.normal(0.0, 2.0, size=len(mine)) - np.array([bin(S).count("1") for S in mine]))
        offs.append(len(sets))
    return np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32)


def rate(ctx, lists, chains, waves, steps):
    offs, sets, scores = lists
    n = len(offs) - 1
    ctx.set_option("mcmc_waves", waves)
    ctx.order_mcmc_begin(offs, sets, scores, chains, seed=1)
    kw = dict(want_order=False, want_score=False, want_parents=False)
    ctx.order_mcmc_run(max(steps // 10, 1), 1, **kw)  # untimed: the code object, the lists into the caches
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = ctx.order_mcmc_run(steps, 1, **kw)
        times.append(time.perf_counter() - t0)
    per_step = (n + 4) / 3 * (int(offs[-1]) / n)
    best = min(times)
    return {"chains": chains, "mcmc_waves": waves, "steps": steps, "seconds": times, "steps_per_second": chains * steps / best,
            "entries_per_step": per_step, "entries_per_second": chains * steps * per_step / best,
            "acceptance": float(r["accepted"].sum()) / (chains * r["step"])}


def quality(ctx, n, K):
    offs, sets, scores = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
    chains, burn, thin = 256, 5000, 100
    recs = -(-K // chains)
    t0 = time.perf_counter()
    lz, edge, _ = ctx.posterior(offs, sets, scores, want_sets=False)
    t_exact = time.perf_counter() - t0
    t0 = time.perf_counter()
    ctx.posterior_sample(K, seed=1)
    t_sample = time.perf_counter() - t0
    ctx.set_option("mcmc_waves", 4)
    t0 = time.perf_counter()
    ctx.order_mcmc_begin(offs, sets, scores, chains, seed=1)
    t_begin = time.perf_counter() - t0
    t0 = time.perf_counter()
    ctx.order_mcmc_run(burn, thin, want_order=False, want_score=False, want_parents=False)
    t_burn = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = ctx.order_mcmc_run(thin * (burn // thin + recs) - burn, thin)
    t_run = time.perf_counter() - t0
    par = r["parents"].reshape(-1, n)[:K]
    freq = np.array([[float((((par[:, v] >> np.uint64(u)) & np.uint64(1)) == 1).mean()) for v in range(n)] for u in range(n)])
    se = np.sqrt(np.maximum(edge * (1 - edge), 0) / K)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(se > 0, np.abs(freq - edge) / se, 0.0)
    return {"n": n, "sets": int(len(sets)), "chains": chains, "burn": burn, "thin": thin, "samples": K, "records_per_chain": recs,
            "steps_each": int(r["step"]), "acceptance": float(r["accepted"].sum()) / (chains * r["step"]),
            "rhat_log_score": ulg.order_rhat(r["log_score"]), "largest_edge_deviation_in_standard_errors": float(z.max()),
            "largest_edge_deviation": float(np.abs(freq - edge).max()), "log_z_exact": lz,
            "seconds": {"exact_posterior": t_exact, "exact_sample": t_sample, "mcmc_begin": t_begin, "mcmc_burn": t_burn,
                        "mcmc_records": t_run}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--quality-samples", type=int, default=10000)
    ap.add_argument("--quality-ns", default="20,25")
    a = ap.parse_args()
    res = {"rate": {}, "quality": {}}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    ctx = ulg.Context(0)
    families = {"n25": (pr.make_lists(25, "dense", 2525, max_parents=4), 200), "c4like": (c4like(), 4000),
                "c5like": (om.make_lists(32, 3232, max_parents=3).triple(), 400)}
    for name, (lists, steps) in families.items():
        res["rate"][name] = {"n": len(lists[0]) - 1, "sets": int(lists[0][-1]), "runs": []}
        for chains in (256, 1024):
            for waves in (1, 2, 4, 8):
                res["rate"][name]["runs"].append(rate(ctx, lists, chains, waves, steps))
                print(json.dumps({name: res["rate"][name]["runs"][-1]}), flush=True)
                save()
    # the numpy restatement on the n25 lists: 8 chains, 10 steps
    L = om.Lists(25, *families["n25"][0])
    t0 = time.perf_counter()
    om.run(L, 1, 8, 10, thin=10, want_parents=False)
    res["numpy_reference"] = {"lists": "n25", "chains": 8, "steps": 10, "steps_per_second": 80 / (time.perf_counter() - t0)}
    print(json.dumps(res["numpy_reference"]), flush=True)
    save()
    for n in [int(x) for x in a.quality_ns.split(",") if x]:
        res["quality"][f"n{n}"] = quality(ctx, n, a.quality_samples)
        print(json.dumps({f"n{n}": res["quality"][f"n{n}"]}), flush=True)
        save()
    ctx.close()


if __name__ == "__main__":
    main()
