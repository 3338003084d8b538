"""First measurement of the tempered ladders (profiles/r32/order_mc3.json).

(a) Throughput.  ulg_order_mc3_run without records for (ladders, rungs) = (256, 4) and (64, 16) at every
    "mc3_waves", against ulg_order_mcmc_run with as many independent chains (1024) at every "mcmc_waves",
    on the three list families of scripts/order_mcmc_profile.py.  Every configuration has a context of its
    own, begun and warmed once; the timed repeats are interleaved (one call of each configuration per
    round), a call ends in a synchronise, and the figure is replica-steps per second of the fastest repeat
    with all repeats kept.  The spread of the baseline's repeats is the yardstick for "slower".
(b) What it buys.  The n = 20 and n = 25 probe lists, whose exact edge matrix ulg_posterior gives: 256
    chains (burn 5000, thin 100, 40 records each) against 64 ladders of 4 rungs (geometric betas down to
    0.1, an exchange round every 10 steps; burn 5000, thin 25, 160 records each): 9000 steps per replica
    and 10240 cold records either way.  R-hat, acceptance per rung, swap acceptance per pair, the worst
    edge in standard errors of independent draws, and the summed squared error of the sampled edge
    frequencies (-o) and of the Rao-Blackwellised matrix (--rb-edges) against the exact one.

    python scripts/order_mc3_profile.py out.json [--repeats 3] [--part a|b|ab]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from order_mcmc_profile import c4like, om, pr, ulg  # noqa: E402  (it sets the paths)

QUIET = dict(want_order=False, want_score=False, want_parents=False)


def throughput(lists, steps, repeats):
    offs, sets, scores = lists
    runs = []
    for waves in (1, 2, 4, 8):
        c = ulg.Context(0)
        c.set_option("mcmc_waves", waves)
        c.order_mcmc_begin(offs, sets, scores, 1024, seed=1)
        runs.append(dict(kind="chains", replicas=1024, waves=waves, ctx=c, call=c.order_mcmc_run, seconds=[]))
    for L, R in ((256, 4), (64, 16)):
        for waves in (1, 2, 4, 8, 16):
            c = ulg.Context(0)
            c.set_option("mc3_waves", waves)
            c.order_mc3_begin(offs, sets, scores, L, ulg.geometric_betas(R, 0.1), swap_every=10, seed=1)
            runs.append(dict(kind=f"ladders {L}x{R}", replicas=L * R, waves=waves, ctx=c, call=c.order_mc3_run, seconds=[]))
    for r in runs:
        r["call"](max(steps // 10, 1), 1, **QUIET)  # untimed: the code object, the lists into the caches
    for _ in range(repeats):
        for r in runs:
            t0 = time.perf_counter()
            r["call"](steps, 1, **QUIET)
            r["seconds"].append(time.perf_counter() - t0)
    out = []
    for r in runs:
        r.pop("ctx").close()
        r.pop("call")
        r.update(steps=steps, replica_steps_per_second=r["replicas"] * steps / min(r["seconds"]),
                 spread=(max(r["seconds"]) - min(r["seconds"])) / min(r["seconds"]))
        out.append(r)
    return out


def errors(ctx, r, exact, n):
    K = r["order"].shape[0] * r["order"].shape[1]
    par = r["parents"].reshape(-1, n)
    freq = np.array([[float((((par[:, v] >> np.uint64(u)) & np.uint64(1)) == 1).mean()) for v in range(n)] for u in range(n)])
    tab, zero = ctx.order_edges(r["order"].reshape(-1, n), groups=1)
    rb = ulg.order_edge_posterior(tab, K - zero)
    se = np.sqrt(np.maximum(exact * (1 - exact), 0) / K)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(se > 0, np.abs(freq - exact) / se, 0.0)
    return {"cold_records": K, "rhat_log_score": ulg.order_rhat(r["log_score"]), "worst_edge_in_standard_errors": float(z.max()),
            "worst_edge_deviation": float(np.abs(freq - exact).max()), "sse_sampled_edges": float(((freq - exact) ** 2).sum()),
            "sse_rb_edges": float(((rb - exact) ** 2).sum()), "worst_rb_edge_deviation": float(np.abs(rb - exact).max())}


def quality(ctx, n):
    offs, sets, scores = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
    _, exact, _ = ctx.posterior(offs, sets, scores, want_sets=False)
    ctx.order_mcmc_begin(offs, sets, scores, 256, seed=1)
    ctx.order_mcmc_run(5000, 100, **QUIET)
    r = ctx.order_mcmc_run(4000, 100)
    chains = dict(errors(ctx, r, exact, n), steps_each=r["step"], acceptance=float(r["accepted"].sum()) / (256 * r["step"]))
    betas, E = ulg.geometric_betas(4, 0.1), 10
    ctx.order_mc3_begin(offs, sets, scores, 64, betas, swap_every=E, seed=1)
    ctx.order_mc3_run(5000, 25, **QUIET)
    r = ctx.order_mc3_run(4000, 25)
    tried = np.array([(r["step"] // E + (p % 2)) // 2 for p in range(3)])
    ladders = dict(errors(ctx, r, exact, n), steps_each=r["step"], betas=[float(b) for b in betas], swap_every=E,
                   acceptance_by_rung=[float(x) for x in r["accepted"].mean(axis=0) / r["step"]],
                   swap_acceptance_by_pair=[float(x) for x in r["swaps"].mean(axis=0) / tried])
    return {"n": n, "sets": int(len(sets)), "replica_steps": 256 * 9000, "chains_256": chains, "ladders_64x4": ladders}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--part", default="ab")
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}

    def save():
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if "a" in a.part:
        families = {"n25": (pr.make_lists(25, "dense", 2525, max_parents=4), 200), "c4like": (c4like(), 4000),
                    "c5like": (om.make_lists(32, 3232, max_parents=3).triple(), 400)}
        for name, (lists, steps) in families.items():
            res.setdefault("throughput", {})[name] = {"n": len(lists[0]) - 1, "sets": int(lists[0][-1]), "runs": throughput(lists, steps, a.repeats)}
            for r in res["throughput"][name]["runs"]:
                print(json.dumps({name: r}), flush=True)
            save()
    if "b" in a.part:
        ctx = ulg.Context(0)
        for n in (20, 25):
            res.setdefault("quality", {})[f"n{n}"] = quality(ctx, n)
            print(json.dumps(res["quality"][f"n{n}"]), flush=True)
            save()
        ctx.close()


if __name__ == "__main__":
    main()
