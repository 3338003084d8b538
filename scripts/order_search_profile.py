"""First measurement of the order search (profiles/r34/order_search.json).

1. Rate.  ulg_order_search_run beside ulg_order_mcmc_run of the same build, without
   traces or records, on the three list families of scripts/order_mcmc_profile.py, 256
   and 1024 searches / chains, default "mcmc_waves": steps per second over the wall
   clock of a call that ends in a synchronise.  The two are timed in alternation,
   REPEATS times each after an untimed call; median, least and largest are kept.
   Beside it the list entries a search step visits: the lengths of the lists its at
   most four scans stride, from a traced run's positions, per second at the median.
2. What the command line's defaults (256 searches, 20 n^2 steps, tenure n / 2,
   patience 4 n; untuned) deliver at n = 20 and 25 against the optimum of ulg_astar's
   GPU mode on the same lists -- the gap and the searches that reach it -- and at
   c5like (n = 32), where there is no optimum: the best score, the searches that share
   it, the wall clock.

    python scripts/order_search_profile.py out.json
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


def spread(times, work):
    rates = sorted(work / t for t in times)
    return {"seconds": times, "steps_per_second_median": statistics.median(rates), "least": rates[0], "largest": rates[-1]}


def defaults(n):
    return dict(tenure=n // 2, patience=4 * n)


def visited_per_step(lists, steps=300):
    """Mean list entries one search step scans: swaps p-1 and p+1 of the applied position, both sides."""
    offs, sets, scores = lists
    n = len(offs) - 1
    length = np.diff(np.asarray(offs))
    ctx = ulg.Context(0)
    try:
        ctx.order_search_begin(offs, sets, scores, 8, seed=1, **defaults(n))
        ctx.order_search_run(500)
        order = ctx.order_search_state()[0].astype(np.int64)
        pos = ctx.order_search_run(steps, trace=True)["trace_pos"]
    finally:
        ctx.close()
    # the kicks' full work lists are left out: an undercount by 3 n - 2 scans per kick
    total, count = 0, 0
    for c in range(8):
        o = list(order[c])
        for s in range(steps):
            p = int(pos[s, c])
            if p == 255:
                continue
            o[p], o[p + 1] = o[p + 1], o[p]
            for q in (p - 1, p + 1):
                if 0 <= q < n - 1:
                    total += int(length[o[q]] + length[o[q + 1]])
            count += 1
    return total / max(count, 1)


def rate(lists, C, steps):
    offs, sets, scores = lists
    n = len(offs) - 1
    search, order = ulg.Context(0), ulg.Context(0)
    try:
        search.order_search_begin(offs, sets, scores, C, seed=1, **defaults(n))
        order.order_mcmc_begin(offs, sets, scores, C, seed=1)
        ok = dict(want_order=False, want_score=False, want_parents=False)
        search.order_search_run(500)  # untimed: the code object, the caches, and off the initial ascent
        order.order_mcmc_run(500, 1, **ok)
        ts, to = [], []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            r = search.order_search_run(steps)
            ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            order.order_mcmc_run(steps, 1, **ok)
            to.append(time.perf_counter() - t0)
        out = {"searches": C, "steps": steps, "search": spread(ts, C * steps), "order_mcmc": spread(to, C * steps),
               "moves_per_step": float(r["moves"].sum()) / (C * r["step"]), "kicks": int(r["kicks"].sum())}
    finally:
        search.close()
        order.close()
    return out


def run_defaults(lists, C=256):
    offs, sets, scores = lists
    n = len(offs) - 1
    ctx = ulg.Context(0)
    try:
        t0 = time.perf_counter()
        ctx.order_search_begin(offs, sets, scores, C, seed=1, **defaults(n))
        r = ctx.order_search_run(20 * n * n)
        wall = time.perf_counter() - t0
    finally:
        ctx.close()
    best = float(r["best_score"].max())
    return r, {"n": n, "sets": int(len(sets)), "searches": C, "steps": 20 * n * n, **defaults(n), "best_score": best,
               "searches_at_best": int((r["best_score"] == best).sum()), "moves": int(r["moves"].sum()), "kicks": int(r["kicks"].sum()),
               "seconds_begin_and_run": wall}


def quality(n):
    lists = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
    offs, sets, scores = lists
    r, out = run_defaults(lists)
    ctx = ulg.Context(0)
    try:
        ctx.search_load_scores(offs, sets, scores)
        t0 = time.perf_counter()
        vpar = ctx.astar(mode=1, net_text=False)["vpar"]
        out["seconds_astar_gpu"] = time.perf_counter() - t0
    finally:
        ctx.close()
    # the optimum's score from its parent sets on the lists, in FP64 (the search's cost is FP32)
    opt = 0.0
    for v in range(n):
        S = np.asarray(sets[offs[v]:offs[v + 1]], dtype=np.uint64)
        opt += float(np.asarray(scores[offs[v]:offs[v + 1]], dtype=np.float64)[np.flatnonzero(S == np.uint64(vpar[v]))[0]])
    out["optimum"] = opt
    out["gap"] = opt - out["best_score"]
    out["searches_within_1e-9_of_optimum"] = int((np.abs(r["best_score"] - opt) <= 1e-9 * abs(opt)).sum())
    return out


def main():
    out = sys.argv[1]
    res = {"repeats": REPEATS, "rate": {}, "quality": {}}
    c5like = om.make_lists(32, 3232, max_parents=3).triple()
    families = {"n25": (pr.make_lists(25, "dense", 2525, max_parents=4), 200), "c5like": (c5like, 400), "c4like": (c4like(), 4000)}
    for name, (lists, steps) in families.items():
        visited = visited_per_step(lists)
        runs = [rate(lists, C, steps) for C in (256, 1024)]
        for r in runs:
            r["entries_visited_per_second_median"] = visited * r["search"]["steps_per_second_median"]
        res["rate"][name] = {"n": len(lists[0]) - 1, "sets": int(lists[0][-1]), "entries_visited_per_step": visited, "runs": runs}
        print(json.dumps({name: res["rate"][name]}), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    for n in (20, 25):
        res["quality"][f"n{n}"] = quality(n)
        print(json.dumps(res["quality"][f"n{n}"]), flush=True)
    res["quality"]["c5like"] = run_defaults(c5like)[1]
    print(json.dumps(res["quality"]["c5like"]), flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
