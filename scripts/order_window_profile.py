"""First measurement of the window re-optimisation (profiles/r35/order_window.json).

1. Rate.  One sweep of ulg_order_window (max_sweeps = 1, the default stride) over the
   best orders of 500 search steps, 256 and 1024 orders, widths 6, 8, 10 and 12, on the
   three list families of scripts/order_search_profile.py, beside ulg_order_search_run
   of the same build: the wall clock of a call that ends in a synchronise (the window
   call's includes its copies of the orders in and the six outputs back).  The calls are
   timed in alternation, REPEATS times each after an untimed one; median, least and
   largest are kept.  The list entries of a sweep are the lengths of the lists of every
   window of the input orders (a window accepted earlier in the sweep may change which
   variables a later one holds: an estimate).
2. "window_waves": the same call on n25, 256 orders, widths 8 and 12, at every value,
   in alternation.
3. Outcome.  The command line's defaults (256 searches, 20 n^2 steps, tenure n / 2,
   patience 4 n; untuned) followed by --window 8 and 12, --rounds 1 and 3, as
   host/ordersearch_main.cpp runs them: the gap to ulg_astar's GPU optimum at n = 20
   and 25, the best score at c5like (n = 32).

    python scripts/order_window_profile.py out.json [resource-usage.txt]

The optional second file is the compiler's -Rpass-analysis=kernel-resource-usage remarks
for csrc/order_window.hip (`make resource-usage`); its figures are copied in.
"""
import json
import os
import re
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
from order_search_profile import defaults  # noqa: E402

REPEATS = 5
WIDTHS = (6, 8, 10, 12)


def spread(times):
    return {"seconds": times, "median": statistics.median(times), "least": min(times), "largest": max(times)}


def sweep_entries(offs, orders, w):
    """List entries one sweep of every order scans: the lists of each window's variables."""
    length, n = np.diff(np.asarray(offs)), orders.shape[1]
    w = min(w, n)
    stride, a, starts = min(max(1, w // 2), w), 0, [0]
    while a != n - w:
        a = min(a + stride, n - w)
        starts.append(a)
    return int(sum(length[orders[:, a:a + w]].sum() for a in starts)), len(starts)


def rate(lists, C, steps):
    offs, sets, scores = lists
    n = len(offs) - 1
    ctx = ulg.Context(0)
    try:
        ctx.order_search_begin(offs, sets, scores, C, seed=1, **defaults(n))
        orders = ctx.order_search_run(500)["best_order"]
        for w in WIDTHS:
            ctx.order_window(orders, w, 0, 1)  # untimed: the code objects, the buffers
        tw, ts = {w: [] for w in WIDTHS}, []
        for _ in range(REPEATS):
            for w in WIDTHS:
                t0 = time.perf_counter()
                r = ctx.order_window(orders, w, 0, 1)
                tw[w].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.order_search_run(steps)
            ts.append(time.perf_counter() - t0)
        out = {"orders": C, "search_steps": steps, "search_seconds_per_step": spread([t / steps for t in ts]), "widths": {}}
        for w in WIDTHS:
            entries, windows = sweep_entries(offs, orders, w)
            s = spread(tw[w])
            out["widths"][str(w)] = {"seconds_per_sweep": s, "windows_per_sweep": windows, "entries_per_sweep": entries,
                                     "entries_per_second_median": entries / s["median"],
                                     "sweep_over_search_step": s["median"] / out["search_seconds_per_step"]["median"]}
        del r
    finally:
        ctx.close()
    return out


def waves(lists, C=256):
    offs, sets, scores = lists
    n = len(offs) - 1
    ctx = ulg.Context(0)
    try:
        ctx.order_search_begin(offs, sets, scores, C, seed=1, **defaults(n))
        orders = ctx.order_search_run(500)["best_order"]
        t = {(w, W): [] for w in (8, 12) for W in (1, 2, 4, 8, 16)}
        for rep in range(REPEATS + 1):
            for (w, W), ts in t.items():
                ctx.set_option("window_waves", W)
                t0 = time.perf_counter()
                ctx.order_window(orders, w, 0, 1)
                if rep:
                    ts.append(time.perf_counter() - t0)
    finally:
        ctx.close()
    return {f"w{w}_waves{W}": spread(ts) for (w, W), ts in t.items()}


def outcome(lists, width, rounds, C=256):
    """host/ordersearch_main.cpp's --window width --rounds rounds with its defaults, seed 1."""
    offs, sets, scores = lists
    n = len(offs) - 1
    steps = 20 * n * n
    ctx = ulg.Context(0)
    try:
        t0 = time.perf_counter()
        ctx.order_search_begin(offs, sets, scores, C, seed=1, **defaults(n))
        r = ctx.order_search_run(steps)
        before_first = float(r["best_score"].max())
        orders, accepted, window_s = r["best_order"], 0, 0.0
        for k in range(rounds):
            if k:
                ctx.order_search_begin(offs, sets, scores, C, seed=1 + k, init_order=orders, **defaults(n))
                r = ctx.order_search_run(steps)
                orders = r["best_order"]
            before = float(r["best_score"].max())
            w0 = time.perf_counter()
            win = ctx.order_window(orders, width)
            window_s += time.perf_counter() - w0
            orders, accepted = win["orders"], accepted + int(win["accepted"].sum())
        wall = time.perf_counter() - t0
    finally:
        ctx.close()
    best = float(win["score"].max())
    return {"width": width, "rounds": rounds, "best_score": best, "orders_at_best": int((win["score"] == best).sum()),
            "best_before_first_window": before_first, "best_before_last_window": before, "windows_accepted": accepted,
            "sweeps_last_max": int(win["sweeps"].max()), "seconds": wall, "seconds_in_windows": window_s}, win["score"]


def optimum(lists):
    offs, sets, scores = lists
    n = len(offs) - 1
    ctx = ulg.Context(0)
    try:
        ctx.search_load_scores(offs, sets, scores)
        vpar = ctx.astar(mode=1, net_text=False)["vpar"]
    finally:
        ctx.close()
    opt = 0.0  # from its parent sets on the lists, in FP64 (the search's cost is FP32)
    for v in range(n):
        S = np.asarray(sets[offs[v]:offs[v + 1]], dtype=np.uint64)
        opt += float(np.asarray(scores[offs[v]:offs[v + 1]], dtype=np.float64)[np.flatnonzero(S == np.uint64(vpar[v]))[0]])
    return opt


def main():
    out = sys.argv[1]
    res = {"repeats": REPEATS, "rate": {}, "window_waves_n25": {}, "outcome": {}}
    if len(sys.argv) > 2:
        text = open(sys.argv[2]).read()
        res["resources"] = [dict(zip(("kernel", "vgprs", "scratch_bytes_per_lane", "occupancy", "static_lds_bytes"), (m[0],) + tuple(map(int, m[1:]))))
                            for m in re.findall(r"Function Name: (\S*owindow\S*).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                                                r"Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", text, re.S)]
    c5like = om.make_lists(32, 3232, max_parents=3).triple()
    n25 = pr.make_lists(25, "dense", 2525, max_parents=4)
    families = {"n25": (n25, 200), "c5like": (c5like, 400), "c4like": (c4like(), 4000)}
    for name, (lists, steps) in families.items():
        res["rate"][name] = {"n": len(lists[0]) - 1, "sets": int(lists[0][-1]), "runs": [rate(lists, C, steps) for C in (256, 1024)]}
        print(json.dumps({name: res["rate"][name]}), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    res["window_waves_n25"] = waves(n25)
    print(json.dumps(res["window_waves_n25"]), flush=True)
    cases = {"n20": pr.make_lists(20, "dense", 2520, max_parents=4), "n25": pr.make_lists(25, "dense", 2525, max_parents=4), "c5like": c5like}
    for name, lists in cases.items():
        opt = optimum(lists) if name != "c5like" else None
        runs = []
        for width in (8, 12):
            for rounds in (1, 3):
                o, score = outcome(lists, width, rounds)
                if opt is not None:
                    o["gap"] = opt - o["best_score"]
                    o["orders_within_1e-9_of_optimum"] = int((np.abs(score - opt) <= 1e-9 * abs(opt)).sum())
                runs.append(o)
        res["outcome"][name] = {"n": len(lists[0]) - 1, "optimum": opt, "runs": runs}
        print(json.dumps(res["outcome"][name]), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
