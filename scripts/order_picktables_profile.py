"""First measurement of a record's DAG drawn from the order MCMC's tables (profiles/r38/order_picktables.json).

The command line's default run (256 chains, burn 5000, thin 100, 10^4 samples) over the log-sum tables, on
the dense lists of n = 20 and n = 25 (scripts/order_mcmc_tables_profile.py's) and the C4-like lists, with
option "mcmc_table_picks" on and off in two contexts of the same build, timed in alternation, REPEATS times
each after an untimed round; medians with least and largest:
  burn      5000 steps without records;
  records   the steps that give the 10^4 samples with their DAGs (the picks), and the same steps and records
            without parents -- the floor either pick stands on;
  whole     burn + records;
  begin     ulg_order_mcmc_begin with the snapshots and without them, and its kernels' times by the
            library's event timers in one further begin;
  law       n = 20 and 25: the largest deviation of the samples' edge frequencies from ulg_posterior's exact
            matrix, in standard errors, either mode.

    python scripts/order_picktables_profile.py out.json [n20] [n25] [c4like]

With ULG_LIB set to another build's library only the option-off mode is timed (the parent commit's).
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
import posterior_ref as pr  # noqa: E402
import ulg  # noqa: E402
from order_mcmc_profile import c4like  # noqa: E402

REPEATS = 5
OTHER_BUILD = "ULG_LIB" in os.environ
QUIET = dict(want_order=False, want_score=False, want_parents=False)
CHAINS, BURN, THIN, SAMPLES = 256, 5000, 100, 10000


def begin(ctx, lists, picks):
    kw = {} if not picks else {"table_picks": True}
    t0 = time.perf_counter()
    ctx.order_mcmc_begin(*lists, CHAINS, seed=1, tables=True, **kw)
    return time.perf_counter() - t0


def spread(times):
    return {"seconds": times, "median": statistics.median(times), "least": min(times), "largest": max(times)}


def family(lists, exact):
    n = len(lists[0]) - 1
    recs = -(-SAMPLES // CHAINS)
    more = THIN * (BURN // THIN + recs) - BURN
    out = {"n": n, "sets": int(len(lists[1])), "chains": CHAINS, "burn": BURN, "thin": THIN, "samples": SAMPLES}
    edge = None
    if exact:
        ctx = ulg.Context(0)
        _, edge, _ = ctx.posterior(*lists, want_sets=False)
        ctx.close()
    modes = {"off": False} if OTHER_BUILD else {"off": False, "on": True}
    ctxs = {k: ulg.Context(0) for k in modes}
    try:
        t = {k: {"begin": [], "burn": [], "records_with_picks": [], "records_without_parents": [], "whole": []} for k in modes}
        for k, picks in modes.items():  # untimed: the code objects, the allocations
            begin(ctxs[k], lists, picks)
        for _ in range(REPEATS):
            for k, picks in modes.items():
                t[k]["begin"].append(begin(ctxs[k], lists, picks))
        for k, picks in modes.items():  # one more begin with the library's event timers on: its kernels, ms
            ctxs[k].profile(True)
            ctxs[k].profile_reset()
            begin(ctxs[k], lists, picks)
            out.setdefault("begin_kernels_ms", {})[k] = {name: x["total_ms"] for name, x in ctxs[k].profile_dump().items()}
            ctxs[k].profile(False)
        if not OTHER_BUILD:
            K = [bin(ctxs["on"].order_mcmc_table(v)[0]).count("1") for v in range(n)]
            out["K_max"], out["table_bytes"] = max(K), int(sum(8 << k for k in K))
            out["pick_bytes_more"] = int(sum((8 * (max(1, -(-k // 6)) - 1) + 4) << k for k in K))
        last = {}
        for rep in range(REPEATS + 1):  # round 0 is untimed
            for k in modes:
                ctx = ctxs[k]
                t0 = time.perf_counter()
                ctx.order_mcmc_run(BURN, THIN, **QUIET)
                t1 = time.perf_counter()
                last[k] = ctx.order_mcmc_run(more, THIN)
                t2 = time.perf_counter()
                ctx.order_mcmc_run(more, THIN, want_parents=False)
                t3 = time.perf_counter()
                if rep:
                    for name, dt in (("burn", t1 - t0), ("records_with_picks", t2 - t1), ("records_without_parents", t3 - t2),
                                     ("whole", t2 - t0)):
                        t[k][name].append(dt)
        for k in modes:
            res = {name: spread(x) for name, x in t[k].items()}
            res["picks_median"] = res["records_with_picks"]["median"] - res["records_without_parents"]["median"]
            if edge is not None:
                par = last[k]["parents"].reshape(-1, n)[:SAMPLES]
                freq = np.array([[float((((par[:, v] >> np.uint64(u)) & np.uint64(1)) == 1).mean()) for v in range(n)] for u in range(n)])
                se = np.sqrt(np.maximum(edge * (1 - edge), 0) / SAMPLES)
                with np.errstate(divide="ignore", invalid="ignore"):
                    z = np.where(se > 0, np.abs(freq - edge) / se, 0.0)
                res["largest_edge_deviation_in_standard_errors"] = float(z.max())
            out[k] = res
        if "on" in out:
            out["records_on_over_off"] = out["on"]["records_with_picks"]["median"] / out["off"]["records_with_picks"]["median"]
            out["whole_on_over_off"] = out["on"]["whole"]["median"] / out["off"]["whole"]["median"]
    finally:
        for ctx in ctxs.values():
            ctx.close()
    return out


def main():
    out, want = sys.argv[1], sys.argv[2:] or ["n20", "n25", "c4like"]
    res = {"repeats": REPEATS, "other_build": OTHER_BUILD}
    makers = {"n20": lambda: pr.make_lists(20, "dense", 2520, max_parents=4), "n25": lambda: pr.make_lists(25, "dense", 2525, max_parents=4),
              "c4like": c4like}
    for name in want:
        res[name] = family(makers[name](), name != "c4like" and not OTHER_BUILD)
        print(json.dumps({name: res[name]}), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
