"""First measurement of the order search over candidate-set tables (profiles/r36/order_tables.json).

On the three list families of scripts/order_search_profile.py, 1024 searches, the command
line's default tenure and patience, no traces:
1. Rate.  ulg_order_search_run with option "search_tables" beside the same build's list path,
   in two contexts timed in alternation, REPEATS times each after an untimed call: steps per
   second over the wall clock of a call that ends in a synchronise; median, least, largest.
   The two must also agree bit for bit on the best scores.  A family the tables refuse (a
   variable with more than 26 candidate parents) is recorded with the refusal's text.
2. Begin.  The wall clock of ulg_order_search_begin with and without the tables' build,
   alternated likewise, and the tables' bytes.

    python scripts/order_tables_profile.py out.json [family ..]

With ULG_LIB set to another build's library only the list path is timed (the parent commit's,
for the run-to-run spread).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "urlearning-cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import order_mcmc_ref as om  # noqa: E402
import posterior_ref as pr  # noqa: E402
import ulg  # noqa: E402
from order_mcmc_profile import c4like  # noqa: E402

REPEATS = 5
SEARCHES = 1024
OTHER_BUILD = "ULG_LIB" in os.environ


def spread(times, work):
    rates = sorted(work / t for t in times)
    return {"seconds": times, "steps_per_second_median": statistics.median(rates), "least": rates[0], "largest": rates[-1]}


def begin(ctx, lists, tables):
    offs, sets, scores = lists
    n = len(offs) - 1
    kw = {} if OTHER_BUILD else {"tables": tables}
    t0 = time.perf_counter()
    ctx.order_search_begin(offs, sets, scores, SEARCHES, seed=1, tenure=n // 2, patience=4 * n, **kw)
    return time.perf_counter() - t0


def family(lists, steps):
    offs = lists[0]
    out = {"n": len(offs) - 1, "sets": int(offs[-1]), "searches": SEARCHES, "steps": steps}
    paths = {"lists": ulg.Context(0)}
    try:
        begin(paths["lists"], lists, False)
        if not OTHER_BUILD:
            paths["tables"] = ulg.Context(0)
            try:
                begin(paths["tables"], lists, True)
            except ulg.ULGError as e:
                out["tables_refused"] = str(e)
                paths.pop("tables").close()
        if "tables" in paths:
            K = [bin(paths["tables"].order_search_table(v)[0]).count("1") for v in range(out["n"])]
            out["K_max"], out["table_bytes"] = max(K), int(sum(8 << k for k in K))
        times, last = {k: [] for k in paths}, {}
        for ctx in paths.values():
            ctx.order_search_run(500)  # untimed: the code object, the caches, and off the initial ascent
        for _ in range(REPEATS):
            for k, ctx in paths.items():
                t0 = time.perf_counter()
                last[k] = ctx.order_search_run(steps)
                times[k].append(time.perf_counter() - t0)
        out["run"] = {k: spread(t, SEARCHES * steps) for k, t in times.items()}
        if "tables" in paths:
            out["same_bits"] = last["tables"]["best_score"].tobytes() == last["lists"]["best_score"].tobytes()
            out["tables_over_lists"] = out["run"]["tables"]["steps_per_second_median"] / out["run"]["lists"]["steps_per_second_median"]
            tb = {"lists": [], "tables": []}
            for _ in range(3):
                tb["lists"].append(begin(paths["lists"], lists, False))
                tb["tables"].append(begin(paths["tables"], lists, True))
            out["begin_seconds"] = tb
    finally:
        for ctx in paths.values():
            ctx.close()
    return out


def main():
    out, want = sys.argv[1], sys.argv[2:]
    # steps: the table path's timed call lasts a tenth of a second or more (n25: 4 x the command line's default of 20 n^2)
    families = {"n25": (lambda: pr.make_lists(25, "dense", 2525, max_parents=4), 50000),
                "c5like": (lambda: om.make_lists(32, 3232, max_parents=3).triple(), 20000), "c4like": (c4like, 200000)}
    res = {"repeats": REPEATS, "other_build": OTHER_BUILD, "families": {}}
    for name, (make, steps) in families.items():
        if want and name not in want:
            continue
        res["families"][name] = family(make(), steps)
        print(json.dumps({name: res["families"][name]}), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
