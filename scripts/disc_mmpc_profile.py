"""First measurement of the discrete MMPC (profiles/r10/disc_mmpc.json).

Workload: synthetic discrete data, n = 30 variables of arity 3, N = 100 000
records, seeded (column j follows column j - 1 with probability 0.4);
ulg_disc_mmpc at alpha = 0.01, max_cond = 3, min_per_cell = 5.  Reports the tests
performed and skipped, the rounds (launches of the test kernel), wall and kernel
time and record visits/s (tests x N over the kernel time) beside the discrete
scorer's record visits/s of profiles/r8/disc_bic.json, and the time of one
discrete BIC scoring call with and without the resulting skeleton.  The scoring
calls take the parent limit --score-parents (default 4), not the command line's
(int) log(2N / log N) = 9: at 9 the call without a skeleton would score 5e8
sets, about five minutes at the r8 rate.  No target: these are first numbers.

    python scripts/disc_mmpc_profile.py out.json [--repeats 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "urlearning-cpp_amd")
sys.path.insert(0, PKG)
import ulg  # noqa: E402


def synthetic(n, N, arity, seed):
    rng = np.random.default_rng(seed)
    codes = np.zeros((N, n), dtype=np.uint8)
    for j in range(n):
        col = rng.integers(0, arity, size=N)
        if j:
            follow = rng.random(N) < 0.4
            col = np.where(follow, codes[:, j - 1], col)
        codes[:, j] = col
    return codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--arity", type=int, default=3)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--max-cond", type=int, default=3)
    ap.add_argument("--score-parents", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    n, N = a.n, a.records
    codes = synthetic(n, N, a.arity, a.seed)
    ctx = ulg.Context(0)
    ctx.load_discrete(codes, [a.arity] * n)
    ctx.mmpc_discrete(a.alpha, 0, 5)  # warm-up: module load, buffers
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        rows = ctx.mmpc_discrete(a.alpha, a.max_cond, 5)
        runs.append(time.perf_counter() - t0)
    tests, skipped = ctx.info("disc_mmpc_tests"), ctx.info("disc_mmpc_skipped")
    ctx.profile(True)
    ctx.profile_reset()
    ctx.mmpc_discrete(a.alpha, a.max_cond, 5)
    prof = ctx.profile_get("disc_g2") or {"count": 0, "total_ms": float("nan")}
    ctx.profile(False)
    kernel_s = prof["total_ms"] / 1e3
    edges = sum(bin(r).count("1") for r in rows) // 2
    full = [(1 << n) - 1] * n
    cands = ulg.candidates_from_edges(rows, n)
    score = {}
    for label, cs in (("full_skeleton", full), ("mmpc_skeleton", cands)):
        ctx.score_discrete(list(range(n)), cs, 1)
        best = None
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            stored, scored = ctx.score_discrete(list(range(n)), cs, a.score_parents)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        score[label] = {"sets_scored": scored, "sets_stored": stored, "seconds": best}
    ctx.close()
    r8 = os.path.join(ROOT, "profiles", "r8", "disc_bic.json")
    yard = json.load(open(r8))["record_visits_per_s"] if os.path.exists(r8) else None
    res = {
        "workload": {"n": n, "N": N, "arity": a.arity, "seed": a.seed, "alpha": a.alpha, "max_cond": a.max_cond,
                     "min_per_cell": 5},
        "tests_performed": tests, "tests_skipped": skipped, "rounds": prof["count"], "edges": edges,
        "wall_s": min(runs), "wall_s_all_runs": runs, "kernel_s": kernel_s,
        "record_visits_per_s": tests * N / kernel_s if kernel_s > 0 else None,
        "disc_bic_record_visits_per_s_r8": yard,
        "scoring": {"parent_limit": a.score_parents, **score},
    }
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
