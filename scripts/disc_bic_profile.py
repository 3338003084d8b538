"""First measurement of the discrete BIC scorer (profiles/r8/disc_bic.json).

Workload: synthetic discrete data, n = 25 variables of arity 3, N = 10 000
records, seeded; full skeleton (every other variable is a candidate); the
parent limit `score -f BIC` would apply, (int) log(2N / log N) = 7.  Reports
sets scored, seconds, sets/s, record visits/s (sets x N) and the share of sets
on each counting path, plus the wall time of `bin/score -s` on
tests/golden/hepatitis.clean.csv.  No target: these are first numbers.

    python scripts/disc_bic_profile.py out.json [--repeats 2]
"""
import argparse
import json
import math
import os
import subprocess
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
    ap.add_argument("--n", type=int, default=25)
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--arity", type=int, default=3)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    n, N = a.n, a.records
    limit = min(n - 1, int(math.log(2 * N / math.log(N))))
    codes = synthetic(n, N, a.arity, a.seed)
    ctx = ulg.Context(0)
    ctx.load_discrete(codes, [a.arity] * n)
    full = [(1 << n) - 1] * n
    ctx.score_discrete(list(range(n)), full, 2)  # warm-up: module load, buffers
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        stored, scored = ctx.score_discrete(list(range(n)), full, limit)
        runs.append(time.perf_counter() - t0)
    dense, sparse = ctx.info("disc_dense_sets"), ctx.info("disc_sparse_sets")
    ctx.close()
    best = min(runs)
    res = {
        "workload": {"n": n, "N": N, "arity": a.arity, "seed": a.seed, "skeleton": "full", "function": "BIC",
                     "parent_limit": limit},
        "sets_scored": scored, "sets_stored": stored, "seconds": best, "seconds_all_runs": runs,
        "sets_per_s": scored / best, "record_visits_per_s": scored * N / best,
        "dense_share": dense / max(dense + sparse, 1), "sparse_share": sparse / max(dense + sparse, 1),
    }
    hep = os.path.join(ROOT, "tests", "golden", "hepatitis.clean.csv")
    out_pss = a.out + ".hepatitis.pss"
    t0 = time.perf_counter()
    r = subprocess.run([os.path.join(PKG, "bin", "score"), hep, out_pss, "-s"], capture_output=True, text=True)
    wall = time.perf_counter() - t0
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("ulg_metrics ")]
    res["hepatitis_score_s"] = {"command": "bin/score hepatitis.clean.csv out.pss -s", "exit": r.returncode,
                                "wall_s": wall, "metrics": json.loads(line[0][12:]) if line else None}
    if os.path.exists(out_pss):
        os.remove(out_pss)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
