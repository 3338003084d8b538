"""First measurement of the discrete BDeu scorer (profiles/r14/disc_bdeu.json).

Workload: disc_bic_profile.py's -- synthetic discrete data, n = 25 variables of
arity 3, N = 10 000 records, seeded, full skeleton, 7 parents (the limit
`score -f BIC` applies at this N, taken here for both scores so that they count
the same tables) -- scored with BDeu (ess = 1) and, in the same process and
alternating with it, with BIC.  The counting pass of the two is identical, so
the ratio of their times is the cost of the lgamma terms.  Reports seconds per
call, sets/s and record visits/s (sets x N) of both and the ratio.  No target:
these are first numbers.

    python scripts/disc_bdeu_profile.py out.json [--repeats 3]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "urlearning-cpp_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import ulg  # noqa: E402
from disc_bic_profile import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--n", type=int, default=25)
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--arity", type=int, default=3)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--ess", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    n, N = a.n, a.records
    limit = min(n - 1, int(math.log(2 * N / math.log(N))))
    codes = synthetic(n, N, a.arity, a.seed)
    ctx = ulg.Context(0)
    ctx.load_discrete(codes, [a.arity] * n)
    ctx.set_ess(a.ess)
    full = [(1 << n) - 1] * n
    kinds = {"bic": ctx.SCORE_BIC, "bdeu": ctx.SCORE_BDEU}
    for kind in kinds.values():
        ctx.score_discrete(list(range(n)), full, 2, kind=kind)  # warm-up: module load, buffers
    runs = {"bic": [], "bdeu": []}
    counts = {}
    for _ in range(a.repeats):
        for name, kind in kinds.items():  # alternating
            t0 = time.perf_counter()
            stored, scored = ctx.score_discrete(list(range(n)), full, limit, kind=kind)  # ends in a synchronise
            runs[name].append(time.perf_counter() - t0)
            counts[name] = (stored, scored, ctx.info("disc_dense_sets"), ctx.info("disc_sparse_sets"))
    ctx.close()
    res = {"workload": {"n": n, "N": N, "arity": a.arity, "seed": a.seed, "skeleton": "full", "parent_limit": limit,
                        "ess": a.ess}}
    for name in kinds:
        best = min(runs[name])
        stored, scored, dense, sparse = counts[name]
        res[name] = {"sets_scored": scored, "sets_stored": stored, "seconds": best, "seconds_all_runs": runs[name],
                     "sets_per_s": scored / best, "record_visits_per_s": scored * N / best,
                     "dense_share": dense / max(dense + sparse, 1)}
    res["bdeu_over_bic"] = res["bdeu"]["seconds"] / res["bic"]["seconds"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
