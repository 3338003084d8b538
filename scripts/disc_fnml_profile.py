"""First measurement of the discrete fNML scorer (profiles/r22/disc_fnml.json).

Workload: disc_bic_profile.py's -- synthetic discrete data, n = 25 variables of
arity 3, N = 10 000 records, seeded, full skeleton, 7 parents (the limit
`score -f BIC` applies at this N, taken here for every score so that they count
the same tables) -- scored with fNML and, in the same process and alternating
with it, with BIC and BDeu (ess = 1).  The counting pass of the three is
identical, so the ratio of fNML's time to BIC's is the cost of one gathered
table load per non-empty parent configuration.  Reports seconds per call (the
best and every repeat), sets/s and record visits/s (sets x N) of each, the
ratios, and the regret table: its bytes and the time of building it (a load,
then ulg_disc_regret of one entry, which launches fnml_regret_kernel and
waits), with the time of the load alone beside it.

--skip-fnml runs BIC and BDeu only: with ULG_LIB set to the parent commit's
libulg.so that is the yardstick for "BIC and BDeu did not move".

    python scripts/disc_fnml_profile.py out.json [--repeats 5] [--skip-fnml]
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-fnml", action="store_true")
    a = ap.parse_args()
    n, N = a.n, a.records
    limit = min(n - 1, int(math.log(2 * N / math.log(N))))
    codes = synthetic(n, N, a.arity, a.seed)
    ctx = ulg.Context(0)
    ctx.set_ess(a.ess)
    full = [(1 << n) - 1] * n
    kinds = {"bic": ctx.SCORE_BIC, "bdeu": ctx.SCORE_BDEU}
    res = {"workload": {"n": n, "N": N, "arity": a.arity, "seed": a.seed, "skeleton": "full", "parent_limit": limit,
                        "ess": a.ess},
           "library": os.path.relpath(ulg.LIB_PATH, ROOT)}
    if not a.skip_fnml:
        kinds["fnml"] = ctx.SCORE_FNML
        # the table: load + build against the load alone, after one untimed round of both
        loads, builds = [], []
        for i in range(a.repeats + 1):
            t0 = time.perf_counter()
            ctx.load_discrete(codes, [a.arity] * n)
            t1 = time.perf_counter()
            assert ctx.info("fnml_table_bytes") == 0
            ctx.regret(a.arity, 0, 1)
            t2 = time.perf_counter()
            if i:
                loads.append(t1 - t0)
                builds.append(t2 - t1)
        res["regret_table"] = {"bytes": ctx.info("fnml_table_bytes"), "rows": 1, "entries_per_row": N + 1,
                               "build_seconds": min(builds), "build_seconds_all_runs": builds,
                               "load_seconds_all_runs": loads}
    ctx.load_discrete(codes, [a.arity] * n)
    for kind in kinds.values():
        ctx.score_discrete(list(range(n)), full, 2, kind=kind)  # warm-up: module load, buffers, the table
    runs = {name: [] for name in kinds}
    counts = {}
    for _ in range(a.repeats):
        for name, kind in kinds.items():  # alternating
            t0 = time.perf_counter()
            stored, scored = ctx.score_discrete(list(range(n)), full, limit, kind=kind)  # ends in a synchronise
            runs[name].append(time.perf_counter() - t0)
            counts[name] = (stored, scored, ctx.info("disc_dense_sets"), ctx.info("disc_sparse_sets"))
    ctx.close()
    for name in kinds:
        best = min(runs[name])
        stored, scored, dense, sparse = counts[name]
        res[name] = {"sets_scored": scored, "sets_stored": stored, "seconds": best, "seconds_all_runs": runs[name],
                     "spread": (max(runs[name]) - best) / best,
                     "sets_per_s": scored / best, "record_visits_per_s": scored * N / best,
                     "dense_share": dense / max(dense + sparse, 1)}
    res["bdeu_over_bic"] = res["bdeu"]["seconds"] / res["bic"]["seconds"]
    if not a.skip_fnml:
        res["fnml_over_bic"] = res["fnml"]["seconds"] / res["bic"]["seconds"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
