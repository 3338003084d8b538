"""First measurement of the structural features (profiles/r29/dagfeat.json).

Workload: ulg_dag_features at n = 16, 20 and 25 on K = 10^5 DAGs drawn by the
sampler from the posterior probe's lists (scripts/posterior_profile.py: every
subset of at most 4 of the other variables).  Per n: Context.dag_features with
all five tables, one untimed call and --repeats timed ones (wall clock of the
whole call: upload of 8 n K bytes, kernel, tables back), the kernel's own time
by events from one profiled call, DAGs per second from both, the same with the
integer weights of the uniform prior on the first 1,000 samples' counts
repeated (weights cost one more 8-byte load per DAG), the call with "compelled"
alone and with everything but "compelled" (what the Meek closure costs), and
the grid sweep of option "dagfeat_grid".  Beside it, from the SAME session: the
sampling call that drew the DAGs (ulg_posterior_sample, parents only), timed
the same way -- the yardstick: a reduction slower than the draw would be the
pipeline's bottleneck.  For scale: tests/dagfeat_ref.py's Python reference on
1,000 of the same DAGs.  Once: 200 dense and 200 sparse random DAGs at n = 63
(the global-atomics path).

    python scripts/dagfeat_profile.py out.json [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "urlearning-cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dagfeat_ref as df  # noqa: E402
import posterior_ref as pr  # noqa: E402
import ulg  # noqa: E402


def timed(fn, repeats):
    fn()  # untimed: allocations, first launches
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def kernel_ms(ctx, parents, weight=None, want=ulg.DAG_FEATURES):
    ctx.profile(True)
    ctx.profile_reset()
    ctx.dag_features(parents, weight, want=want)
    d = ctx.profile_dump()
    ctx.profile(False)
    return d.get("dagfeat", {"total_ms": 0.0})["total_ms"]


def call(ctx, parents, repeats, weight=None, want=ulg.DAG_FEATURES):
    K = len(parents)
    t = timed(lambda: ctx.dag_features(parents, weight, want=want), repeats)
    kms = kernel_ms(ctx, parents, weight, want)
    return {"seconds": t, "seconds_best": min(t), "dags_per_second": K / min(t), "grid": ctx.info("dagfeat_grid"),
            "kernel_ms": kms, "kernel_dags_per_second": K / (kms * 1e-3) if kms else None,
            "kernel_ns_per_dag": 1e6 * kms / K}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="16,20,25")
    ap.add_argument("--samples", type=int, default=100000)
    a = ap.parse_args()
    K = a.samples
    res = {"workload": f"ulg_dag_features on {K} sampler draws of the posterior probe's lists (up to 4 parents)", "calls": {}}
    ctx = ulg.Context(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        offs, sets, scores = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
        ctx.posterior(offs, sets, scores, want_sets=False)
        draw = timed(lambda: ctx.posterior_sample(K, seed=n, want_order=False, want_weight=False), a.repeats)
        parents, _, _ = ctx.posterior_sample(K, seed=n, want_order=False, want_weight=False)
        r = {"n": n, "dags": K, "distinct": int(len(np.unique(parents, axis=0))),
             "sample_seconds": draw, "sample_seconds_best": min(draw), "samples_per_second": K / min(draw),
             "all": call(ctx, parents, a.repeats)}
        r["features_over_sampling"] = r["all"]["seconds_best"] / min(draw)
        _, le = ctx.dag_linear_extensions(parents[:1000])
        w = np.tile(ulg.uniform_prior_weights(le) >> np.uint64(8), (K + 999) // 1000)[:K]  # sum below 2^63 at K = 10^5
        r["all_weighted"] = call(ctx, parents, a.repeats, weight=w)
        r["compelled_alone"] = call(ctx, parents, a.repeats, want=("compelled",))
        r["all_but_compelled"] = call(ctx, parents, a.repeats, want=("edge", "ancestor", "blanket", "vstruct"))
        r["total_alone"] = call(ctx, parents, a.repeats, want=())
        sweep = {}
        for grid in (256, 512, 1024, 2048, 4096, 8192):
            ctx.set_option("dagfeat_grid", grid)
            sweep[str(grid)] = kernel_ms(ctx, parents)
        ctx.set_option("dagfeat_grid", 0)
        r["kernel_ms_by_dagfeat_grid"] = sweep
        got = ctx.dag_features(parents[:1000])
        t0 = time.perf_counter()
        want = df.features(n, parents[:1000])
        r["python_reference_seconds_per_1000"] = time.perf_counter() - t0
        r["equal_on_1000"] = bool(got["total"] == want["total"] and all(np.array_equal(got[k], want[k]) for k in ulg.DAG_FEATURES))
        r["python_over_call"] = r["python_reference_seconds_per_1000"] / 1000 * r["all"]["dags_per_second"]
        res["calls"][f"n{n}"] = r
        print(json.dumps({f"n{n}": r}), flush=True)
    rng = np.random.default_rng(63)
    for kind in ("sparse", "dense"):
        dags = np.array([df.random_dag(63, kind, rng) for _ in range(200)], dtype=np.uint64)
        res[f"n63_{kind}_200"] = call(ctx, dags, a.repeats)
        print(json.dumps({f"n63_{kind}_200": res[f"n63_{kind}_200"]}), flush=True)
    ctx.close()
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: {"call_Mdags_per_s": v["all"]["dags_per_second"] / 1e6,
                          "kernel_Mdags_per_s": (v["all"]["kernel_dags_per_second"] or 0.0) / 1e6,
                          "sample_Msamples_per_s": v["samples_per_second"] / 1e6,
                          "features_over_sampling": v["features_over_sampling"]} for k, v in res["calls"].items()}))


if __name__ == "__main__":
    main()
