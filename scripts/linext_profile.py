"""First measurement of the linear-extension count (profiles/r28/linext.json).

Workload: ulg_dag_linear_extensions at n = 16, 20 and 25 on K = 10^4, 10^3 and
10^2 DAGs drawn by the sampler from the posterior probe's lists
(scripts/posterior_profile.py: every subset of at most 4 of the other
variables), and on the empty graph of each n.  Per n: Context.
dag_linear_extensions with dedupe and without, one untimed call and --repeats
timed ones each (wall clock of the whole call, numpy's unique included), the
share of distinct DAGs, and from one profiled raw call the kernels' own time
(linext_init + linext_layer, by events).  From the kernels' time: 128-bit
gather-adds per second (n 2^(n-1) per DAG, the terms that can count) and the
table bytes they move (16 bytes each, plus 16 per node written).  For scale:
tests/linext_ref.py's Python recursion on one DAG at n = 16.  The raw call again
under "linext_batch" 256, 32 and 4 against the default rule.  End to end:
`posterior --sample 10000` at n = 20 with --uniform and without.

    python scripts/linext_profile.py out.json [--repeats 3]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "urlearning-cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linext_ref as lx  # noqa: E402
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


def kernel_ms(ctx, parents):
    ctx.profile(True)
    ctx.profile_reset()
    ctx.dag_linear_extensions(parents, dedupe=False)
    d = ctx.profile_dump()
    ctx.profile(False)
    return sum(d.get(k, {"total_ms": 0.0})["total_ms"] for k in ("linext_init", "linext_layer")), \
        int(d.get("linext_layer", {"count": 0})["count"])


def case(ctx, n, parents, repeats):
    K = len(parents)
    distinct = len(np.unique(parents, axis=0))
    on = timed(lambda: ctx.dag_linear_extensions(parents), repeats)
    off = timed(lambda: ctx.dag_linear_extensions(parents, dedupe=False), repeats)
    batches = ctx.info("linext_batches")
    kms, launches = kernel_ms(ctx, parents)
    adds = K * n * 2.0 ** (n - 1)
    return {"dags": K, "distinct": distinct, "distinct_share": distinct / K,
            "dedupe_seconds": on, "dedupe_seconds_best": min(on), "dedupe_us_per_dag": 1e6 * min(on) / K,
            "dedupe_dags_per_second": K / min(on),
            "raw_seconds": off, "raw_seconds_best": min(off), "raw_us_per_dag": 1e6 * min(off) / K,
            "raw_dags_per_second": K / min(off), "raw_batches": batches,
            "raw_kernel_ms": kms, "raw_layer_launches": launches, "raw_kernel_us_per_dag": 1e3 * kms / K,
            "table_bytes_per_dag": 16 * 2 ** n,
            "gather_adds_per_second_kernel": adds / (kms * 1e-3),
            "table_read_TBps_kernel": adds * 16 / (kms * 1e-3) / 1e12,
            "table_write_TBps_kernel": K * 16 * 2.0 ** n / (kms * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="16:10000,20:1000,25:100")
    ap.add_argument("--cli-samples", type=int, default=10000)
    a = ap.parse_args()
    res = {"workload": "ulg_dag_linear_extensions on sampler output of the posterior probe's lists (up to 4 parents) "
                       "and on the empty graph", "calls": {}}
    ctx = ulg.Context(0)
    pss20 = None
    for spec in a.cases.split(","):
        n, K = [int(x) for x in spec.split(":")]
        offs, sets, scores = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
        if n == 20:
            pss20 = ctx.pss_format_lists("META pss_version = 0.1\n", [f"v{i}" for i in range(n)], [2] * n, offs, sets, scores)
        ctx.posterior(offs, sets, scores, want_sets=False)
        parents, _, _ = ctx.posterior_sample(K, seed=n, want_order=False, want_weight=False)
        r = {"n": n, "sampled": case(ctx, n, parents, a.repeats),
             "empty_graph": case(ctx, n, np.zeros((1, n), dtype=np.uint64), a.repeats)}
        # the batch size: the default rule against fixed caps (the same integers, other launch counts)
        sweep = {}
        for cap in (0, 256, 32, 4):
            ctx.set_option("linext_batch", cap)
            t = timed(lambda: ctx.dag_linear_extensions(parents, dedupe=False), a.repeats)
            sweep[str(cap)] = {"seconds_best": min(t), "batches": ctx.info("linext_batches")}
        ctx.set_option("linext_batch", 0)
        r["raw_seconds_by_linext_batch"] = sweep
        ext, _ = ctx.dag_linear_extensions(parents[:1])
        r["first_sample_ext"] = str(ext[0])
        res["calls"][f"n{n}"] = r
        print(json.dumps({f"n{n}": r}), flush=True)
        if n == 16:
            par = [int(x) for x in parents[0]]
            t0 = time.perf_counter()
            want = lx.count(n, par)
            res["scale_n16"] = {"python_recursion_seconds_per_dag": time.perf_counter() - t0, "equal": want == ext[0]}
            print(json.dumps({"scale_n16": res["scale_n16"]}), flush=True)
    ctx.close()
    if pss20 is not None:
        exe = os.path.join(ROOT, "urlearning-cpp_amd", "bin", "posterior")
        with tempfile.TemporaryDirectory() as tmp:
            pss = os.path.join(tmp, "n20.pss")
            open(pss, "wb").write(pss20)
            base = [exe, pss, "-o", os.path.join(tmp, "e.csv"), "--sample", str(a.cli_samples), "--seed", "1", "-g",
                    os.path.join(tmp, "d.txt")]

            def run(extra):
                r = subprocess.run(base + extra, capture_output=True, text=True, timeout=280)
                assert r.returncode == 0, r.stderr
                return r.stdout

            plain = timed(lambda: run([]), a.repeats)
            uni = timed(lambda: run(["--uniform", "--uniform-edges", os.path.join(tmp, "u.csv")]), a.repeats)
            out = run(["--uniform"])
            res["cli_n20"] = {"samples": a.cli_samples, "plain_seconds": plain, "uniform_seconds": uni,
                              "plain_seconds_best": min(plain), "uniform_seconds_best": min(uni),
                              "added_seconds": min(uni) - min(plain), "ess_line": out.splitlines()[1]}
            print(json.dumps({"cli_n20": res["cli_n20"]}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: {"raw_us_per_dag": v["sampled"]["raw_us_per_dag"], "dedupe_us_per_dag": v["sampled"]["dedupe_us_per_dag"],
                          "kernel_us_per_dag": v["sampled"]["raw_kernel_us_per_dag"]} for k, v in res["calls"].items()}))


if __name__ == "__main__":
    main()
