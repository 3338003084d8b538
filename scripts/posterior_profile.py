"""First measurement of the exact model averaging (profiles/r25/posterior.json).

Workload: ulg_posterior at n = 20 and n = 25 with full lists up to 4 parents
(every subset of at most 4 of the other variables, synthetic scores), host
lists, set_logpost requested.  Per n: one untimed call, then --repeats timed
ones (the best, every repeat), the table bytes, and from one profiled call the
per-kernel split of ulg_profile_*.  For scale: tests/posterior_ref.py's float64
recursion at n = 16 (up to 3 parents) on the host, and the GPU call on the same
lists.  --pytest-log takes the output of `pytest -s` over the GPU tests and adds
the largest observed deviation and the cap per test family
("posterior-observed" lines).

    python scripts/posterior_profile.py out.json [--repeats 3] [--pytest-log file]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "urlearning-cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import posterior_ref as pr  # noqa: E402
import ulg  # noqa: E402


def observed(path):
    """family -> {"max": largest observed, "cap": the cap it was held to, "e64": what float64 numpy loses
    (each the largest over the family's inputs)}."""
    out = {}
    for ln in open(path):
        m = re.search(r"posterior-observed (\S+) (\S+) max (\S+) cap (\S+) e64 (\S+)", ln)
        if m:
            d = out.setdefault(m.group(1), {"max": 0.0, "cap": 0.0, "e64": 0.0, "inputs": 0})
            d["max"] = max(d["max"], float(m.group(3)))
            d["cap"] = max(d["cap"], float(m.group(4)))
            d["e64"] = max(d["e64"], float(m.group(5)))
            d["inputs"] += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ns", default="20,25")
    ap.add_argument("--pytest-log")
    a = ap.parse_args()
    res = {"workload": "ulg_posterior, full lists up to 4 parents, host lists, set_logpost requested", "calls": {}}
    ctx = ulg.Context(0)
    for n in [int(x) for x in a.ns.split(",")]:
        offs, sets, scores = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
        lz, edge, lp = ctx.posterior(offs, sets, scores)  # untimed: allocations
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ctx.posterior(offs, sets, scores)
            times.append(time.perf_counter() - t0)
        ctx.profile(True)
        ctx.profile_reset()
        ctx.posterior(offs, sets, scores)
        split = {k: v for k, v in ctx.profile_dump().items() if k.startswith("post_")}
        ctx.profile(False)
        res["calls"][f"n{n}"] = {"n": n, "sets": int(len(sets)), "seconds_best": min(times), "seconds": times,
                                 "posterior_bytes": ctx.info("posterior_bytes"), "log_z": lz,
                                 "logaddexp_per_transform": n * (n - 1) * 2 ** (n - 2),
                                 "kernel_ms": {k: {"launches": v["count"], "total_ms": v["total_ms"]} for k, v in split.items()},
                                 "kernel_ms_sum": sum(v["total_ms"] for v in split.values())}
        print(json.dumps({f"n{n}": res["calls"][f"n{n}"]["seconds_best"]}), flush=True)
    n = 16
    offs, sets, scores = pr.make_lists(n, "dense", 1600, max_parents=3)
    t0 = time.perf_counter()
    ref = pr.lattice(n, offs, sets, scores, dtype=np.float64, tables=False)
    t_ref = time.perf_counter() - t0
    ctx.posterior(offs, sets, scores)
    t0 = time.perf_counter()
    lz, edge, lp = ctx.posterior(offs, sets, scores)
    t_gpu = time.perf_counter() - t0
    res["scale_n16"] = {"sets": int(len(sets)), "numpy_float64_seconds": t_ref, "gpu_seconds": t_gpu,
                        "log_z_gpu_minus_numpy": float(lz - ref["log_z"])}
    ctx.close()
    if a.pytest_log:
        res["observed"] = observed(a.pytest_log)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"scale_n16": res["scale_n16"]}))


if __name__ == "__main__":
    main()
