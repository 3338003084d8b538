"""First measurement of the posterior sampler (profiles/r27/posterior_sample.json).

Workload: ulg_posterior_sample, K = 10^5 samples with order and log weight, on
the posterior probe's lists (scripts/posterior_profile.py: n = 20 and n = 25,
every subset of at most 4 of the other variables).  Per n: one untimed call,
then --repeats timed ones (wall clock of the whole call, the best and every
repeat) and from one profiled call the kernel's own time (post_sample, by
events); the rest of the call is the copy-out (and the 8-byte read of ln Z).
Where the kernel's time goes: the same K on lists of the empty set alone (n
entries in all), where a step is its two table gathers, the Philox draw and the
scans with a one-entry list; the difference to the full lists is the list
scans.  For scale: tests/posterior_sample_ref.py's numpy walk at n = 16 (up to 3
parents) over --ref-samples samples, and the GPU call on the same lists.

    python scripts/posterior_sample_profile.py out.json [--repeats 3] [--samples 100000]
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
import posterior_ref as pr  # noqa: E402
import posterior_sample_ref as ps  # noqa: E402
import ulg  # noqa: E402


def measure(ctx, K, repeats):
    ctx.posterior_sample(K, seed=1)  # untimed: allocations
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ctx.posterior_sample(K, seed=1)
        times.append(time.perf_counter() - t0)
    ctx.profile(True)
    ctx.profile_reset()
    ctx.posterior_sample(K, seed=1)
    kern = ctx.profile_dump().get("post_sample", {"total_ms": float("nan"), "count": 0})
    ctx.profile(False)
    return {"seconds_best": min(times), "seconds": times, "kernel_ms": kern["total_ms"], "kernel_launches": kern["count"],
            "copy_out_and_host_ms": 1e3 * min(times) - kern["total_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--ref-samples", type=int, default=2000)
    ap.add_argument("--ns", default="20,25")
    a = ap.parse_args()
    K = a.samples
    res = {"workload": f"ulg_posterior_sample, K = {K}, order and log weight requested, full lists up to 4 parents", "calls": {}}
    ctx = ulg.Context(0)
    for n in [int(x) for x in a.ns.split(",")]:
        offs, sets, scores = pr.make_lists(n, "dense", 2500 + n, max_parents=4)
        ctx.posterior(offs, sets, scores, want_sets=False)
        full = measure(ctx, K, a.repeats)
        # the empty set alone: gathers, draws and scans without a list to stride
        eo = np.arange(n + 1, dtype=np.int64)
        ctx.posterior(eo, np.zeros(n, dtype=np.uint64), scores[offs[:-1]], want_sets=False)
        bare = measure(ctx, K, a.repeats)
        out_bytes = K * (8 * n + n + 8)
        res["calls"][f"n{n}"] = {"n": n, "sets": int(len(sets)), "entries_per_list": int(offs[1] - offs[0]),
                                 "output_bytes": out_bytes, "full_lists": full, "empty_set_lists": bare,
                                 "list_scan_ms": full["kernel_ms"] - bare["kernel_ms"],
                                 "list_scan_share_of_kernel": 1 - bare["kernel_ms"] / full["kernel_ms"],
                                 "samples_per_second_call": K / full["seconds_best"]}
        print(json.dumps({f"n{n}": res["calls"][f"n{n}"]}), flush=True)
    n = 16
    offs, sets, scores = pr.make_lists(n, "dense", 1616, max_parents=3)
    ctx.posterior(offs, sets, scores, want_sets=False)
    alpha = np.stack([ctx.posterior_table(0, v) for v in range(n)])
    f = ctx.posterior_table(1)
    u = ps.draws(16, 0, a.ref_samples, n)
    t0 = time.perf_counter()
    ref = ps.sample(n, offs, sets, scores, alpha, f, u)
    t_ref = time.perf_counter() - t0
    ctx.posterior_sample(a.ref_samples, seed=16)
    t0 = time.perf_counter()
    got = ctx.posterior_sample(a.ref_samples, seed=16)
    t_gpu = time.perf_counter() - t0
    res["scale_n16"] = {"samples": a.ref_samples, "sets": int(len(sets)), "numpy_reference_seconds": t_ref, "gpu_seconds": t_gpu,
                        "equal": bool(np.array_equal(got[0], ref["parents"]) and np.array_equal(got[1], ref["order"])
                                      and got[2].tobytes() == ref["log_weight"].tobytes()),
                        "undecided_steps": ref["undecided"]}
    ctx.close()
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"scale_n16": res["scale_n16"]}))


if __name__ == "__main__":
    main()
