"""First measurement of the BGe scorer (profiles/r24/bge.json).

Workload: the C3 shape -- synth.gaussian_sem(25, 10000, 9200), full skeleton,
6 parents: 25 x C(24, <= 6) = 4,751,275 parent sets.  In one process and
alternating, after one untimed round of each:

  * ulg_bge_score (the templated layer kernels, slot table, compaction);
  * ulg_cbic_score at that shape (lambda = 2);
  * ulg_bge_score_sets over the same 4.75 M pairs (the generic kernel; the call
    also uploads 76 MB of pairs and downloads 19 MB of values).

Reports seconds per call (the best, every repeat, the spread), sets/s, and from
one profiled call of each BGe entry point the summed kernel times (bge_layer,
bge_sets, disc_compact), whose ratio per set is the templated path against the
generic one without the copies.  --resource-usage takes the text of
`make resource-usage` and adds VGPRs, scratch bytes and waves/SIMD per BGe
kernel instance.

    python scripts/bge_profile.py out.json [--repeats 5] [--resource-usage file]
"""
import argparse
import itertools
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "urlearning-cpp_amd")
sys.path.insert(0, PKG)
import synth  # noqa: E402
import ulg  # noqa: E402


def all_pairs(n, k):
    vs, ms = [], []
    for v in range(n):
        others = [p for p in range(n) if p != v]
        for L in range(k + 1):
            if L == 0:
                m = np.zeros(1, dtype=np.uint64)
            else:
                idx = np.array(list(itertools.combinations(others, L)), dtype=np.uint64)
                m = np.sort(np.bitwise_or.reduce(np.uint64(1) << idx, axis=1))  # the scorer's order: (|set|, set value)
            vs.append(np.full(len(m), v, dtype=np.int32))
            ms.append(m)
    return np.concatenate(vs), np.concatenate(ms)


def resource_usage(path):
    """kernel -> {vgprs, scratch_bytes, waves_per_simd} for the BGe kernels of a `make resource-usage` log."""
    out, name = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            t = re.search(r"bge_layer_kernelILi(\d+)E", name)
            name = f"bge_layer_kernel<{t.group(1)}>" if t else ("bge_sets_kernel" if "bge_sets_kernel" in name else None)
            if name:
                out[name] = {}
            continue
        if not name:
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch_bytes", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)")):
            m = re.search(pat, ln)
            if m:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--n", type=int, default=25)
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--parents", type=int, default=6)
    ap.add_argument("--seed", type=int, default=9200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resource-usage")
    a = ap.parse_args()
    n, N, k = a.n, a.records, a.parents
    X, _ = synth.gaussian_sem(n, N, a.seed)
    full = [(1 << n) - 1] * n
    variables = list(range(n))
    vs, ms = all_pairs(n, k)
    ctx = ulg.Context(0)
    ctx.load(X, 2.0)
    res = {"workload": {"n": n, "N": N, "parents": k, "seed": a.seed, "skeleton": "full", "sets": int(len(vs)),
                        "alpha_mu": 1.0, "alpha_w": "default"},
           "library": os.path.relpath(ulg.LIB_PATH, ROOT)}
    calls = {"bge_score": lambda: ctx.score_bge(variables, full, k),
             "cbic_score": lambda: ctx.score(variables, full, k),
             "bge_score_sets": lambda: ctx.score_sets_bge(vs, ms)}
    for f in calls.values():
        f()  # warm-up: module load, buffers, the cBIC launch graph
    runs = {name: [] for name in calls}
    counts = {}
    for _ in range(a.repeats):
        for name, f in calls.items():  # alternating; every call ends in a synchronise
            t0 = time.perf_counter()
            r = f()
            runs[name].append(time.perf_counter() - t0)
            counts[name] = r
    st, sc = counts["bge_score"]
    assert sc == len(vs)
    # the lists against the generic path, once (the cBIC call has replaced them since)
    assert ctx.score_bge(variables, full, k) == (st, sc)
    offs, sets, scores = ctx.fetch(st)
    vals = counts["bge_score_sets"]
    keep = np.isfinite(vals)
    res["lists_equal_score_sets"] = bool(sets.tobytes() == ms[keep].tobytes() and scores.tobytes() == vals[keep].tobytes())
    for name in calls:
        best = min(runs[name])
        res[name] = {"seconds": best, "seconds_all_runs": runs[name], "spread": (max(runs[name]) - best) / best,
                     "sets_per_s": len(vs) / best}
    res["bge_score"].update(stored=st, scored=sc, positive=int((scores > 0).sum()))
    res["cbic_score"].update(stored=counts["cbic_score"][0], scored=counts["cbic_score"][1])
    res["bge_over_cbic"] = res["bge_score"]["seconds"] / res["cbic_score"]["seconds"]
    res["score_sets_over_score"] = res["bge_score_sets"]["seconds"] / res["bge_score"]["seconds"]
    # kernel times of one profiled call each
    ctx.profile(True)
    ctx.profile_reset()
    ctx.score_bge(variables, full, k)
    ctx.score_sets_bge(vs, ms)
    prof = ctx.profile_dump()
    ctx.profile(False)
    ctx.close()
    res["kernels_ms"] = {name: prof[name] for name in ("bge_layer", "bge_sets", "disc_compact") if name in prof}
    if "bge_layer" in prof and "bge_sets" in prof:
        def total(x):
            return x["total_ms"] if isinstance(x, dict) else x
        res["generic_over_templated_kernel_time"] = total(prof["bge_sets"]) / total(prof["bge_layer"])
    if a.resource_usage:
        res["resource_usage"] = resource_usage(a.resource_usage)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
