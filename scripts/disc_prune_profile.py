"""Measurement of the discrete scorer's prune pass (profiles/r12/disc_prune.json).

Workload: the shape of profiles/r8/disc_bic.json (scripts/disc_bic_profile.py):
n = 25 variables of arity 3, N = 10 000 records, seed 8, full skeleton, the
parent limit of `score -f BIC`, (int) log(2N / log N) = 7.

Every timing is a host clock around a call that ends in a device synchronise,
after a warm-up call of the same shape, in a process of its own per
configuration:
  * ulg_disc_score with option "disc_prune" off, on this build and -- with
    --parent-lib, a libulg.so built from the parent commit -- on the parent's,
    the two alternating, `--rounds` processes each of `--repeats` timed calls.
    The spread is that of the repeated calls of one build;
  * the same call with the option on;
  * the summed disc_prune kernel time of one call (ulg_profile_*, a call of
    its own: the event records are not in the timed calls);
  * sets stored and kept, and for both settings the .pss bytes, the
    ulg_pss_format time and the ulg_search_from_scores time.

    python scripts/disc_prune_profile.py out.json [--parent-lib path/libulg.so]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "urlearning-cpp_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def worker(a):
    import ulg
    from disc_bic_profile import synthetic
    n, N = a.n, a.records
    limit = min(n - 1, int(math.log(2 * N / math.log(N))))
    codes = synthetic(n, N, a.arity, a.seed)
    ctx = ulg.Context(0)
    ctx.load_discrete(codes, [a.arity] * n)
    full = [(1 << n) - 1] * n
    variables = list(range(n))
    if a.worker == "on":
        ctx.set_option("disc_prune", 1)
    ctx.score_discrete(variables, full, limit)  # warm-up: the same shape
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        stored, scored = ctx.score_discrete(variables, full, limit)
        runs.append(time.perf_counter() - t0)
    res = {"lib": ulg.LIB_PATH, "prune": a.worker == "on", "score_s": runs, "stored": stored, "scored": scored,
           "parent_limit": limit}
    if a.detail:
        res["pruned"] = ctx.info("disc_pruned")
        ctx.profile(True)
        ctx.profile_reset()
        ctx.score_discrete(variables, full, limit)
        prof = ctx.profile_dump()
        ctx.profile(False)
        res["kernels_ms"] = prof
        names = [f"V{j}" for j in range(n)]
        nm = ctx._names_arg(names)
        ar = np.ascontiguousarray([a.arity] * n, dtype=np.int32)
        header = f"META pss_version = 0.1\nMETA input_file={a.out}\nMETA num_records={N}\nMETA parent_limit={limit}\n" \
                 f"META score_type=bic\nMETA ess=1\n\n"
        fmt = []
        for _ in range(2):  # the first call sizes the text buffers
            text, ln = C.c_void_p(), C.c_int64()
            t0 = time.perf_counter()
            ctx._check(ulg.lib().ulg_pss_format(ctx._h, header.encode(), C.cast(nm, C.c_void_p), ulg._ptr(ar),
                                               C.byref(text), C.byref(ln)), "ulg_pss_format")
            fmt.append(time.perf_counter() - t0)
        res["pss_format_s"] = fmt
        res["pss_bytes"] = ln.value
        srch = []
        for _ in range(2):
            t0 = time.perf_counter()
            ctx.search_from_scores()
            srch.append(time.perf_counter() - t0)
        res["search_from_scores_s"] = srch
    ctx.close()
    print("RESULT " + json.dumps(res))


def run_worker(a, mode, lib=None, detail=False):
    cmd = [sys.executable, os.path.abspath(__file__), a.out, "--worker", mode, "--n", str(a.n), "--records",
           str(a.records), "--arity", str(a.arity), "--seed", str(a.seed), "--repeats", str(a.repeats)]
    if detail:
        cmd.append("--detail")
    env = dict(os.environ)
    if lib:
        env["ULG_LIB"] = lib
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"worker {mode} ({lib or 'this build'}) failed with {r.returncode}:\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])


def summary(runs):
    return {"median_s": statistics.median(runs), "min_s": min(runs), "max_s": max(runs), "runs_s": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--n", type=int, default=25)
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--arity", type=int, default=3)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--worker", choices=["off", "on"], default=None)
    ap.add_argument("--detail", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    this_off, parent_off = [], []
    for _ in range(a.rounds):  # alternating processes
        if a.parent_lib:
            parent_off += run_worker(a, "off", lib=os.path.abspath(a.parent_lib))["score_s"]
        this_off += run_worker(a, "off")["score_s"]
    off = run_worker(a, "off", detail=True)
    on = run_worker(a, "on", detail=True)
    this_off += off["score_s"]
    prune_ms = on["kernels_ms"].get("disc_prune")
    res = {
        "workload": {"n": a.n, "N": a.records, "arity": a.arity, "seed": a.seed, "skeleton": "full", "function": "BIC",
                     "parent_limit": off["parent_limit"]},
        "method": "host clock around ulg_disc_score (ends in a stream synchronise), one warm-up call per process, "
                  f"{a.repeats} timed calls per process; option off: this build and the parent's alternate",
        "sets_scored": off["scored"], "sets_stored": off["stored"], "sets_kept": on["stored"], "sets_pruned": on["pruned"],
        "disc_score_off_s": summary(this_off),
        "disc_score_off_parent_s": summary(parent_off) if parent_off else "not measured",
        "disc_score_on_s": summary(on["score_s"]),
        "disc_prune_kernels": prune_ms if prune_ms else "not measured",
        "kernels_ms_on": on["kernels_ms"], "kernels_ms_off": off["kernels_ms"],
        "pss_bytes": {"off": off["pss_bytes"], "on": on["pss_bytes"]},
        "pss_format_s": {"off": off["pss_format_s"], "on": on["pss_format_s"]},
        "search_from_scores_s": {"off": off["search_from_scores_s"], "on": on["search_from_scores_s"]},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
