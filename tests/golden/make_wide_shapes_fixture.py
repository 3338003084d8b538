#!/usr/bin/env python3
"""Generate tests/golden/wide_shapes_oracle.json: the CPU oracle's whole
stored list (ora_score_variable, the literal recursion) of the designed input
m24_all of tests/wide_shapes.py -- 24 strong candidates, k = 24, N = 256,
lambda 2: the largest m >= 21 whose full list the oracle finishes in under
ten minutes (m21_all 53 s, m22_all 109 s, m24_all 549 s; m = 25 doubles that
again).  The inputs with junk candidates are out of its reach: the
literal recursion visits every absent subset of a dominated set.

In the manner of make_c45_fixture.py the fixture keeps the stored-set count,
a SHA-256 of the sorted uint64 masks, the float64 sum of the float32 scores
and every 512th (set, score) pair in sorted-set order.  At 2^24 stored sets
that is 32,768 pairs, so the pairs are kept compactly: the scores as float32
in tests/golden/wide_shapes_oracle_<case>_scores.npy, and the sets not at all,
since the SHA-256 over the whole sorted list already fixes every one of them.

    python tests/golden/make_wide_shapes_fixture.py [case ...]
"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "urlearning-cpp_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import wide_shapes as ws  # noqa: E402

STRIDE = 512


def digest(sets, scores, seconds):
    """-> (the JSON entry, every STRIDE-th score in sorted-set order as float32)"""
    order = np.argsort(sets, kind="stable")
    s, f = np.ascontiguousarray(sets[order], dtype=np.uint64), np.ascontiguousarray(scores[order], dtype=np.float32)
    return {
        "stored": int(len(s)),
        "sets_sha256": hashlib.sha256(s.tobytes()).hexdigest(),
        "score_sum": float(np.sum(f.astype(np.float64))),
        "sample_stride": STRIDE,
        "samples": int(len(f[::STRIDE])),
        "oracle_seconds": round(float(seconds), 1),
    }, np.ascontiguousarray(f[::STRIDE])


def main():
    import oracle
    oracle.build()
    out = {"generator": "tests/golden/make_wide_shapes_fixture.py (oracle ora_score_variable)", "lambda": ws.LAM}
    for name in sys.argv[1:] or ["m24_all"]:
        c = ws.case(name)
        t0 = time.time()
        sets, scores = oracle.Dataset(c.X).score_variable(ws.LAM, c.variables[0], c.cands[0], c.k)
        out[name], sample = digest(sets, scores, time.time() - t0)
        np.save(os.path.join(ROOT, "tests", "golden", f"wide_shapes_oracle_{name}_scores.npy"), sample)
        print(f"{name}: {out[name]['stored']} stored in {out[name]['oracle_seconds']} s", flush=True)
    path = os.path.join(ROOT, "tests", "golden", "wide_shapes_oracle.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
