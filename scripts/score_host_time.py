"""Host side of a warm C3 scoring call (graph replay on): wall time of score(), GPU time of one
profiled step, and the time score_async() takes to return.  usage: host_time.py PKG_DIR LABEL"""
import json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
import ulg, synth
n, N, k = 25, 10000, 6
X, _ = synth.gaussian_sem(n, N, 9200)
ctx = ulg.Context(0)
ctx.load(X, 2.0)
vs, full = list(range(n)), [(1 << n) - 1] * n
for _ in range(10): ctx.score(vs, full, k)
wall, host = [], []
for _ in range(1000):
    t0 = time.perf_counter(); ctx.score(vs, full, k); wall.append(time.perf_counter() - t0)
for _ in range(1000):
    t0 = time.perf_counter(); ctx.score_async(vs, full, k); host.append(time.perf_counter() - t0); ctx.score_finish()
ctx.profile(True); ctx.profile_reset(); ctx.score(vs, full, k); ctx.score(vs, full, k)
d = ctx.profile_dump(); ctx.profile(False)
gpu_ms = sum(v["total_ms"] for v in d.values()) / 2
res = {"label": sys.argv[2], "score_wall_ms_median": 1e3 * float(np.median(wall)), "score_wall_ms_min": 1e3 * float(np.min(wall)),
       "profiled_step_gpu_ms_sum_of_kernels": gpu_ms, "wall_minus_gpu_ms": 1e3 * float(np.median(wall)) - gpu_ms,
       "score_async_return_ms_median": 1e3 * float(np.median(host)), "score_async_return_ms_min": 1e3 * float(np.min(host))}
print(json.dumps(res)); ctx.close()
