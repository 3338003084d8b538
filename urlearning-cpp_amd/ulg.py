"""ctypes binding of libulg.so (include/ulg.h) -- the HIP hot path.

This module is plumbing for tests, bench.py and scripts: every compute call
goes through the C ABI into the gfx950 kernels.  There is no CPU fallback:
if libulg.so is missing, or no HIP device is present, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ULG_LIB", os.path.join(HERE, "libulg.so"))  # ULG_LIB: A/B builds
HEADER = os.path.join(os.path.dirname(HERE), "include", "ulg.h")

_lib = None


class ULGError(RuntimeError):
    pass


def lib():
    """Load libulg.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ULGError(f"{LIB_PATH} not built: run __graft_entry__.build() or make -C urlearning-cpp_amd")
        L = C.CDLL(LIB_PATH)
        P, I, I64, D, F = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_float
        L.ulg_create.argtypes = [C.POINTER(I), I, C.POINTER(P)]
        L.ulg_destroy.argtypes = [P]
        L.ulg_last_error.argtypes = [P]
        L.ulg_last_error.restype = C.c_char_p
        L.ulg_version.restype = C.c_char_p
        L.ulg_cbic_load.argtypes = [P, P, I64, I, D]
        L.ulg_cbic_gram.argtypes = [P, P]
        L.ulg_cbic_score.argtypes = [P, P, I, P, I, C.POINTER(I64), C.POINTER(I64)]
        L.ulg_cbic_score_async.argtypes = [P, P, I, P, I]
        L.ulg_cbic_score_finish.argtypes = [P, C.POINTER(I64), C.POINTER(I64)]
        L.ulg_cbic_fetch.argtypes = [P, P, P, P, I]
        L.ulg_cbic_score_vars.argtypes = [P, P, I, P, I, P, P, P, I64]
        L.ulg_cbic_score_sets.argtypes = [P, I64, P, P, P]
        L.ulg_cbic_set_constraints.argtypes = [P, I, P, P, P]
        L.ulg_disc_load.argtypes = [P, P, I64, I, P]
        L.ulg_disc_score.argtypes = [P, I, P, I, P, I, C.POINTER(I64), C.POINTER(I64)]
        L.ulg_disc_score_sets.argtypes = [P, I, I64, P, P, P]
        L.ulg_disc_set_ess.argtypes = [P, D]
        L.ulg_disc_counts.argtypes = [P, I, C.c_uint64, P, I64, C.POINTER(I64)]
        if hasattr(L, "ulg_disc_regret"):  # ULG_LIB may name a build from before fNML (A/B runs of BIC and BDeu)
            L.ulg_disc_regret.argtypes = [P, I, I64, I64, P]
        if hasattr(L, "ulg_bge_score"):  # ULG_LIB may name a build from before BGe (A/B runs of the benchmark)
            L.ulg_bge_set_prior.argtypes = [P, D, D]
            L.ulg_bge_score.argtypes = [P, P, I, P, I, C.POINTER(I64), C.POINTER(I64)]
            L.ulg_bge_score_sets.argtypes = [P, I64, P, P, P]
        L.ulg_chi2_log_sf.argtypes = [D, D]
        L.ulg_chi2_log_sf.restype = D
        L.ulg_disc_g2.argtypes = [P, I64, P, P, P, P, P, P]
        L.ulg_disc_mmpc.argtypes = [P, D, I, I, P]
        L.ulg_quantize_costs.argtypes = [P, P, P, I64]
        L.ulg_search_load.argtypes = [P, I, P, P, P]
        L.ulg_search_from_scores.argtypes = [P]
        L.ulg_search_load_scores.argtypes = [P, I, P, P, P, I]
        L.ulg_bestscore_query.argtypes = [P, I64, P, P, P, P]
        L.ulg_pdb_build.argtypes = [P, I, C.c_uint64, C.c_uint64]
        L.ulg_pdb_query.argtypes = [P, I64, P, P, P]
        L.ulg_bestscore_table.argtypes = [P, I, C.POINTER(C.c_uint64), P, I64, C.POINTER(I64)]
        L.ulg_pdb_table.argtypes = [P, I, C.POINTER(C.c_uint64), P, I64, C.POINTER(I64)]
        L.ulg_astar.argtypes = [P, P, I, I, P, P, C.POINTER(F), C.POINTER(I64), C.c_char_p, I64]
        L.ulg_triplet_astar.argtypes = [P, P, I, P, P]
        L.ulg_triplet_clusters.argtypes = [P, P, P, I64, C.POINTER(I64)]
        L.ulg_triplet_solve.argtypes = [P, P, I64, I, P, P]
        L.ulg_triplet_memo_put.argtypes = [P, P, I64, I, P]
        L.ulg_mmpc.argtypes = [P, D, I, P]
        L.ulg_mmpc_min_z.argtypes = [P, I64, P, P, P, P, I, P, P]
        L.ulg_pss_format.argtypes = [P, C.c_char_p, P, P, C.POINTER(C.c_void_p), C.POINTER(I64)]
        L.ulg_pss_format_lists.argtypes = [P, I, P, P, P, C.c_char_p, P, P, C.POINTER(C.c_void_p), C.POINTER(I64)]
        L.ulg_astar_scc.argtypes = [P, P, I, I, C.c_uint64, C.c_uint64, P, P, C.POINTER(F), C.POINTER(I64),
                                    C.c_char_p, I64]
        L.ulg_sweep_shard_begin.argtypes = [P, C.c_uint64, C.POINTER(I64)]
        L.ulg_sweep_shard_layer.argtypes = [P, I, P]
        L.ulg_sweep_shard_commit.argtypes = [P, I, P]
        L.ulg_sweep_shard_end.argtypes = [P, P, P, C.POINTER(F), C.POINTER(I64)]
        L.ulg_sweep_leaves.argtypes = [P, P, I64, C.POINTER(I64)]
        # ULG_LIB may name a build from before the model averaging: A/B runs of bench.py against an older
        # library load it through this binding, as for the two guards above; calling a method whose
        # symbol the library lacks still raises
        if hasattr(L, "ulg_posterior"):
            L.ulg_posterior.argtypes = [P, I, P, P, P, I, C.POINTER(D), P, P]
            L.ulg_posterior_from_scores.argtypes = [P, C.POINTER(D), P, P]
            L.ulg_posterior_table.argtypes = [P, I, I, P, I64, C.POINTER(I64)]
        if hasattr(L, "ulg_posterior_sample"):  # ... or from before the sampler
            L.ulg_posterior_sample.argtypes = [P, C.c_uint64, I64, I64, P, P, P]
            L.ulg_posterior_sample_u.argtypes = [P, I64, P, P, P, P]
        if hasattr(L, "ulg_dag_linear_extensions"):  # ... or from before the linear-extension count
            L.ulg_dag_linear_extensions.argtypes = [P, I, I64, P, P, P, P]
        if hasattr(L, "ulg_dag_features"):  # ... or from before the structural features
            L.ulg_dag_features.argtypes = [P, I, I64, P, P, P, P, P, P, P, C.POINTER(C.c_uint64), C.POINTER(I64)]
        if hasattr(L, "ulg_order_mcmc_begin"):  # ... or from before the order MCMC
            L.ulg_order_mcmc_begin.argtypes = [P, I, P, P, P, I, I64, C.c_uint64, P]
            L.ulg_order_mcmc_begin_from_scores.argtypes = [P, I64, C.c_uint64, P]
            L.ulg_order_mcmc_run.argtypes = [P, I64, I64, P, P, P, P, P, P, P, C.POINTER(I64)]
            L.ulg_order_mcmc_state.argtypes = [P, P, P, C.POINTER(I64)]
            L.ulg_order_score.argtypes = [P, I64, P, P]
        if hasattr(L, "ulg_order_edges"):  # ... or from before the Rao-Blackwellised edges
            L.ulg_order_edges.argtypes = [P, I64, P, I64, P, C.POINTER(I64)]
        L.ulg_set_option.argtypes = [P, C.c_char_p, I64]
        L.ulg_get_info.argtypes = [P, C.c_char_p, C.POINTER(I64)]
        L.ulg_profile_enable.argtypes = [P, I]
        L.ulg_profile_get.argtypes = [P, C.c_char_p, C.POINTER(D), C.POINTER(I64), C.POINTER(D)]
        L.ulg_profile_dump.argtypes = [P, C.c_char_p, I64]
        L.ulg_profile_reset.argtypes = [P]
        L.ulg_profile_select.argtypes = [P, C.c_char_p]
        L.ulg_diag_pdb_host.argtypes = [P, C.c_uint64, I, I, P]
        _lib = L
    return _lib


def header_symbols():
    """Every function the C ABI header declares."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(ulg_[a-z0-9_]+)\s*\(", txt)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def chi2_log_sf(x: float, dof: float) -> float:
    """ulg_chi2_log_sf: ln of the chi-square survival function (pure host, no GPU)."""
    return lib().ulg_chi2_log_sf(float(x), float(dof))


def uniform_prior_edges(parents, log_ext):
    """Edge posteriors under the prior uniform over DAGs (of the stored families) from samples of
    the order-modular posterior: the self-normalised importance-sampling estimate with weights
    1 / ext(G_k).  parents uint64 (K, n) as Context.posterior_sample returns them, log_ext float64
    (K) from Context.dag_linear_extensions -> (edge float64 (n, n), ess).
    r_k = exp(min log_ext - log_ext_k); edge[u, v] = sum_k r_k [u in Pa_v^k] / sum_k r_k;
    ess = (sum r)^2 / sum r^2.  Every sum is a float64 sum over k ascending (np.cumsum, not
    np.sum's pairwise order), which `posterior --uniform-edges` repeats term by term.  A count of 0
    (log_ext = -inf) cannot come from the sampler: it raises."""
    p = np.ascontiguousarray(parents, dtype=np.uint64)
    le = np.ascontiguousarray(log_ext, dtype=np.float64)
    if p.ndim != 2 or le.ndim != 1 or p.shape[0] != le.shape[0] or p.shape[0] < 1:
        raise ULGError(f"uniform_prior_edges: parents (K, n) and log_ext (K) with K >= 1, not {p.shape} and {le.shape}")
    if not np.all(np.isfinite(le)):
        raise ULGError("uniform_prior_edges: a sample without a linear extension (log_ext not finite): not a sampled DAG")
    n = p.shape[1]
    r = np.exp(le.min() - le)
    tot = np.cumsum(r)[-1]
    edge = np.zeros((n, n), dtype=np.float64)
    for v in range(n):
        for u in range(n):
            has = ((p[:, v] >> np.uint64(u)) & np.uint64(1)).astype(np.float64)
            edge[u, v] = np.cumsum(r * has)[-1] / tot  # r * 0 = 0 and x + 0 = x: the terms of the members alone
    return edge, float(tot * tot / np.cumsum(r * r)[-1])


def uniform_prior_weights(log_ext):
    """The integer form of uniform_prior_edges' weights, for Context.dag_features: log_ext float64 (K)
    from Context.dag_linear_extensions -> q uint64 (K), q_k = floor(r_k 2^B) with
    r_k = exp(min log_ext - log_ext_k) <= 1 and B = min(52, 62 - ceil(log2 K)), so that
    sum q <= K 2^B < 2^63, the limit of ulg_dag_features.  A sample whose weight is below 2^-B of
    the largest gets q = 0 and drops out of every table and of `total`.  A count of 0
    (log_ext not finite) cannot come from the sampler: it raises."""
    le = np.ascontiguousarray(log_ext, dtype=np.float64)
    if le.ndim != 1 or le.shape[0] < 1:
        raise ULGError(f"uniform_prior_weights: log_ext (K) with K >= 1, not {le.shape}")
    if not np.all(np.isfinite(le)):
        raise ULGError("uniform_prior_weights: a sample without a linear extension (log_ext not finite): not a sampled DAG")
    bits = min(52, 62 - (le.shape[0] - 1).bit_length())  # (K - 1).bit_length() = ceil(log2 K)
    return np.floor(np.ldexp(np.exp(le.min() - le), bits)).astype(np.uint64)


def order_rhat(log_score):
    """Gelman-Rubin's potential scale reduction of Context.order_mcmc_run's "log_score", float64
    (records R, chains C) -> float; NaN for R < 2 or C < 2, or when no chain moved (W = 0).
    m_c = (sum_r x[r, c]) / R, m = (sum_c m_c) / C, W = (sum_c (sum_r (x[r, c] - m_c)^2) / (R - 1)) / C,
    B = R (sum_c (m_c - m)^2) / (C - 1), R-hat = sqrt(((R - 1) / R W + B / R) / W).  Every sum is a
    float64 sum over its index ascending (np.cumsum, not np.sum's pairwise order), which
    `posterior --mcmc` repeats term by term."""
    x = np.ascontiguousarray(log_score, dtype=np.float64)
    if x.ndim != 2:
        raise ULGError(f"order_rhat: log_score must be (records, chains), not {x.shape}")
    R, Cn = x.shape
    if R < 2 or Cn < 2:
        return float("nan")
    mc = np.cumsum(x, axis=0)[-1] / R
    m = np.cumsum(mc)[-1] / Cn
    d = x - mc
    W = np.cumsum(np.cumsum(d * d, axis=0)[-1] / (R - 1))[-1] / Cn
    B = R * np.cumsum((mc - m) * (mc - m))[-1] / (Cn - 1)
    if not W > 0:
        return float("nan")
    return float(np.sqrt(((R - 1) / R * W + B / R) / W))


EDGE_BITS = 40  # ulg_order_edges: an order's edge posterior p is the integer floor(p 2^40)


def order_edge_posterior(edge, counts):
    """The Rao-Blackwellised edge matrix from Context.order_edges' tables: edge uint64 (groups, n, n),
    counts (groups) or a scalar: the orders of each group that count, i.e. those added to it minus its
    orders of probability 0 -> mean float64 (n, n) for one group, (mean, stderr) for two or more.
    mean[u, v] = (sum_g edge[g, u, v]) / (2^40 sum_g counts[g]), the integer sum exact (below 2^62 by the
    call's limit on count), one float64 division.  stderr: with m_g = edge[g] / (2^40 counts[g]) over the
    G >= 2 groups that counted an order, sqrt(sum_g (m_g - mbar)^2 / (G (G - 1))), mbar their plain mean,
    float64 sums over g ascending (np.cumsum), which `posterior --rb-edges` repeats term by term: the
    standard error of the mean across groups (chains), NaN with fewer than two such groups."""
    e = np.ascontiguousarray(edge, dtype=np.uint64)
    if e.ndim == 2:
        e = e[None]
    if e.ndim != 3 or e.shape[1] != e.shape[2]:
        raise ULGError(f"order_edge_posterior: edge must be (groups, n, n), not {e.shape}")
    G, n = e.shape[0], e.shape[1]
    cnt = np.ascontiguousarray(np.broadcast_to(np.asarray(counts, dtype=np.int64), (G,)) if np.ndim(counts) == 0 else counts, dtype=np.int64)
    if cnt.shape != (G,) or np.any(cnt < 0) or cnt.sum() < 1:
        raise ULGError(f"order_edge_posterior: counts must be ({G},), none negative and not all 0")
    if np.any((cnt == 0) & (e.reshape(G, -1).max(axis=1) > 0)):
        raise ULGError("order_edge_posterior: a group without a counted order has a nonzero table")
    total = e.sum(axis=0, dtype=np.uint64)
    mean = total.astype(np.float64) / (float(1 << EDGE_BITS) * float(cnt.sum()))
    if G < 2:
        return mean
    live = np.flatnonzero(cnt > 0)
    if len(live) < 2:
        return mean, np.full((n, n), np.nan)
    m = e[live].astype(np.float64) / (float(1 << EDGE_BITS) * cnt[live].astype(np.float64))[:, None, None]
    mbar = np.cumsum(m, axis=0)[-1] / len(live)
    d = m - mbar
    return mean, np.sqrt(np.cumsum(d * d, axis=0)[-1] / (len(live) * (len(live) - 1)))


DAG_FEATURES = ("edge", "ancestor", "blanket", "compelled", "vstruct")


class Context:
    """One ulg_ctx on one GPU (one process per GPU for multi-GPU work)."""

    def __init__(self, device: int = 0):
        L = lib()
        self._h = C.c_void_p()
        dev = (C.c_int * 1)(device)
        rc = L.ulg_create(dev, 1, C.byref(self._h))
        if rc != 0:
            raise ULGError(f"ulg_create(device={device}) failed with status {rc}")
        self.device = device
        self.n = None

    def close(self):
        if self._h:
            lib().ulg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = lib().ulg_last_error(self._h).decode()
            raise ULGError(f"{what}: status {rc}: {msg}")

    # ---- cBIC -------------------------------------------------------------
    def load(self, data: np.ndarray, lam: float):
        """data: N x n array (rows = records).  Stored column-major."""
        x = np.asfortranarray(np.asarray(data, dtype=np.float64))
        N, n = x.shape
        flat = np.ascontiguousarray(x.T.reshape(-1))  # column-major flatten
        self._check(lib().ulg_cbic_load(self._h, _ptr(flat), N, n, float(lam)), "ulg_cbic_load")
        self.n = n
        self.N = N

    def mmpc(self, alpha=0.05, max_cond=-1):
        """ulg_mmpc on the loaded data -> skeleton rows (bit j of row i = edge i-j)."""
        rows = np.zeros(64, dtype=np.uint64)
        self._check(lib().ulg_mmpc(self._h, float(alpha), int(max_cond), _ptr(rows)), "ulg_mmpc")
        return [int(x) for x in rows[:self.n]]

    def mmpc_min_z(self, ts, xs, musts, pools, max_cond=-1, stops=None) -> np.ndarray:
        """ulg_mmpc_min_z: per query the minimum |Fisher z| of (xs[i], ts[i] | S) over the
        subsets S of pools[i] (a variable mask) with |S| <= max_cond that contain musts[i]
        (< 0: every subset), stopping at the first value <= stops[i] (default -inf: never)."""
        t = np.ascontiguousarray(ts, dtype=np.int32)
        x = np.ascontiguousarray(xs, dtype=np.int32)
        m = np.ascontiguousarray(musts, dtype=np.int32)
        p = np.ascontiguousarray([int(v) for v in pools], dtype=np.uint64)
        s = np.full(len(t), -np.inf) if stops is None else np.ascontiguousarray(stops, dtype=np.float64)
        if not (t.shape == x.shape == m.shape == p.shape == s.shape):
            raise ValueError("mmpc_min_z: ts, xs, musts, pools and stops differ in length")
        out = np.zeros(max(len(t), 1), dtype=np.float64)
        self._check(lib().ulg_mmpc_min_z(self._h, len(t), _ptr(t), _ptr(x), _ptr(m), _ptr(p), int(max_cond), _ptr(s),
                                         _ptr(out)), "ulg_mmpc_min_z")
        return out[:len(t)]

    def gram(self) -> np.ndarray:
        g = np.empty((self.n, self.n), dtype=np.float64)
        self._check(lib().ulg_cbic_gram(self._h, _ptr(g)), "ulg_cbic_gram")
        return g

    def score(self, variables, candidates, max_parents: int):
        """Returns (total_stored, total_scored); results stay on the GPU."""
        v = np.ascontiguousarray(variables, dtype=np.int32)
        c = np.ascontiguousarray(candidates, dtype=np.uint64)
        st, sc = C.c_int64(), C.c_int64()
        self._check(lib().ulg_cbic_score(self._h, _ptr(v), len(v), _ptr(c), int(max_parents),
                                         C.byref(st), C.byref(sc)), "ulg_cbic_score")
        self._nv = len(v)
        return st.value, sc.value

    def score_async(self, variables, candidates, max_parents: int):
        """ulg_cbic_score_async: queues the scoring call; score_finish() waits for it."""
        v = np.ascontiguousarray(variables, dtype=np.int32)
        c = np.ascontiguousarray(candidates, dtype=np.uint64)
        self._check(lib().ulg_cbic_score_async(self._h, _ptr(v), len(v), _ptr(c), int(max_parents)),
                    "ulg_cbic_score_async")
        self._nv = len(v)

    def score_finish(self):
        """-> (total_stored, total_scored) of the last (async) scoring call."""
        st, sc = C.c_int64(), C.c_int64()
        self._check(lib().ulg_cbic_score_finish(self._h, C.byref(st), C.byref(sc)), "ulg_cbic_score_finish")
        return st.value, sc.value

    def fetch(self, total_stored: int):
        sets = np.empty(max(total_stored, 1), dtype=np.uint64)
        scores = np.empty(max(total_stored, 1), dtype=np.float32)
        offs = np.empty(self._nv + 1, dtype=np.int64)
        self._check(lib().ulg_cbic_fetch(self._h, _ptr(sets), _ptr(scores), _ptr(offs), 0), "ulg_cbic_fetch")
        return offs, sets[:total_stored], scores[:total_stored]

    def stream_wait_event(self, event):
        """ulg_stream_wait_event: this context's stream waits for a
        torch.cuda.Event (or a raw hipEvent_t handle) recorded on another
        stream of the same device."""
        h = event.cuda_event if hasattr(event, "cuda_event") else int(event)
        self._check(lib().ulg_stream_wait_event(self._h, C.c_void_p(h)), "ulg_stream_wait_event")

    def fetch_device(self, sets_ptr: int, scores_ptr: int, offsets_ptr: int):
        """Copy results into caller-owned device buffers (e.g. torch tensors).
        Synchronous on the context's stream; see ulg.h's stream contract."""
        self._check(lib().ulg_cbic_fetch(self._h, C.c_void_p(sets_ptr), C.c_void_p(scores_ptr),
                                         C.c_void_p(offsets_ptr), 1), "ulg_cbic_fetch")

    def score_all(self, variables, candidates, max_parents: int):
        st, _ = self.score(variables, candidates, max_parents)
        return self.fetch(st)

    def score_sets(self, variables, parents) -> np.ndarray:
        """ScoringFunction::calculateScore's value per (variable, parent mask) pair (ulg_cbic_score_sets)."""
        v = np.ascontiguousarray(variables, dtype=np.int32)
        p = np.ascontiguousarray(parents, dtype=np.uint64)
        if v.shape != p.shape:
            raise ValueError("score_sets: variables and parents differ in length")
        out = np.empty(max(len(v), 1), dtype=np.float32)
        self._check(lib().ulg_cbic_score_sets(self._h, len(v), _ptr(v), _ptr(p), _ptr(out)), "ulg_cbic_score_sets")
        return out[:len(v)]

    def set_constraints(self, alternatives):
        """ulg_cbic_set_constraints: alternatives = [(v, required, forbidden), ...] with
        required / forbidden as parent masks (bit i = variable i).  A variable with at
        least one alternative takes only parent sets P with required <= P and
        P & forbidden == 0 for one of them; every other set scores -float(n).  Holds
        until the next load(); an empty list clears."""
        alts = list(alternatives)
        v = np.ascontiguousarray([a[0] for a in alts], dtype=np.int32)
        r = np.ascontiguousarray([a[1] for a in alts], dtype=np.uint64)
        f = np.ascontiguousarray([a[2] for a in alts], dtype=np.uint64)
        self._check(lib().ulg_cbic_set_constraints(self._h, len(alts), _ptr(v), _ptr(r), _ptr(f)),
                    "ulg_cbic_set_constraints")

    def clear_constraints(self):
        self._check(lib().ulg_cbic_set_constraints(self._h, 0, None, None, None), "ulg_cbic_set_constraints")

    # ---- discrete BIC, BDeu and fNML ----------------------------------------
    SCORE_BIC = 1
    SCORE_BDEU = 3
    SCORE_FNML = 5

    def set_ess(self, ess: float):
        """ulg_disc_set_ess: the equivalent sample size of SCORE_BDEU (sticky, default 1.0,
        1e-6 <= ess <= 1e6; a refused value leaves the previous one)."""
        self._check(lib().ulg_disc_set_ess(self._h, float(ess)), "ulg_disc_set_ess")

    def load_discrete(self, codes: np.ndarray, arity):
        """ulg_disc_load: codes = N x n array of value codes (rows = records),
        arity[j] = cardinality of variable j.  Replaces the loaded data."""
        x = np.asarray(codes)
        if x.ndim != 2:
            raise ValueError("load_discrete: codes must be N x n")
        if x.size and (x.min() < 0 or x.max() > 255):
            raise ValueError("load_discrete: codes must be 0..255")
        N, n = x.shape
        flat = np.ascontiguousarray(x.astype(np.uint8).T.reshape(-1))  # column-major flatten
        ar = np.ascontiguousarray(arity, dtype=np.int32)
        if len(ar) != n:
            raise ValueError("load_discrete: one arity per column")
        self._check(lib().ulg_disc_load(self._h, _ptr(flat), N, n, _ptr(ar)), "ulg_disc_load")
        self.n = n
        self.N = N

    def score_discrete(self, variables, candidates, max_parents: int, kind: int = SCORE_BIC, prune=None, ess=None):
        """ulg_disc_score -> (total_stored, total_scored); fetch() reads the lists.
        kind: SCORE_BIC, SCORE_BDEU or SCORE_FNML.
        prune: True / False sets option "disc_prune" (sticky) before the call -- the
        reference's prune(): a set goes when a kept proper subset scores at least as
        well; total_stored then counts the kept sets and info("disc_pruned") the
        removed ones.  None leaves the option as it is.
        ess: set_ess(ess) before the call (sticky; only SCORE_BDEU reads it).  None
        leaves it as it is."""
        if prune is not None:
            self.set_option("disc_prune", 1 if prune else 0)
        if ess is not None:
            self.set_ess(ess)
        v = np.ascontiguousarray(variables, dtype=np.int32)
        c = np.ascontiguousarray(candidates, dtype=np.uint64)
        st, sc = C.c_int64(), C.c_int64()
        self._check(lib().ulg_disc_score(self._h, int(kind), _ptr(v), len(v), _ptr(c), int(max_parents),
                                         C.byref(st), C.byref(sc)), "ulg_disc_score")
        self._nv = len(v)
        return st.value, sc.value

    def score_sets_discrete(self, variables, parents, kind: int = SCORE_BIC, ess=None) -> np.ndarray:
        """calculateScore's value (BIC, BDeu or fNML, by kind) per (variable, parent mask) pair
        (ulg_disc_score_sets).  ess: as in score_discrete."""
        if ess is not None:
            self.set_ess(ess)
        v = np.ascontiguousarray(variables, dtype=np.int32)
        p = np.ascontiguousarray(parents, dtype=np.uint64)
        if v.shape != p.shape:
            raise ValueError("score_sets_discrete: variables and parents differ in length")
        out = np.empty(max(len(v), 1), dtype=np.float32)
        self._check(lib().ulg_disc_score_sets(self._h, int(kind), len(v), _ptr(v), _ptr(p), _ptr(out)),
                    "ulg_disc_score_sets")
        return out[:len(v)]

    # ---- BGe (continuous data) ------------------------------------------------
    def set_bge_prior(self, alpha_mu: float = 1.0, alpha_w: float = 0.0):
        """ulg_bge_set_prior: sticky; alpha_w = 0 means n + alpha_mu + 1 at scoring time.
        1e-3 <= alpha_mu <= 1e3 and alpha_w = 0 or n + 1 < alpha_w <= n + 1e6; a refused
        value leaves the previous prior."""
        self._check(lib().ulg_bge_set_prior(self._h, float(alpha_mu), float(alpha_w)), "ulg_bge_set_prior")
        self._bge_prior = (float(alpha_mu), float(alpha_w))

    def _bge_args(self, alpha_mu, alpha_w):
        if alpha_mu is not None or alpha_w is not None:
            cur = getattr(self, "_bge_prior", (1.0, 0.0))
            self.set_bge_prior(cur[0] if alpha_mu is None else alpha_mu, cur[1] if alpha_w is None else alpha_w)

    def score_bge(self, variables, candidates, max_parents: int, prune=None, alpha_mu=None, alpha_w=None):
        """ulg_bge_score on the data of load() -> (total_stored, total_scored); fetch() reads
        the lists.  Every finite value is stored, whatever its sign.
        prune: True / False sets option "bge_prune" (sticky) before the call; info("bge_pruned")
        then counts the removed sets.  None leaves the option as it is.
        alpha_mu / alpha_w: set_bge_prior before the call (sticky; None keeps that part)."""
        if prune is not None:
            self.set_option("bge_prune", 1 if prune else 0)
        self._bge_args(alpha_mu, alpha_w)
        v = np.ascontiguousarray(variables, dtype=np.int32)
        c = np.ascontiguousarray(candidates, dtype=np.uint64)
        st, sc = C.c_int64(), C.c_int64()
        self._check(lib().ulg_bge_score(self._h, _ptr(v), len(v), _ptr(c), int(max_parents),
                                        C.byref(st), C.byref(sc)), "ulg_bge_score")
        self._nv = len(v)
        return st.value, sc.value

    def score_sets_bge(self, variables, parents, alpha_mu=None, alpha_w=None) -> np.ndarray:
        """The BGe value per (variable, parent mask) pair (ulg_bge_score_sets): NaN for a set on a
        constant column, a pivot <= 0 or a set that violates the constraints."""
        self._bge_args(alpha_mu, alpha_w)
        v = np.ascontiguousarray(variables, dtype=np.int32)
        p = np.ascontiguousarray(parents, dtype=np.uint64)
        if v.shape != p.shape:
            raise ValueError("score_sets_bge: variables and parents differ in length")
        out = np.empty(max(len(v), 1), dtype=np.float32)
        self._check(lib().ulg_bge_score_sets(self._h, len(v), _ptr(v), _ptr(p), _ptr(out)), "ulg_bge_score_sets")
        return out[:len(v)]

    def regret(self, arity: int, first: int, count: int) -> np.ndarray:
        """ulg_disc_regret: ln C(arity, first .. first + count - 1) as SCORE_FNML uses it
        (the device table's entries; the table is built if need be)."""
        out = np.empty(max(int(count), 1), dtype=np.float64)
        self._check(lib().ulg_disc_regret(self._h, int(arity), int(first), int(count), _ptr(out)), "ulg_disc_regret")
        return out[:max(int(count), 0)]

    def discrete_counts(self, variable: int, parents: int, cap=None) -> np.ndarray:
        """ulg_disc_counts: the dense contingency table of (variable, parents),
        cell = sum_p code_p base_p + code_v q (parents ascending, first base 1)."""
        nc = C.c_int64()
        if cap is None:
            probe = np.zeros(1, dtype=np.int32)
            rc = lib().ulg_disc_counts(self._h, int(variable), C.c_uint64(int(parents)), _ptr(probe), 0, C.byref(nc))
            if rc != 0 and nc.value <= 0:
                self._check(rc, "ulg_disc_counts")
            cap = nc.value
        out = np.zeros(max(int(cap), 1), dtype=np.int32)
        self._check(lib().ulg_disc_counts(self._h, int(variable), C.c_uint64(int(parents)), _ptr(out), int(cap),
                                          C.byref(nc)), "ulg_disc_counts")
        return out[:nc.value]

    def g2_discrete(self, xs, ts, conds):
        """ulg_disc_g2: the G^2 statistic of each test (xs[i], ts[i] | conds[i] as a mask)
        -> (g2 float64, dof int64, cells int64); g2 is NaN where cells > 32768."""
        x = np.ascontiguousarray(xs, dtype=np.int32)
        t = np.ascontiguousarray(ts, dtype=np.int32)
        s = np.ascontiguousarray([int(m) for m in conds], dtype=np.uint64)
        if not (x.shape == t.shape == s.shape):
            raise ValueError("g2_discrete: xs, ts and conds differ in length")
        g2 = np.zeros(max(len(x), 1), dtype=np.float64)
        dof = np.zeros(max(len(x), 1), dtype=np.int64)
        cells = np.zeros(max(len(x), 1), dtype=np.int64)
        self._check(lib().ulg_disc_g2(self._h, len(x), _ptr(x), _ptr(t), _ptr(s), _ptr(g2), _ptr(dof), _ptr(cells)),
                    "ulg_disc_g2")
        return g2[:len(x)], dof[:len(x)], cells[:len(x)]

    def mmpc_discrete(self, alpha=0.05, max_cond=-1, min_per_cell=5):
        """ulg_disc_mmpc on the loaded value codes -> skeleton rows (bit j of row i = edge i-j)."""
        rows = np.zeros(64, dtype=np.uint64)
        self._check(lib().ulg_disc_mmpc(self._h, float(alpha), int(max_cond), int(min_per_cell), _ptr(rows)),
                    "ulg_disc_mmpc")
        return [int(x) for x in rows[:self.n]]

    def quantize(self, scores: np.ndarray) -> np.ndarray:
        s = np.ascontiguousarray(scores, dtype=np.float32)
        out = np.empty_like(s)
        self._check(lib().ulg_quantize_costs(self._h, _ptr(s), _ptr(out), s.size), "ulg_quantize_costs")
        return out

    # ---- search side -------------------------------------------------------
    ASTAR_EXACT = 0
    ASTAR_GPU = 1

    def search_load(self, offsets, sets, costs):
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        s = np.ascontiguousarray(sets, dtype=np.uint64)
        c = np.ascontiguousarray(costs, dtype=np.float32)
        if s.size == 0:
            s = np.zeros(1, dtype=np.uint64)
            c = np.zeros(1, dtype=np.float32)
        self._check(lib().ulg_search_load(self._h, len(o) - 1, _ptr(o), _ptr(s), _ptr(c)), "ulg_search_load")
        self.search_n = len(o) - 1

    def search_from_scores(self):
        self._check(lib().ulg_search_from_scores(self._h), "ulg_search_from_scores")
        self.search_n = self.n

    def search_load_scores(self, offsets, sets, scores, device_ptrs=False):
        """ulg_search_load_scores: per-variable .pss-score lists in variable
        order (offsets[n+1] on the host).  device_ptrs: sets/scores are
        device addresses (ints, e.g. tensor.data_ptr()); else numpy arrays."""
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        if device_ptrs:
            sp, cp = C.c_void_p(int(sets)), C.c_void_p(int(scores))
            keep = None
        else:
            s = np.ascontiguousarray(sets, dtype=np.uint64)
            c = np.ascontiguousarray(scores, dtype=np.float32)
            if s.size == 0:
                s, c = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.float32)
            sp, cp, keep = _ptr(s), _ptr(c), (s, c)
        self._check(lib().ulg_search_load_scores(self._h, len(o) - 1, _ptr(o), sp, cp, 1 if device_ptrs else 0),
                    "ulg_search_load_scores")
        del keep
        self.search_n = len(o) - 1

    # ---- exact model averaging over the order lattice ------------------------
    def posterior(self, offsets, sets, scores, device_ptrs=False, want_sets=True):
        """ulg_posterior on per-variable lists (offsets[n+1] on the host; sets / scores numpy
        arrays, or device addresses with device_ptrs) under the order-modular prior
        -> (log_z, edge float64 (n, n) with edge[u, v] = p(u -> v), set_logpost float64 per
        list entry or None)."""
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(o) - 1
        total = int(o[-1] - o[0]) if n >= 0 and len(o) else 0
        if device_ptrs:
            sp, cp, keep = C.c_void_p(int(sets)), C.c_void_p(int(scores)), None
        else:
            s = np.ascontiguousarray(sets, dtype=np.uint64)
            c = np.ascontiguousarray(scores, dtype=np.float32)
            if s.size == 0:
                s, c = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.float32)
            sp, cp, keep = _ptr(s), _ptr(c), (s, c)
        lz = C.c_double()
        edge = np.zeros((max(n, 1), max(n, 1)), dtype=np.float64)
        lp = np.zeros(max(total, 1), dtype=np.float64) if want_sets else None
        self._post_n = None  # a refused call leaves nothing to sample
        self._check(lib().ulg_posterior(self._h, n, _ptr(o), sp, cp, 1 if device_ptrs else 0, C.byref(lz), _ptr(edge),
                                        _ptr(lp) if lp is not None else None), "ulg_posterior")
        self._post_n = n
        del keep
        return lz.value, edge, (lp[:max(total, 0)] if lp is not None else None)

    def posterior_from_scores(self, want_sets=True):
        """ulg_posterior_from_scores: the same from the lists of the last scoring call (every
        variable scored), scores as they are; set_logpost in variable order."""
        n = self.n or 1
        total = 0
        if want_sets and hasattr(self, "_nv"):  # the list entries: the last offset of the stored lists
            offs = np.zeros(self._nv + 1, dtype=np.int64)
            self._check(lib().ulg_cbic_fetch(self._h, None, None, _ptr(offs), 0), "ulg_cbic_fetch")
            total = int(offs[-1])
        lz = C.c_double()
        edge = np.zeros((n, n), dtype=np.float64)
        lp = np.zeros(max(total, 1), dtype=np.float64) if want_sets else None
        self._post_n = None
        self._check(lib().ulg_posterior_from_scores(self._h, C.byref(lz), _ptr(edge),
                                                    _ptr(lp) if lp is not None else None), "ulg_posterior_from_scores")
        self._post_n = n
        return lz.value, edge, (lp[:total] if lp is not None else None)

    def posterior_table(self, which: int, var: int = 0) -> np.ndarray:
        """ulg_posterior_table: one table of the last posterior call as float64 -- which = 0: ln
        alpha_var, 1: ln f, 2: ln b, 3: ln gamma_var (option "posterior_keep" 1 at the call)."""
        cnt = C.c_int64()
        self._check(lib().ulg_posterior_table(self._h, int(which), int(var), None, 0, C.byref(cnt)),
                    "ulg_posterior_table")
        out = np.empty(cnt.value, dtype=np.float64)
        self._check(lib().ulg_posterior_table(self._h, int(which), int(var), _ptr(out), out.size, C.byref(cnt)),
                    "ulg_posterior_table")
        return out

    def _sample_outputs(self, who, count, want_order, want_weight):
        """The host arrays of `count` samples, n from the last successful posterior call of this object.
        None where the library must refuse the call itself (no such call, a negative count); arrays that
        do not fit the host are the caller's error as much as buffers that do not fit the device."""
        n = getattr(self, "_post_n", None)
        if n is None or count < 0:
            return None
        try:
            parents = np.zeros((count, n), dtype=np.uint64)
            order = np.zeros((count, n), dtype=np.uint8) if want_order else None
            weight = np.zeros(count, dtype=np.float64) if want_weight else None
        except (MemoryError, ValueError) as e:
            raise ULGError(f"{who}: status 4: {count} samples of n = {n} do not fit the host memory ({e})") from None
        return parents, order, weight

    def posterior_sample(self, count, seed=0, first=0, want_order=True, want_weight=True):
        """ulg_posterior_sample: samples first .. first + count - 1 of `seed` from the order-modular
        posterior of the last posterior call -> (parents uint64 (count, n): parents[k, v] = the parent
        mask of v, order uint8 (count, n): order[k, i] = the variable at position i, or None,
        log_weight float64 (count): the sum of the chosen sets' scores, or None)."""
        count, first, seed = int(count), int(first), int(seed)
        out = self._sample_outputs("ulg_posterior_sample", count, want_order, want_weight)
        if out is None:  # the library's own refusal: state, or a negative count
            self._check(lib().ulg_posterior_sample(self._h, seed, first, min(count, 0), None, None, None), "ulg_posterior_sample")
            raise ULGError("ulg_posterior_sample: status 3: the last posterior call through this object was refused")
        parents, order, weight = out
        self._check(lib().ulg_posterior_sample(self._h, seed, first, count, _ptr(parents),
                                               _ptr(order) if want_order else None, _ptr(weight) if want_weight else None),
                    "ulg_posterior_sample")
        return parents, order, weight

    def posterior_sample_u(self, u, want_order=True, want_weight=True):
        """ulg_posterior_sample_u (tests): the same with the draws given, u uint64 (count, n, 2):
        u[k, i] = (U_sink, U_set) of step position i of sample k."""
        u = np.ascontiguousarray(u, dtype=np.uint64)
        out = self._sample_outputs("ulg_posterior_sample_u", int(u.shape[0]) if u.ndim == 3 else 0, want_order, want_weight)
        if out is None:
            self._check(lib().ulg_posterior_sample_u(self._h, 0, None, None, None, None), "ulg_posterior_sample_u")
            raise ULGError("ulg_posterior_sample_u: status 3: the last posterior call through this object was refused")
        parents, order, weight = out
        if u.ndim != 3 or u.shape[1:] != (parents.shape[1], 2):
            raise ULGError(f"posterior_sample_u: u must be (count, {parents.shape[1]}, 2), not {u.shape}")
        self._check(lib().ulg_posterior_sample_u(self._h, u.shape[0], _ptr(u), _ptr(parents), _ptr(order) if want_order else None,
                                                 _ptr(weight) if want_weight else None), "ulg_posterior_sample_u")
        return parents, order, weight

    def dag_linear_extensions(self, parents, dedupe=True):
        """ulg_dag_linear_extensions on parents uint64 (count, n), parents[k, v] = the parent mask of v
        in DAG k (what posterior_sample returns) -> (ext: a list of Python ints, the exact number of
        linear extensions of each DAG, 0 for a cyclic one; log_ext float64 (count), -inf for 0).
        dedupe: the distinct rows only go to the library and their results are scattered back (a
        peaked posterior repeats DAGs); False is the raw call."""
        p = np.ascontiguousarray(parents, dtype=np.uint64)
        if p.ndim != 2 or p.shape[1] < 1:
            raise ULGError(f"dag_linear_extensions: parents must be (count, n) with n >= 1, not {p.shape}")
        count, n = p.shape
        inverse = None
        if dedupe and count > 1:
            p, inverse = np.unique(p, axis=0, return_inverse=True)
            p, inverse = np.ascontiguousarray(p), np.asarray(inverse).reshape(-1)
        lo = np.zeros(p.shape[0], dtype=np.uint64)
        hi = np.zeros(p.shape[0], dtype=np.uint64)
        le = np.zeros(p.shape[0], dtype=np.float64)
        self._check(lib().ulg_dag_linear_extensions(self._h, n, p.shape[0], _ptr(p), _ptr(lo), _ptr(hi), _ptr(le)),
                    "ulg_dag_linear_extensions")
        ext = [(int(h) << 64) | int(l) for l, h in zip(lo, hi)]
        if inverse is not None:
            ext, le = [ext[i] for i in inverse], le[inverse]
        return ext, le

    def dag_features(self, parents, weight=None, want=DAG_FEATURES):
        """ulg_dag_features on parents uint64 (count, n) (what posterior_sample returns) and integer
        weights uint64 (count) (None: every weight 1; uniform_prior_weights gives those of the uniform
        prior) -> dict: for each name of `want`, the exact sum over the acyclic graphs of the batch as a
        uint64 array -- "edge", "ancestor", "blanket", "compelled" (n, n), entry [u, v]; "vstruct"
        (n, n, n), entry [v, u, w] with u < w -- plus "total" (the weight of the acyclic graphs) and
        "cyclic" (the number of cyclic ones) as Python ints.  An estimate is table / total."""
        p = np.ascontiguousarray(parents, dtype=np.uint64)
        if p.ndim != 2 or p.shape[1] < 1:
            raise ULGError(f"dag_features: parents must be (count, n) with n >= 1, not {p.shape}")
        count, n = p.shape
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.uint64)
            if w.shape != (count,):
                raise ULGError(f"dag_features: weight must be ({count},), not {w.shape}")
        unknown = [name for name in want if name not in DAG_FEATURES]
        if unknown:
            raise ULGError(f"dag_features: unknown features {unknown}; known: {DAG_FEATURES}")
        out = {name: np.zeros((n, n, n) if name == "vstruct" else (n, n), dtype=np.uint64) for name in want}
        total, cyclic = C.c_uint64(0), C.c_int64(0)
        self._check(lib().ulg_dag_features(self._h, n, count, _ptr(p), None if w is None else _ptr(w),
                                           *[_ptr(out[name]) if name in out else None for name in DAG_FEATURES],
                                           C.byref(total), C.byref(cyclic)), "ulg_dag_features")
        out["total"], out["cyclic"] = int(total.value), int(cyclic.value)
        return out

    # ---- order MCMC ----------------------------------------------------------
    def _mcmc_init_arg(self, who, init_order, chains, n):
        if init_order is None:
            return None, None
        o = np.ascontiguousarray(init_order, dtype=np.uint8)
        if o.shape != (chains, n):
            raise ULGError(f"{who}: init_order must be ({chains}, {n}), not {o.shape}")
        return o, _ptr(o)

    def order_mcmc_begin(self, offsets, sets, scores, chains, seed=0, init_order=None, device_ptrs=False):
        """ulg_order_mcmc_begin on per-variable lists (as Context.posterior takes them): `chains` chains of
        seed `seed`, each from its row of init_order uint8 (chains, n) or, with None, from the contract's
        shuffle; step 0."""
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        n, chains = len(o) - 1, int(chains)
        if device_ptrs:
            sp, cp, keep = C.c_void_p(int(sets)), C.c_void_p(int(scores)), None
        else:
            s = np.ascontiguousarray(sets, dtype=np.uint64)
            c = np.ascontiguousarray(scores, dtype=np.float32)
            if s.size == 0:
                s, c = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.float32)
            sp, cp, keep = _ptr(s), _ptr(c), (s, c)
        init, ip = self._mcmc_init_arg("order_mcmc_begin", init_order, chains, n)
        self._mcmc = None  # a refused call leaves no chains
        self._check(lib().ulg_order_mcmc_begin(self._h, n, _ptr(o), sp, cp, 1 if device_ptrs else 0, chains, int(seed), ip),
                    "ulg_order_mcmc_begin")
        self._mcmc = (n, chains)
        del keep, init

    def order_mcmc_begin_from_scores(self, chains, seed=0, init_order=None):
        """ulg_order_mcmc_begin_from_scores: the same on the lists of the last scoring call (every
        variable scored), scores as they are."""
        n, chains = self.n or 1, int(chains)
        init, ip = self._mcmc_init_arg("order_mcmc_begin_from_scores", init_order, chains, n)
        self._mcmc = None
        self._check(lib().ulg_order_mcmc_begin_from_scores(self._h, chains, int(seed), ip), "ulg_order_mcmc_begin_from_scores")
        self._mcmc = (n, chains)
        del init

    def _mcmc_shape(self, who):
        """(n, chains) of the chains this object began; without them the library's own refusal is raised."""
        if getattr(self, "_mcmc", None) is None:
            self._check(lib().ulg_order_mcmc_state(self._h, None, None, None), who)
            raise ULGError(f"{who}: status 3: the last order_mcmc_begin through this object was refused")
        return self._mcmc

    def order_mcmc_state(self):
        """ulg_order_mcmc_state -> (order uint8 (chains, n), terms float64 (chains, n): terms[c, p] = the
        term of position p, step: the steps every chain has made since begin)."""
        n, chains = self._mcmc_shape("ulg_order_mcmc_state")
        order = np.zeros((chains, n), dtype=np.uint8)
        terms = np.zeros((chains, n), dtype=np.float64)
        step = C.c_int64()
        self._check(lib().ulg_order_mcmc_state(self._h, _ptr(order), _ptr(terms), C.byref(step)), "ulg_order_mcmc_state")
        return order, terms, step.value

    def order_mcmc_run(self, steps, thin=1, want_order=True, want_score=True, want_parents=True, want_weight=True, trace=False):
        """ulg_order_mcmc_run: every chain `steps` steps on, a record after each step t with t % thin == 0
        (t counts from begin) -> dict: "records" (per chain, R = (t0 + steps) // thin - t0 // thin),
        "order" uint8 (R, chains, n), "log_score" float64 (R, chains), "parents" uint64 (R, chains, n),
        "log_weight" float64 (R, chains) -- each present if wanted (want_weight needs want_parents) --
        "accepted" int64 (chains): accepted moves since begin, "step": the steps made since begin; with
        trace also "trace_delta" float64 and "trace_accept" uint8 (steps, chains)."""
        n, chains = self._mcmc_shape("ulg_order_mcmc_run")
        steps, thin = int(steps), int(thin)
        t0 = C.c_int64()
        self._check(lib().ulg_order_mcmc_state(self._h, None, None, C.byref(t0)), "ulg_order_mcmc_state")
        ok = steps >= 0 and thin >= 1
        R = (t0.value + steps) // thin - t0.value // thin if ok else 0
        want_weight = want_weight and want_parents
        out = {}
        try:
            if want_order:
                out["order"] = np.zeros((R, chains, n), dtype=np.uint8)
            if want_score:
                out["log_score"] = np.zeros((R, chains), dtype=np.float64)
            if want_parents:
                out["parents"] = np.zeros((R, chains, n), dtype=np.uint64)
            if want_weight:
                out["log_weight"] = np.zeros((R, chains), dtype=np.float64)
            if trace:
                out["trace_delta"] = np.zeros((max(steps, 0), chains), dtype=np.float64)
                out["trace_accept"] = np.zeros((max(steps, 0), chains), dtype=np.uint8)
        except (MemoryError, ValueError) as e:
            raise ULGError(f"ulg_order_mcmc_run: status 4: {R} records of {chains} chains do not fit the host memory ({e})") from None
        out["accepted"] = np.zeros(chains, dtype=np.int64)
        recs = C.c_int64()
        arg = lambda name: _ptr(out[name]) if name in out else None  # noqa: E731
        self._check(lib().ulg_order_mcmc_run(self._h, steps, thin, arg("order"), arg("log_score"), arg("parents"), arg("log_weight"),
                                             _ptr(out["accepted"]), arg("trace_delta"), arg("trace_accept"), C.byref(recs)),
                    "ulg_order_mcmc_run")
        assert recs.value == R
        out["records"], out["step"] = R, t0.value + steps
        return out

    def order_score(self, orders):
        """ulg_order_score: orders uint8 (count, n), each a permutation -> terms float64 (count, n),
        terms[k, p] = the term of position p of order k on the lists of the last order_mcmc_begin."""
        n, _ = self._mcmc_shape("ulg_order_score")
        o = np.ascontiguousarray(orders, dtype=np.uint8)
        if o.ndim != 2 or o.shape[1] != n:
            raise ULGError(f"order_score: orders must be (count, {n}), not {o.shape}")
        terms = np.zeros(o.shape, dtype=np.float64)
        self._check(lib().ulg_order_score(self._h, o.shape[0], _ptr(o), _ptr(terms)), "ulg_order_score")
        return terms

    def order_edges(self, orders, groups=1):
        """ulg_order_edges: orders uint8 (count, n), each a permutation -> (edge uint64 (groups, n, n), zero):
        order k adds g(u -> v) = floor(p(u -> v | order k) 2^40) into edge[k % groups, u, v]; zero = the orders
        of probability 0 (a term of -inf), which add nothing.  ulg.order_edge_posterior turns the tables into
        the mean matrix."""
        n, _ = self._mcmc_shape("ulg_order_edges")
        o = np.ascontiguousarray(orders, dtype=np.uint8)
        if o.ndim != 2 or o.shape[1] != n:
            raise ULGError(f"order_edges: orders must be (count, {n}), not {o.shape}")
        groups = int(groups)
        tables = groups if 1 <= groups <= max(o.shape[0], 1) else 1  # a number of groups the library refuses: it writes nothing
        try:
            edge = np.zeros((tables, n, n), dtype=np.uint64)
        except (MemoryError, ValueError) as e:
            raise ULGError(f"ulg_order_edges: status 4: {groups} tables of n = {n} do not fit the host memory ({e})") from None
        zero = C.c_int64()
        self._check(lib().ulg_order_edges(self._h, o.shape[0], _ptr(o), groups, _ptr(edge), C.byref(zero)), "ulg_order_edges")
        return edge, zero.value

    def bestscore(self, variables, S):
        v = np.ascontiguousarray(variables, dtype=np.int32)
        s = np.ascontiguousarray([int(x) for x in S], dtype=np.uint64)
        costs = np.empty(len(v), dtype=np.float32)
        par = np.empty(len(v), dtype=np.uint64)
        self._check(lib().ulg_bestscore_query(self._h, len(v), _ptr(v), _ptr(s), _ptr(costs), _ptr(par)),
                    "ulg_bestscore_query")
        return costs, par

    def pdb_build(self, pd_count=2, ancestors=0, scc=None):
        if scc is None:
            scc = (1 << self.search_n) - 1
        self._check(lib().ulg_pdb_build(self._h, int(pd_count), int(ancestors), int(scc)), "ulg_pdb_build")

    def pdb_h(self, S):
        s = np.ascontiguousarray([int(x) for x in S], dtype=np.uint64)
        h = np.empty(len(s), dtype=np.float32)
        comp = np.empty(len(s), dtype=np.int32)
        self._check(lib().ulg_pdb_query(self._h, len(s), _ptr(s), _ptr(h), _ptr(comp)), "ulg_pdb_query")
        return h, comp

    def bestscore_table(self, v):
        """ulg_bestscore_table: (D_v, float32[2^m]) -- variable v's best-score
        table as the device holds it, indexed by pext(S, D_v); an empty array
        for a variable without a table (sharded tables)."""
        sup, cnt = C.c_uint64(), C.c_int64()
        self._check(lib().ulg_bestscore_table(self._h, int(v), C.byref(sup), None, 0, C.byref(cnt)),
                    "ulg_bestscore_table")
        out = np.empty(cnt.value, dtype=np.float32)
        if out.size:
            self._check(lib().ulg_bestscore_table(self._h, int(v), C.byref(sup), _ptr(out), out.size, C.byref(cnt)),
                        "ulg_bestscore_table")
        return sup.value, out

    def pdb_table(self, g):
        """ulg_pdb_table: (group mask, float32[2^size]) -- pattern-database
        group g from the device array, indexed by pext(R, mask)."""
        mask, cnt = C.c_uint64(), C.c_int64()
        self._check(lib().ulg_pdb_table(self._h, int(g), C.byref(mask), None, 0, C.byref(cnt)), "ulg_pdb_table")
        out = np.empty(cnt.value, dtype=np.float32)
        self._check(lib().ulg_pdb_table(self._h, int(g), C.byref(mask), _ptr(out), out.size, C.byref(cnt)),
                    "ulg_pdb_table")
        return mask.value, out

    def astar(self, edges=None, pd_count=2, mode=0, net_text=True, ancestors=None, scc=None):
        n = self.search_n
        vpar = np.zeros(n, dtype=np.uint64)
        order = np.zeros(n, dtype=np.int32)
        cost = C.c_float()
        exp = C.c_int64()
        buf = C.create_string_buffer(1 << 16) if net_text else None
        e = None
        if edges is not None:
            e = np.ascontiguousarray([int(x) for x in edges], dtype=np.uint64)
        if ancestors is None and scc is None:
            self._check(lib().ulg_astar(self._h, _ptr(e) if e is not None else None, int(pd_count), int(mode),
                                        _ptr(vpar), _ptr(order), C.byref(cost), C.byref(exp), buf,
                                        len(buf) if buf is not None else 0), "ulg_astar")
        else:
            anc = int(ancestors or 0)
            sc = int(scc) if scc is not None else (1 << n) - 1
            self._check(lib().ulg_astar_scc(self._h, _ptr(e) if e is not None else None, int(pd_count), int(mode),
                                            anc, sc, _ptr(vpar), _ptr(order), C.byref(cost), C.byref(exp), buf,
                                            len(buf) if buf is not None else 0), "ulg_astar_scc")
        return {"vpar": vpar, "order": order, "cost": cost.value, "expanded": exp.value,
                "net_text": buf.value.decode() if buf is not None else None}

    def sweep_shard_begin(self, own: int) -> int:
        """This rank's tables and sweep slices for the variables in `own`
        (ulg_sweep_shard_begin); returns the largest layer's node count."""
        mx = C.c_int64()
        self._check(lib().ulg_sweep_shard_begin(self._h, int(own), C.byref(mx)), "ulg_sweep_shard_begin")
        return mx.value

    def sweep_shard_layer(self, layer: int, keys_ptr: int):
        self._check(lib().ulg_sweep_shard_layer(self._h, int(layer), C.c_void_p(keys_ptr)), "ulg_sweep_shard_layer")

    def sweep_shard_commit(self, layer: int, keys_ptr: int):
        self._check(lib().ulg_sweep_shard_commit(self._h, int(layer), C.c_void_p(keys_ptr)), "ulg_sweep_shard_commit")

    def sweep_shard_end(self):
        n = self.search_n
        vpar = np.zeros(n, dtype=np.uint64)
        order = np.zeros(n, dtype=np.int32)
        cost = C.c_float()
        exp = C.c_int64()
        self._check(lib().ulg_sweep_shard_end(self._h, _ptr(vpar), _ptr(order), C.byref(cost), C.byref(exp)),
                    "ulg_sweep_shard_end")
        return {"vpar": vpar, "order": order, "cost": cost.value, "expanded": exp.value}

    def sweep_leaves(self) -> np.ndarray:
        """ulg_sweep_leaves: the leaf bytes (uint8, 2^m, layer then colex
        order) of the last component the GPU sweep finished."""
        cnt = C.c_int64()
        self._check(lib().ulg_sweep_leaves(self._h, None, 0, C.byref(cnt)), "ulg_sweep_leaves")
        out = np.empty(cnt.value, dtype=np.uint8)
        self._check(lib().ulg_sweep_leaves(self._h, _ptr(out), out.size, C.byref(cnt)), "ulg_sweep_leaves")
        return out

    def _names_arg(self, names):
        arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
        return arr

    def pss_format(self, header: str, names, arity) -> bytes:
        """ulg_pss_format: the .pss text of the last score() call (every variable)."""
        nm = self._names_arg(names)
        ar = np.ascontiguousarray(arity, dtype=np.int32)
        text, ln = C.c_void_p(), C.c_int64()
        self._check(lib().ulg_pss_format(self._h, header.encode(), C.cast(nm, C.c_void_p), _ptr(ar), C.byref(text),
                                         C.byref(ln)), "ulg_pss_format")
        return C.string_at(text.value, ln.value)

    def pss_format_lists(self, header: str, names, arity, offsets, sets, scores) -> bytes:
        nm = self._names_arg(names)
        ar = np.ascontiguousarray(arity, dtype=np.int32)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        st = np.ascontiguousarray(sets, dtype=np.uint64)
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        text, ln = C.c_void_p(), C.c_int64()
        self._check(lib().ulg_pss_format_lists(self._h, len(names), _ptr(offs), _ptr(st), _ptr(sc), header.encode(),
                                               C.cast(nm, C.c_void_p), _ptr(ar), C.byref(text), C.byref(ln)),
                    "ulg_pss_format_lists")
        return C.string_at(text.value, ln.value)

    def triplet(self, edges=None, pd_count=2):
        """ulg_triplet_astar -> {"mec": n x n int32 (i -> j at [i, j]), "runs", "distinct", "expanded"}."""
        n = self.search_n
        dg = np.zeros(n * n, dtype=np.int32)
        stats = np.zeros(3, dtype=np.int64)
        e = None
        if edges is not None:
            e = np.ascontiguousarray([int(x) for x in edges], dtype=np.uint64)
        self._check(lib().ulg_triplet_astar(self._h, _ptr(e) if e is not None else None, int(pd_count), _ptr(dg),
                                            _ptr(stats)), "ulg_triplet_astar")
        return {"mec": dg.reshape(n, n), "runs": int(stats[0]), "distinct": int(stats[1]), "expanded": int(stats[2])}

    def triplet_clusters(self, edges=None):
        """ulg_triplet_clusters -> uint64 array of the first sweep's distinct clusters."""
        e = None if edges is None else np.ascontiguousarray([int(x) for x in edges], dtype=np.uint64)
        cnt = C.c_int64()
        self._check(lib().ulg_triplet_clusters(self._h, _ptr(e) if e is not None else None, None, 0,
                                               C.byref(cnt)), "ulg_triplet_clusters")
        out = np.zeros(max(cnt.value, 1), dtype=np.uint64)
        self._check(lib().ulg_triplet_clusters(self._h, _ptr(e) if e is not None else None, _ptr(out), len(out),
                                               C.byref(cnt)), "ulg_triplet_clusters")
        return out[:cnt.value]

    def triplet_solve(self, clusters, pd_count=2):
        """ulg_triplet_solve -> (parents [nc, n] uint64, {"runs", "distinct", "expanded"})."""
        cl = np.ascontiguousarray(clusters, dtype=np.uint64)
        par = np.zeros((max(len(cl), 1), self.search_n), dtype=np.uint64)
        stats = np.zeros(3, dtype=np.int64)
        self._check(lib().ulg_triplet_solve(self._h, _ptr(cl), len(cl), int(pd_count), _ptr(par), _ptr(stats)),
                    "ulg_triplet_solve")
        return par[:len(cl)], {"runs": int(stats[0]), "distinct": int(stats[1]), "expanded": int(stats[2])}

    def triplet_memo_put(self, clusters, parents, pd_count=2):
        cl = np.ascontiguousarray(clusters, dtype=np.uint64)
        par = np.ascontiguousarray(parents, dtype=np.uint64).reshape(len(cl), self.search_n) if len(cl) else \
            np.zeros((1, self.search_n), dtype=np.uint64)
        self._check(lib().ulg_triplet_memo_put(self._h, _ptr(cl), len(cl), int(pd_count), _ptr(par)),
                    "ulg_triplet_memo_put")

    def set_option(self, name: str, value: int):
        self._check(lib().ulg_set_option(self._h, name.encode(), int(value)), "ulg_set_option")

    def diag_pdb_host(self, cluster: int, pd_count: int = 2, cancel_preset: bool = False):
        """ulg_diag_pdb_host (tests): -> (built, cancelled, entries, entries equal to the device PDB's)."""
        out = np.zeros(4, dtype=np.int64)
        self._check(lib().ulg_diag_pdb_host(self._h, C.c_uint64(int(cluster)), int(pd_count), int(bool(cancel_preset)),
                                            _ptr(out)), "ulg_diag_pdb_host")
        return tuple(int(x) for x in out)

    def info(self, name: str) -> int:
        """ulg_get_info: "out_of_time", "highest_completed_layer", "score_error_word",
        "exact_cycles", "exact_instructions", "exact_cache_misses", "disc_mmpc_tests",
        "disc_mmpc_skipped", "disc_pruned" (sets the last score_discrete's prune pass
        removed; 0 with option "disc_prune" off), "bge_pruned" (likewise for score_bge and
        option "bge_prune"), "fnml_table_bytes" (the SCORE_FNML
        regret table of the loaded data; 0 while there is none), "score_graph_captures"
        (scoring calls of this context that captured their launch graph anew)."""
        v = C.c_int64()
        self._check(lib().ulg_get_info(self._h, name.encode(), C.byref(v)), "ulg_get_info")
        return v.value

    # ---- profiling ----------------------------------------------------------
    def profile(self, on: bool = True):
        self._check(lib().ulg_profile_enable(self._h, 1 if on else 0), "ulg_profile_enable")

    def profile_select(self, names=None):
        """Time only these kernels (None = all)."""
        arg = ",".join(names).encode() if names else None
        self._check(lib().ulg_profile_select(self._h, arg), "ulg_profile_select")

    def profile_reset(self):
        self._check(lib().ulg_profile_reset(self._h), "ulg_profile_reset")

    def profile_get(self, name: str):
        avg, tot = C.c_double(), C.c_double()
        cnt = C.c_int64()
        rc = lib().ulg_profile_get(self._h, name.encode(), C.byref(avg), C.byref(cnt), C.byref(tot))
        if rc != 0:
            return None
        return {"avg_ms": avg.value, "count": cnt.value, "total_ms": tot.value}

    def profile_dump(self) -> dict:
        buf = C.create_string_buffer(1 << 16)
        self._check(lib().ulg_profile_dump(self._h, buf, len(buf)), "ulg_profile_dump")
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, tot = line.split()
            out[name] = {"count": int(cnt), "total_ms": float(tot)}
        return out


def candidates_from_edges(edges, n: int):
    """2-hop candidate sets N(v) U N(N(v)) (score_main.cpp:146-153)."""
    allm = (1 << n) - 1
    if edges is None:
        return [allm] * n
    out = []
    for v in range(n):
        nb = int(edges[v])
        for j in range(n):
            if (int(edges[v]) >> j) & 1 and j != v:
                nb |= int(edges[j])
        out.append(nb)
    return out
