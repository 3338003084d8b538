"""GPU tests of the partition MCMC (ulg_partition_mcmc_*, ulg_partition_score; kernels:
csrc/partition_mcmc.hip) against tests/partition_mcmc_ref.py, whose docstring and
order_mcmc_ref's derive every cap used here; none is measured on the device.  Each
comparison prints "partition-mcmc-observed <family> <input> max <fraction of its cap>".
tests/test_partition_mcmc_ref.py shows on the CPU that the chain inputs have no
undecided step and meet every move kind, every no-op case, a -inf rejection and a sum
past 2^64 (n = 33, 63), and that the statistical inputs have mixed."""
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import order_mcmc_ref as om
import partition_mcmc_ref as pm
import ulg

pytestmark = pytest.mark.gpu

STATUS = {"ARG": 1, "STATE": 3}
LD = np.longdouble
KEYS = ("part", "parts", "log_score", "parents", "log_weight", "accepted", "trace_delta", "trace_accept")


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _observed(family, name, got, want, cap):
    got, want, cap = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=LD), np.asarray(cap, dtype=np.float64)
    fin = want > -np.inf
    assert np.array_equal(got > -np.inf, fin) and np.all(got[~fin] == -np.inf), "finite / -inf pattern differs"
    frac = float((np.abs(got[fin].astype(LD) - want[fin]) / np.maximum(cap[fin], 1e-300)).max()) if fin.any() else 0.0
    print(f"partition-mcmc-observed {family} {name} max {frac:.3g} of its cap")
    assert frac <= 1.0, (family, name, frac)


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


def _same(a, b, keys=KEYS):
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()] == []


# ---- 1. step by step against the restatement -----------------------------------------------
@pytest.mark.parametrize("name", sorted(pm.chain_inputs()))
def test_chains_equal_the_restatement(ctx, name):
    L, seed, init = pm.chain_inputs()[name]
    ref = pm.chain_reference(name)
    n, steps, thin = L.n, pm.CHAIN_STEPS, pm.CHAIN_THIN
    ctx.partition_mcmc_begin(*L.triple(), len(init), seed=seed, init_part=init)
    p0, t0, step = ctx.partition_mcmc_state()
    assert step == 0 and np.array_equal(p0, init)
    assert np.array_equal(ctx.partition_score(init), t0)  # 5. the same device function, the same bits
    r = ctx.partition_mcmc_run(steps, thin, trace=True)
    assert r["records"] == steps // thin and r["step"] == steps
    for k in ("trace_accept", "accepted", "part", "parts", "parents", "log_weight"):
        assert np.array_equal(r[k].astype(ref[k].dtype), ref[k]), k
    p1, t1, step = ctx.partition_mcmc_state()
    assert step == steps and np.array_equal(p1, ref["final_part"])
    assert np.array_equal(ctx.partition_score(p1), t1)
    _observed("delta", name, r["trace_delta"], ref["trace_delta"], ref["trace_cap"])
    _observed("log-score", name, r["log_score"], ref["log_score"], ref["score_cap"])
    _observed("final-terms", name, t1, ref["final_terms"], ref["final_cap"])
    # every decision again, from the device's own delta bits: the slack is exp's 8 units alone
    u_acc = np.stack([[(lambda x: int(x[0][0]) | (int(x[1][0]) << 32))(om._draw(seed, t, [c], pm.AUX)) for c in range(len(init))]
                      for t in range(1, steps + 1)]).astype(np.uint64)
    acc, margin, slack = om.decide(r["trace_delta"], None, u_acc)
    assert np.array_equal(acc, r["trace_accept"].astype(bool)) and np.all(margin >= slack)


# ---- 2. invariance, bit for bit ------------------------------------------------------------
def test_invariance(ctx):
    L, seed, init = pm.chain_inputs()["sparse-33"]
    thin = pm.CHAIN_THIN
    many = np.tile(init, (16, 1))  # 64 chains
    ctx.partition_mcmc_begin(*L.triple(), 64, seed=seed, init_part=many)
    whole = ctx.partition_mcmc_run(150, thin, trace=True)
    state = ctx.partition_mcmc_state()
    ctx.partition_mcmc_begin(*L.triple(), 64, seed=seed, init_part=many)
    a, b = ctx.partition_mcmc_run(40, thin, trace=True), ctx.partition_mcmc_run(110, thin, trace=True)
    assert a["records"] == 5 and b["records"] == 16 and b["step"] == 150
    for k in KEYS:
        assert (b[k] if k == "accepted" else np.concatenate([a[k], b[k]])).tobytes() == whole[k].tobytes(), k
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(ctx.partition_mcmc_state(), state))
    ctx.partition_mcmc_begin(*L.triple(), 3, seed=seed, init_part=many[:3])
    few = ctx.partition_mcmc_run(150, thin, trace=True)
    for k in KEYS:
        assert few[k].tobytes() == np.ascontiguousarray(whole[k][:3] if k == "accepted" else whole[k][:, :3]).tobytes(), k
    for opt, values, back in (("mcmc_waves", (1, 2, 4, 8), 4), ("mcmc_launch_steps", (1, 7, 4096), 4096)):
        for value in values:
            ctx.set_option(opt, value)
            ctx.partition_mcmc_begin(*L.triple(), 64, seed=seed, init_part=many)
            assert _same(ctx.partition_mcmc_run(150, thin, trace=True), whole), (opt, value)
        ctx.set_option(opt, back)


# ---- 3. the exact law ----------------------------------------------------------------------
def test_partitions_follow_their_exact_law_at_n4(ctx):
    L, seed, T, chains = pm.STAT[4]
    ctx.partition_mcmc_begin(*L.triple(), chains, seed=seed)
    r = ctx.partition_mcmc_run(T, T, want_parents=False)
    par, w, part, _ = pm.dag_table(L)
    law = {}
    for row, x in zip(part, w / w.sum()):
        law[tuple(row)] = law.get(tuple(row), 0.0) + float(x)
    counts = {}
    for row in r["part"][0]:
        counts[tuple(int(x) for x in row)] = counts.get(tuple(int(x) for x in row), 0) + 1
    # asserts a tail of 1e-6; the threshold here is 1e-4
    stat_line = []
    om.chi_square("partitions-4", counts, law, chains, lambda x, dof: stat_line.append(ulg.chi2_log_sf(x, dof)) or stat_line[-1])
    assert stat_line[-1] >= np.log(1e-4), stat_line
    print(f"partitions-4: acceptance {r['accepted'].sum() / (chains * T):.3f}, mean parts {r['parts'].mean():.3f}")


def test_edges_follow_the_uniform_prior_at_n5_and_order_mcmc_does_not(ctx):
    """Each edge's count over 4096 chains' one record within 5 binomial standard deviations of K p, p the exact
    uniform-prior edge posterior over all 29,281 DAGs; the order MCMC's records on the same lists miss it."""
    L, seed, T, K = pm.STAT[5]
    n = L.n
    par, w, _, _ = pm.dag_table(L)
    p = pm.edge_matrix(par, w, n)
    sd = np.sqrt(K * p * (1 - p))

    def worst(parents):
        cnt = np.array([[int((((parents[:, v] >> np.uint64(u)) & np.uint64(1)) == 1).sum()) for v in range(n)] for u in range(n)])
        off = ~np.eye(n, dtype=bool)
        assert np.all(cnt[~off] == 0)
        return float((np.abs(cnt - K * p)[off] / sd[off]).max())

    ctx.partition_mcmc_begin(*L.triple(), K, seed=seed)
    r = ctx.partition_mcmc_run(T, T)
    f = ctx.dag_features(r["parents"][0])
    assert f["total"] == K and f["cyclic"] == 0
    mine = worst(r["parents"][0])
    ctx.order_mcmc_begin(*L.triple(), K, seed=seed)
    theirs = worst(ctx.order_mcmc_run(om.STAT_T[6], om.STAT_T[6])["parents"][0])
    print(f"edges-5: partition MCMC's worst edge {mine:.2f} standard deviations, order MCMC's {theirs:.2f}")
    assert mine <= 5.0 and theirs > 5.0


# ---- 4. errors and state -------------------------------------------------------------------
def test_errors_and_families(ctx):
    L = om.make_lists(5, 55)
    offs, sets, scores = L.triple()

    def refused(status, call):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS[status], str(e.value)
        return str(e.value)

    wrong = (lambda: ctx.partition_mcmc_run(1), ctx.partition_mcmc_state, lambda: ctx.partition_score(np.zeros((1, 5), np.uint8)))
    for call in wrong:
        refused("STATE", call)
    # a list without the empty set: variable 1, chain 0
    keep = np.ones(len(sets), dtype=bool)
    keep[offs[1]] = False
    offs2 = offs.copy()
    offs2[2:] -= 1
    msg = refused("ARG", lambda: ctx.partition_mcmc_begin(offs2, sets[keep], scores[keep], 4))
    assert "chain 0" in msg and "variable 1" in msg
    rows = np.zeros((4, 5), dtype=np.uint8)
    rows[2] = [0, 2, 2, 0, 0]  # a skipped index
    assert "chain 2" in refused("ARG", lambda: ctx.partition_mcmc_begin(offs, sets, scores, 4, init_part=rows))
    rows[2] = [0, 1, 5, 0, 0]
    assert "chain 2" in refused("ARG", lambda: ctx.partition_mcmc_begin(offs, sets, scores, 4, init_part=rows))
    for call in wrong:  # a refused begin leaves no chains
        refused("STATE", call)
    ctx.partition_mcmc_begin(offs, sets, scores, 4)
    refused("ARG", lambda: ctx.partition_score(np.array([[0, 2, 2, 0, 0]], dtype=np.uint8)))
    for call in (lambda: ctx.order_mcmc_run(1), lambda: ctx.order_mc3_run(1), lambda: ctx.order_score(np.arange(5)[None, :])):
        refused("STATE", call)
    assert ulg.lib().ulg_order_mcmc_state(ctx._h, None, None, None) == STATUS["STATE"]
    ctx.order_mcmc_begin(offs, sets, scores, 4)  # a begin of another family ends these chains
    assert ulg.lib().ulg_partition_mcmc_state(ctx._h, None, None, None) == STATUS["STATE"]
    ctx.partition_mcmc_begin(offs, sets, scores, 4)
    ctx.order_mc3_begin(offs, sets, scores, 2, [1.0, 0.5])
    assert ulg.lib().ulg_partition_mcmc_run(ctx._h, 1, 1, *[None] * 9) == STATUS["STATE"]
    one = om.make_lists(1, 1)
    ctx.partition_mcmc_begin(*one.triple(), 2, seed=3)
    r = ctx.partition_mcmc_run(6, 3, trace=True)  # n = 1: nothing is proposed
    assert np.all(r["accepted"] == 0) and np.all(r["trace_delta"] == -np.inf) and np.all(r["parts"] == 1) and np.all(r["parents"] == 0)
