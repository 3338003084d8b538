"""GPU tests of the order MCMC (ulg_order_mcmc_*, ulg_order_score; kernels:
csrc/order_mcmc.hip) against tests/order_mcmc_ref.py, whose docstring derives
every cap used here; none is measured on the device.  Each comparison prints
"order-mcmc-observed <family> <input> max <fraction of its cap>".

Terms: order_mcmc_ref.term_cases() -- n = 1, 2, 5, 33, 63 (variables and
parents above bit 31 and at bit 62); "lengths-63": list lengths 1, 63, 64, 65,
255, 256, 257 (a wave's stride and the sampler's chunk, one below and above,
and four times that) and 5000 entries of which 4200 equal the maximum: the
orders that put such a list's variable last make the sum pass 2^64 (asserted
from the reference's own T, not assumed); "dynamic-6": scores of +-2e4, gaps beyond 745 nats, a variable
whose only entry is the empty set, a list without it.
Chains: equal to the reference step by step, which
tests/test_order_mcmc_ref.py shows to have no undecided step at these inputs.
"""
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so: imported after it, torch reports no HIP GPU

import order_mcmc_ref as om
import posterior_ref as pr
import ulg

pytestmark = pytest.mark.gpu

STATUS = {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}
LD = np.longdouble


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _observed(family, name, frac):
    print(f"order-mcmc-observed {family} {name} max {frac:.3g} of its cap")
    assert frac <= 1.0, (family, name, frac)


def _frac(got, want, cap):
    """The largest |got - want| / cap over the finite entries of want; the -inf patterns must agree."""
    got, want, cap = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=LD), np.asarray(cap, dtype=np.float64)
    fin = want > -np.inf
    assert np.array_equal(got > -np.inf, fin) and np.all(got[~fin] == -np.inf), "finite / -inf pattern differs"
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin].astype(LD) - want[fin]) / cap[fin]).max())


def _begin(ctx, L, chains, seed=0, init_order=None):
    ctx.order_mcmc_begin(*L.triple(), chains, seed=seed, init_order=init_order)


def _same(a, b, keys):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


RUN_KEYS = ("order", "log_score", "parents", "log_weight", "accepted")


# ---- 1. terms ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(om.term_cases()))
def test_terms(ctx, name):
    L = om.term_cases()[name]
    n = L.n
    orders = om.term_orders(name)  # "dynamic-6": variable 1 first; "lengths-63": the long lists' variables last
    if name == "dynamic-6":
        _begin(ctx, L, 1, init_order=np.arange(n, dtype=np.uint8)[None, :])  # a shuffle may put variable 1 first
    else:
        _begin(ctx, L, 1)
    got = ctx.order_score(orders)
    sums = []
    want, cap, single = om.order_terms(L, orders, sums)
    _observed("terms", name, _frac(got, want, cap))
    if name == "lengths-63":
        # the carry, on the device: scored pairs whose sum of weights is 2^64 or more (T_hi = 1), both long
        # lists; held to the cap above like every other, and here apart so that a cap met elsewhere cannot hide it
        T = np.array(sums, dtype=object).reshape(orders.shape)
        for v in om.LONG_VARS:
            k, p = np.nonzero((orders == v) & (T >= (1 << 64)))
            assert len(k) >= 2 and all(int(T[a, b]) >> 64 == 1 for a, b in zip(k, p)), (v, len(k))
            _observed("terms-carry", f"{name}-v{v}", _frac(got[k, p], want[k, p], cap[k, p]))
            assert np.all(got[k, p] >= 3.5 + np.log(4200.0))  # 4200 entries at the maximum 3.5, and more
    # one compatible entry: the score itself, to the bit
    assert single.any() and np.array_equal(got[single], want[single].astype(np.float64))
    if name == "dynamic-6":
        at = int(np.flatnonzero((orders[:, 0] == 1))[0])
        assert got[at, 0] == -np.inf
        k0 = np.argwhere(orders == 0)
        assert np.all(got[k0[:, 0], k0[:, 1]] == float(L.sc[0][0]))  # variable 0's only entry is the empty set
    # the same bits from the chains' own terms, and in a second call
    if name != "dynamic-6":
        o, t, step = ctx.order_mcmc_state()
        assert step == 0 and np.array_equal(t, ctx.order_score(o)) and np.array_equal(o, om.shuffle(0, [0], n))
    assert np.array_equal(got, ctx.order_score(orders))
    # n <= 10: against ln alpha_v of the exact path's table, within both paths' caps
    if n <= 10:
        post_cap = pr.reference("order-mcmc-" + name, n, *L.triple())["cap"]
        ctx.posterior(*L.triple())
        pre = om.prefixes(orders)
        worst = 0.0
        for v in range(n):
            alpha = ctx.posterior_table(0, v)
            k, p = np.nonzero(orders == v)
            a = alpha[pr.squeeze(pre[k, p].astype(np.int64), v)]
            fin = got[k, p] > -np.inf
            assert np.array_equal(a > -np.inf, fin)
            if fin.any():
                worst = max(worst, float((np.abs(a[fin] - got[k, p][fin]) / (cap[k, p][fin] + post_cap)).max()))
        _observed("terms-vs-alpha", name, worst)


# ---- 2. chains against the reference -------------------------------------------------------
@pytest.mark.parametrize("chains", om.CHAIN_COUNTS)
@pytest.mark.parametrize("name", sorted(om.chain_inputs()))
def test_chains_equal_the_reference(ctx, name, chains):
    L, seed = om.chain_inputs()[name]
    ref = om.chain_reference(name)
    n, steps, thin = L.n, om.CHAIN_STEPS, om.CHAIN_THIN
    _begin(ctx, L, chains, seed=seed)
    o0, t0, step = ctx.order_mcmc_state()
    assert step == 0 and np.array_equal(o0, om.shuffle(seed, np.arange(chains), n))
    r = ctx.order_mcmc_run(steps, thin, trace=True)
    assert r["records"] == steps // thin == ref["records"] and r["step"] == steps
    c = slice(0, chains)
    assert np.array_equal(r["trace_accept"].astype(bool), ref["trace_accept"][:, c])
    assert np.array_equal(r["accepted"], ref["accepted"][c])
    assert np.array_equal(r["order"], ref["order"][:, c])
    assert np.array_equal(r["parents"], ref["parents"][:, c])
    assert np.array_equal(r["log_weight"], ref["log_weight"][:, c])
    o1, t1, step = ctx.order_mcmc_state()
    assert step == steps and np.array_equal(o1, ref["final_order"][c])
    _observed("delta", f"{name}-{chains}", _frac(r["trace_delta"], ref["trace_delta"][:, c], np.maximum(ref["trace_cap"][:, c], 1e-300)))
    _observed("log-score", f"{name}-{chains}", _frac(r["log_score"], ref["log_score"][:, c], ref["score_cap"][:, c]))
    _observed("final-terms", f"{name}-{chains}", _frac(t1, ref["final_terms"][c], ref["final_cap"][c]))
    # every decision again, from the device's own delta bits: the slack is exp's 8 units alone
    u_acc = np.stack([om.moves(seed, t, np.arange(chains), n)[2] for t in range(1, steps + 1)])
    acc, margin, slack = om.decide(r["trace_delta"], None, u_acc)
    assert np.array_equal(acc, r["trace_accept"].astype(bool))
    assert np.all(margin >= slack), int((margin - slack).min())
    # log_score is the full sum of the state's terms
    tot = np.zeros(chains)
    for p in range(n):
        tot = tot + t1[:, p]
    if steps % thin == 0:
        assert np.array_equal(tot, r["log_score"][-1])


# ---- 3. invariance, bit for bit ------------------------------------------------------------
def test_invariance(ctx):
    L, seed = om.chain_inputs()["sparse-33"]
    n, thin = L.n, om.CHAIN_THIN
    _begin(ctx, L, 64, seed=seed)
    whole = ctx.order_mcmc_run(200, thin, trace=True)
    state = ctx.order_mcmc_state()
    # run(50); run(150)
    _begin(ctx, L, 64, seed=seed)
    a = ctx.order_mcmc_run(50, thin, trace=True)
    b = ctx.order_mcmc_run(150, thin, trace=True)
    assert a["records"] == 7 and b["records"] == 21 and b["step"] == 200
    for k in ("order", "log_score", "parents", "log_weight", "trace_delta", "trace_accept"):
        assert np.concatenate([a[k], b[k]]).tobytes() == whole[k].tobytes(), k
    assert np.array_equal(b["accepted"], whole["accepted"])
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(ctx.order_mcmc_state(), state))
    # the first 8 chains of 64 are a run of 8 chains; in a second context
    other = ulg.Context(0)
    try:
        _begin(other, L, 8, seed=seed)
        few = other.order_mcmc_run(200, thin, trace=True)
    finally:
        other.close()
    for k in ("order", "log_score", "parents", "log_weight", "trace_delta", "trace_accept"):
        assert few[k].tobytes() == np.ascontiguousarray(whole[k][:, :8]).tobytes(), k
    assert np.array_equal(few["accepted"], whole["accepted"][:8])
    # the waves of a chain's workgroup, the steps of a launch
    for opt, values, back in (("mcmc_waves", (1, 2, 4, 8), 4), ("mcmc_launch_steps", (7, 4096), 4096)):
        for value in values:
            ctx.set_option(opt, value)
            _begin(ctx, L, 64, seed=seed)
            again = ctx.order_mcmc_run(200, thin, trace=True)
            assert _same(again, whole, RUN_KEYS + ("trace_delta", "trace_accept")), (opt, value)
        ctx.set_option(opt, back)
    for opt, bad in (("mcmc_waves", 3), ("mcmc_waves", 16), ("mcmc_launch_steps", 0)):
        with pytest.raises(ulg.ULGError):
            ctx.set_option(opt, bad)
    # an order given is the order shuffled
    _begin(ctx, L, 64, seed=seed, init_order=om.shuffle(seed, np.arange(64), n).astype(np.uint8))
    assert _same(ctx.order_mcmc_run(200, thin, trace=True), whole, RUN_KEYS + ("trace_delta", "trace_accept"))
    # records that are not asked for change nothing else
    _begin(ctx, L, 64, seed=seed)
    bare = ctx.order_mcmc_run(200, thin, want_order=False, want_parents=False)
    assert set(bare) == {"log_score", "accepted", "records", "step"} and _same(bare, whole, ("log_score", "accepted"))


# ---- 4. stationarity on the device ---------------------------------------------------------
def test_orders_follow_their_exact_law_at_n4(ctx):
    L, seed, T, chains = om.stat_inputs()[4]
    _begin(ctx, L, chains, seed=seed)
    r = ctx.order_mcmc_run(T, T, want_parents=False)
    assert r["records"] == 1
    perms, pi = om.order_law(L)
    counts = {}
    for o in r["order"][0]:
        key = tuple(int(x) for x in o)
        counts[key] = counts.get(key, 0) + 1
    om.chi_square("orders-4", counts, {p: float(x) for p, x in zip(perms, pi)}, chains, ulg.chi2_log_sf)
    print(f"orders-4: acceptance {r['accepted'].sum() / (chains * T):.3f}")


def test_edge_frequencies_against_the_exact_posterior_at_n6(ctx):
    """Each edge's count over 4096 independent chains' one record within 5 binomial standard deviations
    of K p, p = ulg_posterior's exact edge matrix on the same context (the linear-extension tests' bound)."""
    L, seed, T, K = om.stat_inputs()[6]
    n = L.n
    _begin(ctx, L, K, seed=seed)
    r = ctx.order_mcmc_run(T, T)
    par = r["parents"][0]
    _, edge, _ = ctx.posterior(*L.triple())
    worst = 0.0
    for u in range(n):
        for v in range(n):
            cnt = int((((par[:, v] >> np.uint64(u)) & np.uint64(1)) == 1).sum())
            p = float(edge[u, v])
            sd = np.sqrt(K * p * max(1 - p, 0.0))
            dev = abs(cnt - K * p)
            assert dev <= 5 * sd, ("edge", u, v, cnt, K * p, dev / sd if sd else np.inf)
            worst = max(worst, dev / sd if sd else 0.0)
    print(f"edges-6: {n * n} edges over {K} chains, the largest deviation {worst:.2f} standard deviations")
    # the features take the records as they are
    f = ctx.dag_features(par)
    assert f["total"] == K and f["cyclic"] == 0
    assert np.array_equal(f["edge"], np.array([[int((((par[:, v] >> np.uint64(u)) & np.uint64(1)) == 1).sum()) for v in range(n)]
                                                for u in range(n)], dtype=np.uint64))


# ---- 5. errors and state -------------------------------------------------------------------
def test_errors(ctx):
    L = om.make_lists(5, 55)
    offs, sets, scores = L.triple()
    for call in (lambda: ctx.order_mcmc_run(1), ctx.order_mcmc_state, lambda: ctx.order_score(np.arange(5)[None, :])):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS["STATE"]

    def refused(status, *args, **kw):
        with pytest.raises(ulg.ULGError) as e:
            ctx.order_mcmc_begin(*args, **kw)
        assert _status(e) == STATUS[status], str(e.value)
        return str(e.value)

    bad = offs.copy()
    bad[2], bad[3] = bad[3], bad[2]
    assert "ascending" in refused("ARG", bad, sets, scores, 4)
    own = sets.copy()
    own[offs[2] + 1] |= np.uint64(1 << 2)
    assert "own variable" in refused("ARG", offs, own, scores, 4)
    high = sets.copy()
    high[offs[1] + 1] |= np.uint64(1 << 5)
    assert "bit >= n" in refused("ARG", offs, high, scores, 4)
    dup = sets.copy()
    dup[offs[3] + 2] = dup[offs[3] + 1]
    assert "twice" in refused("ARG", offs, dup, scores, 4)
    for x in (np.nan, np.inf, -np.inf):
        s2 = scores.copy()
        s2[7] = x
        assert "NaN or infinite" in refused("ARG", offs, sets, s2, 4)
    refused("ARG", offs, sets, scores, 0)
    refused("ARG", offs, sets, scores, (1 << 20) + 1)
    refused("ARG", offs[:1], sets, scores, 4)  # n = 0
    n64 = np.zeros(65, dtype=np.int64)
    refused("UNSUPPORTED", n64, sets[:1], scores[:1], 4)
    rows = np.tile(np.arange(5, dtype=np.uint8), (4, 1))
    rows[2, 4] = 3
    assert "chain 2" in refused("ARG", offs, sets, scores, 4, init_order=rows)
    rows[2, 4] = 5
    assert "chain 2" in refused("ARG", offs, sets, scores, 4, init_order=rows)
    # an initial order of probability 0: variable 1 without the empty set, first in chain 3
    keep = np.ones(len(sets), dtype=bool)
    keep[offs[1]] = False
    assert sets[offs[1]] == 0
    offs2 = offs.copy()
    offs2[2:] -= 1
    rows = np.tile(np.arange(5, dtype=np.uint8), (5, 1))
    rows[3] = [1, 0, 2, 3, 4]
    assert "chain 3" in refused("ARG", offs2, sets[keep], scores[keep], 5, init_order=rows)
    # a refused begin leaves no chains
    with pytest.raises(ulg.ULGError) as e:
        ctx.order_mcmc_run(1)
    assert _status(e) == STATUS["STATE"]
    _begin(ctx, L, 4)
    for steps, thin in ((-1, 1), (1, 0), (1, -3)):
        with pytest.raises(ulg.ULGError) as e:
            ctx.order_mcmc_run(steps, thin)
        assert _status(e) == STATUS["ARG"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.order_score(np.array([[0, 1, 2, 3, 3]], dtype=np.uint8))
    assert _status(e) == STATUS["ARG"]
    # records beyond the device memory: refused before anything is allocated, the chains as they were
    live = ctx.info("device_bytes_live")
    before = ctx.order_mcmc_state()
    rc = ulg.lib().ulg_order_mcmc_run(ctx._h, 1 << 40, 1, None, None, None, None, None, ulg._ptr(np.zeros(1)), None, None)
    assert rc == STATUS["UNSUPPORTED"] and ctx.info("device_bytes_live") == live
    assert all(np.array_equal(x, y) for x, y in zip(before, ctx.order_mcmc_state()))
    zero = ctx.order_mcmc_run(0, 1)
    assert zero["records"] == 0 and zero["order"].shape == (0, 4, 5) and np.all(zero["accepted"] == 0)
    # every refused begin ends the chains of the one before, in the library itself (the binding aside):
    # refused for its arguments alone, for its offsets, on the device, and for the context's state
    state = lambda: ulg.lib().ulg_order_mcmc_state(ctx._h, None, None, None)  # noqa: E731
    for args, kw in (((offs, sets, scores, 0), {}), ((offs, sets, scores, 4), {"init_order": np.zeros((4, 5), dtype=np.uint8)}),
                     ((bad, sets, scores, 4), {}), ((offs, dup, scores, 4), {}), (None, None)):
        _begin(ctx, L, 4)
        assert state() == 0
        with pytest.raises(ulg.ULGError) as e:
            if args is None:
                ctx.order_mcmc_begin_from_scores(4)  # no scoring call in this context
            else:
                ctx.order_mcmc_begin(*args, **kw)
        assert _status(e) == (STATUS["STATE"] if args is None else STATUS["ARG"])
        assert state() == STATUS["STATE"]
        assert ulg.lib().ulg_order_score(ctx._h, 0, None, None) == STATUS["STATE"]


def test_one_variable(ctx):
    L = om.make_lists(1, 1)
    _begin(ctx, L, 3, seed=9)
    r = ctx.order_mcmc_run(10, 3, trace=True)
    assert r["records"] == 3 and r["step"] == 10 and np.all(r["accepted"] == 0)
    assert np.all(r["order"] == 0) and np.all(r["parents"] == 0) and np.all(r["trace_accept"] == 0) and np.all(r["trace_delta"] == -np.inf)
    assert np.all(r["log_score"] == float(L.sc[0][0])) and np.all(r["log_weight"] == float(L.sc[0][0]))
    assert ctx.order_mcmc_run(2, 3)["records"] == 1  # steps 11, 12: the record of t = 12


def test_state_and_neighbours(ctx):
    """A posterior call frees the chains; begin and run leave the tables, the context's lists and a
    following posterior_sample as they were."""
    import synth
    X, _ = synth.gaussian_sem(6, 500, 77)
    ctx.load(X, 2.0)
    full = [(1 << 6) - 1] * 6
    offs, sets, scores = ctx.score_all(list(range(6)), full, 3)
    fetched = ctx.fetch(int(offs[-1]))
    lz, edge, lp = ctx.posterior_from_scores()
    tables = [ctx.posterior_table(1), ctx.posterior_table(0, 2)]
    sample = ctx.posterior_sample(50, seed=4)
    ctx.order_mcmc_begin_from_scores(16, seed=5)
    r = ctx.order_mcmc_run(40, 4)
    # the lists of the scoring call are the lists given by hand
    other = ulg.Context(0)
    try:
        other.order_mcmc_begin(offs, sets, scores, 16, seed=5)
        assert _same(other.order_mcmc_run(40, 4), r, RUN_KEYS)
    finally:
        other.close()
    assert all(np.array_equal(x, y) for x, y in zip(fetched, ctx.fetch(int(offs[-1]))))
    assert np.array_equal(tables[0], ctx.posterior_table(1)) and np.array_equal(tables[1], ctx.posterior_table(0, 2))
    assert all(np.array_equal(x, y) for x, y in zip(sample, ctx.posterior_sample(50, seed=4)))
    assert ctx.order_mcmc_run(4, 4)["step"] == 44  # the chains are still there after the sampler ran
    again = ctx.posterior_from_scores()
    assert again[0] == lz and np.array_equal(again[1], edge)
    for call in (lambda: ctx.order_mcmc_run(1), ctx.order_mcmc_state):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS["STATE"]
