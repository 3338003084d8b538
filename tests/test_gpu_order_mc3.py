"""ulg_order_mc3_* on the GPU against tests/order_mc3_ref.py: ladders equal the reference (decisions,
exchanges, records and state equal; deltas, d, sums and terms within their derived caps), one rung equals
the chains' bytes, invariance bit for bit, the two rungs' laws at n = 4, errors and neighbours.
tests/test_order_mc3_ref.py shows that no input here has an undecided step."""
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import order_mc3_ref as m3
import order_mcmc_ref as om
import ulg
from test_gpu_order_mcmc import _frac, _observed, _same

pytestmark = pytest.mark.gpu

KEYS = ("order", "log_score", "parents", "log_weight", "accepted", "swaps", "trace_delta", "trace_accept", "trace_swap_d",
        "trace_swap_accept")


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _run(c, L, ladders, betas, E, seed, steps, thin, split=(), **kw):
    """begin, then the steps in the pieces given -> (the pieces' outputs joined, state)."""
    c.order_mc3_begin(*L.triple(), ladders, betas, swap_every=E, seed=seed, init_order=kw.pop("init_order", None))
    parts = [c.order_mc3_run(s, thin, trace=True, **kw) for s in (*split, steps - sum(split))]
    out = {k: np.concatenate([p[k] for p in parts]) for k in KEYS[:4] + KEYS[6:] if k in parts[0]}
    out.update(accepted=parts[-1]["accepted"], swaps=parts[-1]["swaps"])
    return out, c.order_mc3_state()


@pytest.mark.parametrize("ladders", (1, 3))
@pytest.mark.parametrize("R,E", m3.LADDER_CASES)
@pytest.mark.parametrize("name", sorted(om.chain_inputs()))
def test_ladders_equal_the_reference(ctx, name, R, E, ladders):
    L, seed = om.chain_inputs()[name]
    ref, betas = m3.ladder_reference(name, R, E), ulg.geometric_betas(R, 0.1)
    assert np.array_equal(betas, m3.geometric(R))
    r, (order, terms, replica, step) = _run(ctx, L, ladders, betas, E, seed, m3.LADDER_STEPS, om.CHAIN_THIN)
    l = slice(0, ladders)
    for got, want in (("trace_accept", "trace_accept"), ("trace_swap_accept", "swap_accept"), ("accepted", "accepted"), ("swaps", "swaps"),
                      ("order", "order"), ("parents", "parents"), ("log_weight", "log_weight")):
        assert np.array_equal(r[got], ref[want][l] if got in ("accepted", "swaps") else ref[want][:, l]), got
    assert step == m3.LADDER_STEPS and np.array_equal(replica, ref["replica"][l]) and np.array_equal(order, ref["final_order"][l])
    tag = f"{name}-R{R}-L{ladders}"
    _observed("mc3-delta", tag, _frac(r["trace_delta"], ref["trace_delta"][:, l], np.maximum(ref["trace_cap"][:, l], 1e-300)))
    _observed("mc3-swap-d", tag, _frac(r["trace_swap_d"], ref["swap_d"][:, l], np.maximum(ref["swap_cap"][:, l], 1e-300)))
    _observed("mc3-log-score", tag, _frac(r["log_score"], ref["log_score"][:, l], ref["score_cap"][:, l]))
    _observed("mc3-final-terms", tag, _frac(terms, ref["final_terms"][l], ref["final_cap"][l]))
    # every decision again from the device's own delta and d bits: exp's 8 units alone
    ks = (np.arange(ladders)[:, None] * R + np.arange(R)[None, :]).ravel()
    who = np.tile(np.arange(R), (ladders, 1))  # who[l, r]: the slot on rung r
    u_acc, rounds = np.empty((m3.LADDER_STEPS, ladders * R), dtype=np.uint64), 0
    for t in range(1, m3.LADDER_STEPS + 1):
        rows = (np.arange(ladders)[:, None] * R + who).ravel()
        u_acc[t - 1] = om.moves(seed, t, ks, L.n)[2][rows]
        if t % E == 0:
            for p in np.flatnonzero(np.isfinite(r["trace_swap_d"][rounds, 0])):
                a, b, on = who[:, p].copy(), who[:, p + 1].copy(), r["trace_swap_accept"][rounds, :, p].astype(bool)
                who[:, p], who[:, p + 1] = np.where(on, b, a), np.where(on, a, b)
            rounds += 1
    tempered = r["trace_delta"].reshape(m3.LADDER_STEPS, -1) * np.tile(betas, ladders)[None, :]  # FP64: the device's multiply
    acc, margin, slack = om.decide(tempered, None, u_acc)
    assert np.array_equal(acc, r["trace_accept"].reshape(acc.shape).astype(bool)) and np.all(margin >= slack)
    cs = (np.arange(ladders)[:, None] * R + np.arange(R - 1)[None, :]).ravel()
    u = np.stack([(lambda w: w[0] | (w[1] << np.uint64(32)))(om._draw(seed, x * E, cs, m3.SWAP_DOMAIN)) for x in range(1, rounds + 1)])
    acc, margin, slack = om.decide(r["trace_swap_d"].reshape(rounds, -1), None, u)
    assert np.array_equal(acc, r["trace_swap_accept"].reshape(acc.shape).astype(bool)) and np.all(margin >= slack)


def test_one_rung_is_the_chains_bytes(ctx):
    L, seed = om.chain_inputs()["sparse-33"]
    r, (order, terms, replica, step) = _run(ctx, L, 64, [1.0], 5, seed, 200, om.CHAIN_THIN)
    ctx.order_mcmc_begin(*L.triple(), 64, seed=seed)
    want, state = ctx.order_mcmc_run(200, om.CHAIN_THIN, trace=True), ctx.order_mcmc_state()
    for k in ("order", "log_score", "parents", "log_weight", "trace_delta", "trace_accept", "accepted"):
        assert r[k].tobytes() == want[k].tobytes(), k
    assert order.tobytes() == state[0].tobytes() and terms.tobytes() == state[1].tobytes() and step == state[2]
    assert np.array_equal(replica[:, 0], np.arange(64)) and r["swaps"].size == 0 and r["trace_swap_d"].size == 0


def test_invariance(ctx):
    L, seed = om.chain_inputs()["sparse-33"]
    betas, thin = ulg.geometric_betas(4, 0.1), om.CHAIN_THIN
    whole, state = _run(ctx, L, 64, betas, 3, seed, 200, thin)
    same = lambda a, b: _same(a[0], b[0], KEYS) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[1], b[1]))  # noqa: E731
    assert same(_run(ctx, L, 64, betas, 3, seed, 200, thin, split=(50,)), (whole, state))
    other = ulg.Context(0)
    try:
        few, few_state = _run(other, L, 8, betas, 3, seed, 200, thin)
    finally:
        other.close()
    cut = {k: np.ascontiguousarray(v[:8] if k in ("accepted", "swaps") else v[:, :8]) for k, v in whole.items()}
    assert same((few, few_state[:3]), (cut, [x[:8] for x in state[:3]]))
    for opt, values, back in (("mc3_waves", (1, 2, 4, 8, 16), 16), ("mcmc_launch_steps", (7,), 4096)):
        for value in values:
            ctx.set_option(opt, value)
            assert same(_run(ctx, L, 64, betas, 3, seed, 200, thin), (whole, state)), (opt, value)
        ctx.set_option(opt, back)
    init = om.shuffle(seed, np.arange(64 * 4), L.n).astype(np.uint8)
    assert same(_run(ctx, L, 64, betas, 3, seed, 200, thin, init_order=init), (whole, state))
    bare, bare_state = _run(ctx, L, 64, betas, 3, seed, 200, thin, want_order=False, want_parents=False)
    assert "order" not in bare and "parents" not in bare and "log_weight" not in bare
    assert same(({**whole, **bare}, bare_state), (whole, state))


def test_both_rungs_follow_their_exact_laws_at_n4(ctx):
    L, K, T = om.stat_inputs()[4][0], 4096, m3.STAT_T[4]
    ctx.order_mc3_begin(*L.triple(), K, m3.STAT_BETAS, swap_every=1, seed=m3.STAT_SEED)
    r = ctx.order_mc3_run(T, T, want_parents=False)
    order = ctx.order_mc3_state()[0]
    assert r["records"] == 1 and np.array_equal(order[:, 0], r["order"][0])
    perms, pi, hot = m3.ladder_law(L, m3.STAT_BETAS)
    for rung, law in ((0, pi), (1, hot)):
        keys, cnt = np.unique(order[:, rung], axis=0, return_counts=True)
        counts = {tuple(int(x) for x in k): int(c) for k, c in zip(keys, cnt)}
        om.chi_square(f"mc3-rung-{rung}", counts, {p: float(x) for p, x in zip(perms, law)}, K, ulg.chi2_log_sf)
    print(f"mc3-4: acceptance by rung {r['accepted'].mean(axis=0) / T}, swaps {r['swaps'].mean() / (T // 2):.3f}")


def test_errors_and_neighbours(ctx):
    status = lambda e: int(re.search(r"status (\d+)", str(e.value)).group(1))  # noqa: E731
    L, seed = om.chain_inputs()["k3-8"]
    for call in (lambda: ctx.order_mc3_run(1), ctx.order_mc3_state):  # before any begin
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert status(e) == 3
    ctx.order_mcmc_begin(*L.triple(), 4, seed=seed)
    no_empty = om.Lists(2, [0, 1, 2], [0, 1], [0.0, 0.0])  # variable 1 needs variable 0 before it
    bad = [dict(betas=[1.0] * 17), dict(betas=[]), dict(ladders=(1 << 20) // 2 + 1, betas=[1.0, 0.5]), dict(ladders=0), dict(betas=[0.9, 0.5]),
           dict(betas=[1.0, 1.0]), dict(betas=[1.0, 0.5, 0.7]), dict(betas=[1.0, 0.0]), dict(betas=[1.0, -0.5]), dict(betas=[1.0, np.nan]),
           dict(betas=[np.inf, 1.0]), dict(swap_every=0), dict(lists=no_empty, init_order=np.array([[0, 1], [1, 0]], dtype=np.uint8))]
    for kw in bad:
        args = dict(lists=L, ladders=1, betas=[1.0, 0.5], swap_every=1, init_order=None)
        args.update(kw)
        with pytest.raises(ulg.ULGError) as e:
            ctx.order_mc3_begin(*args["lists"].triple(), args["ladders"], args["betas"], swap_every=args["swap_every"], seed=seed,
                                init_order=args["init_order"])
        assert status(e) == 1, kw
        for call in (lambda: ctx.order_mc3_run(1), lambda: ctx.order_mcmc_run(1), lambda: ctx.order_score(np.arange(8)[None, :])):
            with pytest.raises(ulg.ULGError) as e:  # a refused begin ended the chains too
                call()
            assert status(e) == 3, kw
    assert ulg.lib().ulg_order_mc3_begin_from_scores(ctx._h, 1, 2, None, 1, 0, None) == 1  # betas NULL
    # a begin of one kind ends the other's; the lists serve order_score and order_edges either way
    ctx.order_mc3_begin(*L.triple(), 2, [1.0, 0.5], swap_every=2, seed=seed)
    with pytest.raises(ulg.ULGError) as e:
        ctx.order_mcmc_run(1)
    assert status(e) == 3
    orders = ctx.order_mc3_state()[0][:, 0]
    terms, (edge, zero) = ctx.order_score(orders), ctx.order_edges(orders)
    ctx.order_mcmc_begin(*L.triple(), 2, seed=seed)
    with pytest.raises(ulg.ULGError) as e:
        ctx.order_mc3_run(1)
    assert status(e) == 3
    assert terms.tobytes() == ctx.order_score(orders).tobytes() and edge.tobytes() == ctx.order_edges(orders)[0].tobytes() and zero == 0
    # n = 1: nothing moves, every exchange has d = 0 and is accepted
    one = om.Lists(1, [0, 1], [0], [-1.5])
    ctx.order_mc3_begin(*one.triple(), 2, [1.0, 0.5, 0.25], swap_every=1, seed=seed)
    r = ctx.order_mc3_run(4, 2, trace=True)
    assert not r["trace_accept"].any() and np.all(r["trace_delta"] == -np.inf) and np.all(r["log_score"] == np.float32(-1.5))
    assert np.array_equal(r["swaps"], [[2, 2], [2, 2]]) and np.all(r["parents"] == 0) and r["records"] == 2
