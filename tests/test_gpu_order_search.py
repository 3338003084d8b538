"""GPU tests of the order search (ulg_order_search_*, ulg_order_best; kernels:
csrc/order_search.hip) against tests/order_search_ref.py.  Every value of the contract is
a maximum of float32 scores or a fixed FP64 expression of such, without a transcendental:
the tolerance derived for every comparison here is equality, of bits where sums are compared.
tests/test_order_search_ref.py shows on the CPU which events the inputs meet and that the
n8 input's 64 searches reach the optimum."""
import functools
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import order_search_ref as osr
import ulg
from test_order_search_ref import STEPS, optimum

pytestmark = pytest.mark.gpu

KEYS = ("trace_gain", "trace_pos", "best_score", "best_order", "best_parents", "moves", "kicks")
ROWS = ("trace_gain", "trace_pos")  # (steps, searches); the others are (searches, ..)


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def reference(name, searches=4):
    L, seed, tenure, patience = osr.inputs()[name]
    return osr.run([osr.Search(L, seed, c, tenure, patience) for c in range(searches)], STEPS)


def _begin(ctx, name, searches, **kw):
    L, seed, tenure, patience = osr.inputs()[name]
    ctx.order_search_begin(*L.triple(), searches, seed=seed, tenure=tenure, patience=patience, **kw)
    return L


def _bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("name", sorted(osr.inputs()))
def test_searches_equal_the_restatement(ctx, name):
    L, ref = _begin(ctx, name, 4), reference(name)
    r = ctx.order_search_run(STEPS, trace=True)
    assert r["step"] == STEPS
    for k in KEYS:
        assert np.array_equal(r[k], ref[k]), k
    order, terms, score, step = ctx.order_search_state()
    assert step == STEPS and np.array_equal(order, ref["order"]) and np.array_equal(terms, ref["terms"])
    assert _bits(r["best_score"], ref["best_score"]) and _bits(score, ref["score"])
    # ulg_order_best: the run's own terms and parents on the final and the best orders
    assert _bits(ctx.order_best(order)[0], terms)
    bt, bp = ctx.order_best(r["best_order"])
    assert np.array_equal(bp, r["best_parents"]) and np.array_equal(bt, [osr.order_best(L, o)[0] for o in r["best_order"]])


@pytest.mark.parametrize("name", ["n5", "n63"])
def test_order_best_equals_a_direct_maximum(ctx, name):
    L = _begin(ctx, name, 1)
    rng = np.random.default_rng(5)
    orders = np.array([rng.permutation(L.n) for _ in range(40)], dtype=np.uint8)
    terms, parents = ctx.order_best(orders)
    want = [osr.order_best(L, o) for o in orders]
    assert np.array_equal(terms, [w[0] for w in want]) and np.array_equal(parents, np.array([w[1] for w in want], dtype=np.uint64))
    assert np.isinf(terms).any() == (name == "n5")  # the -inf pattern is part of the equality above


def test_invariance(ctx):
    _begin(ctx, "n33", 64)
    whole = ctx.order_search_run(STEPS, trace=True)
    state = ctx.order_search_state()
    ref = reference("n33")
    assert all(np.array_equal(whole[k][:, :4] if k in ROWS else whole[k][:4], ref[k]) for k in KEYS)
    _begin(ctx, "n33", 64)
    a, b = ctx.order_search_run(40, trace=True), ctx.order_search_run(110, trace=True)
    assert b["step"] == STEPS
    for k in KEYS:
        assert _bits(np.concatenate([a[k], b[k]]) if k in ROWS else b[k], whole[k]), k
    assert all(_bits(x, y) for x, y in zip(ctx.order_search_state(), state))
    _begin(ctx, "n33", 3)
    few = ctx.order_search_run(STEPS, trace=True)
    for k in KEYS:
        assert _bits(few[k], np.ascontiguousarray(whole[k][:, :3] if k in ROWS else whole[k][:3])), k
    for opt, values, back in (("mcmc_waves", (1, 2, 4, 8), 4), ("mcmc_launch_steps", (1, 7, 4096), 4096)):
        for value in values:
            ctx.set_option(opt, value)
            _begin(ctx, "n33", 64)
            r = ctx.order_search_run(STEPS, trace=True)
            assert all(_bits(r[k], whole[k]) for k in KEYS), (opt, value)
        ctx.set_option(opt, back)


def test_reachability(ctx):
    L = _begin(ctx, "n8", 64)
    r = ctx.order_search_run(STEPS)
    assert _bits(r["best_score"], reference("n8", 64)["best_score"])
    c = int(np.argmax(r["best_score"]))
    assert np.longdouble(r["best_score"][c]) == optimum(L)
    before = 0  # acyclic: along the best order every parent stands before its child
    for v in r["best_order"][c]:
        assert int(r["best_parents"][c, v]) & ~before == 0
        before |= 1 << int(v)


def test_refusals(ctx):
    def status(call, *a, **kw):
        with pytest.raises(ulg.ULGError) as e:
            call(*a, **kw)
        return int(re.search(r"status (\d+)", str(e.value)).group(1))

    ARG, STATE = 1, 3
    assert status(ulg.Context.order_search_run, ctx, 1) == STATE  # no begin
    L, seed, tenure, patience = osr.inputs()["n5"]
    twice = np.array([[0, 1, 2, 3, 3]], dtype=np.uint8)
    assert status(ctx.order_search_begin, *L.triple(), 1, init_order=twice) == ARG
    rooted_first = np.array([[0, 1, 2, 3, 4]], dtype=np.uint8)  # variable 0 has no empty set: a -inf term
    assert status(ctx.order_search_begin, *L.triple(), 1, init_order=rooted_first) == ARG
    assert status(ctx.order_search_state) == STATE  # a refused begin leaves none
    assert status(ctx.order_search_begin, *L.triple(), 1, tenure=-1) == ARG
    assert status(ctx.order_search_begin, *L.triple(), 1, patience=0) == ARG
    ctx.order_mcmc_begin(*osr.inputs()["n8"][0].triple(), 2, seed=1)
    ctx.order_search_begin(*osr.inputs()["n8"][0].triple(), 2, seed=1, tenure=2, patience=9)
    assert status(ctx.order_mcmc_run, 5) == STATE  # the search's begin ended the chains
    ctx.order_search_run(5)
    ctx.order_mcmc_begin(*osr.inputs()["n8"][0].triple(), 2, seed=1)
    assert status(ctx.order_search_run, 5) == STATE  # ... and theirs ends the searches
