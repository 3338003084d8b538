"""GPU tests of the window re-optimisation (ulg_order_window; kernel: csrc/order_window.hip)
against tests/order_window_ref.py.  Every value of the contract is a maximum of float32
scores or a fixed FP64 sum of such: every comparison here is equality, of bits where sums
are compared.  tests/test_order_window_ref.py shows on the CPU which events these cases meet."""
import functools
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import order_search_ref as osr
import order_window_ref as owr
import ulg

pytestmark = pytest.mark.gpu

KEYS = ("orders", "terms", "score", "parents", "accepted", "sweeps")


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def reference(case):
    name, width, stride, max_sweeps = case
    return owr.run_many(osr.inputs()[name][0], owr.case_orders(name), width, stride, max_sweeps)


def _begin(ctx, name):
    L, seed, tenure, patience = osr.inputs()[name]  # a begin refuses a search whose shuffled order has a -inf term
    ctx.order_search_begin(*L.triple(), 1, seed=seed, tenure=tenure, patience=patience)
    return L


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


@pytest.mark.parametrize("case", owr.CASES, ids=lambda c: "-".join(map(str, c)))
def test_windows_equal_the_restatement(ctx, case):
    name, width, stride, max_sweeps = case
    _begin(ctx, name)
    orders = np.array(owr.case_orders(name), dtype=np.uint8)
    r, ref = ctx.order_window(orders, width, stride, max_sweeps), reference(case)
    for k in KEYS:
        assert r[k].dtype == ref[k].dtype and r[k].tobytes() == ref[k].tobytes(), k
    terms, parents = ctx.order_best(r["orders"])
    assert terms.tobytes() == r["terms"].tobytes() and parents.tobytes() == r["parents"].tobytes()


def test_invariance(ctx):
    L = _begin(ctx, "n33")
    rng = np.random.default_rng(3)
    orders = np.array([rng.permutation(L.n) for _ in range(64)], dtype=np.uint8)
    whole = ctx.order_window(orders, 6, 3, 2)
    few = ctx.order_window(orders[:3], 6, 3, 2)
    assert _same(few, {k: np.ascontiguousarray(whole[k][:3]) for k in KEYS})
    assert _same(few, owr.run_many(L, orders[:3], 6, 3, 2))
    for waves in (1, 2, 4, 16, 8):
        ctx.set_option("window_waves", waves)
        assert _same(ctx.order_window(orders, 6, 3, 2), whole), waves
    one = ctx.order_window(orders, 6, 3, 1)
    two = ctx.order_window(one["orders"], 6, 3, 1)
    for k in ("orders", "terms", "score", "parents"):
        assert two[k].tobytes() == whole[k].tobytes(), k
    assert np.array_equal(one["accepted"] + two["accepted"], whole["accepted"])
    # a second call's only sweep repeats the first's where that one accepted nothing
    assert np.array_equal(np.where(one["accepted"] > 0, 2, 1), whole["sweeps"]) and (two["sweeps"] == 1).all()


def test_refusals(ctx):
    def status(*a, **kw):
        with pytest.raises(ulg.ULGError) as e:
            ctx.order_window(*a, **kw)
        return int(re.search(r"status (\d+)", str(e.value)).group(1))

    ARG, STATE = 1, 3
    good = np.array([[4, 3, 2, 1, 0]], dtype=np.uint8)
    assert status(good, 3) == STATE  # no begin
    _begin(ctx, "n5")
    assert status(good, 1) == ARG and status(good, 13) == ARG
    assert status(good, 3, stride=4) == ARG and status(good, 3, max_sweeps=0) == ARG
    with pytest.raises(ulg.ULGError, match="order 1 is not a permutation"):
        ctx.order_window(np.array([[4, 3, 2, 1, 0], [0, 1, 2, 3, 3], [9, 9, 9, 9, 9]], dtype=np.uint8), 3)
    r = ctx.order_window(good[:0], 3)  # count = 0 returns at once
    assert r["orders"].shape == (0, 5) and r["score"].shape == (0,)
    ctx.order_mcmc_begin(*osr.inputs()["n8"][0].triple(), 2, seed=1)
    assert status(good, 3) == STATE  # the chains' begin ended the searches
