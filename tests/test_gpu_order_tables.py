"""GPU tests of the order search over dense candidate-set tables (option "search_tables",
ulg_order_search_table; kernels: csrc/order_tables.hip) against tests/order_search_ref.py,
which knows nothing of tables.  A table slot is a maximum of integer keys and a search over
tables the same fixed FP64 expressions as one over lists: every comparison is equality.

An empty list gives every order a -inf term, which a begin refuses, so no table of one can
be read back here: bin/order_tables_check holds that case on the host, and K = 0 below is
the list of the empty set alone."""
import functools
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import order_mcmc_ref as om
import order_search_ref as osr
import ulg
from test_order_search_ref import STEPS

pytestmark = pytest.mark.gpu

KEYS = ("trace_gain", "trace_pos", "best_score", "best_order", "best_parents", "moves", "kicks")
ROWS = ("trace_gain", "trace_pos")
LDS_K = 13  # kTableLdsK: the largest table one workgroup builds in LDS


def pooled_lists(n, seed, K_of, draws_of, max_parents=4, rooted=(), grid=0.25):
    """Lists with bounded candidate pools: variable v draws its sets from the K_of(v) highest variables
    other than v (above bit 31 for n > 33), every one of them also as a single parent, so K_v = K_of(v);
    the empty set unless v is in `rooted`; scores on a coarse grid, so that values tie."""
    rng = np.random.default_rng(seed)
    offsets, sets, scores = [0], [], []
    for v in range(n):
        pool = [u for u in range(n - 1, -1, -1) if u != v][:K_of(v)]
        mine = {1 << u for u in pool} | (set() if v in rooted else {0})
        for _ in range(draws_of(v) if pool else 0):
            k = int(rng.integers(1, min(max_parents, len(pool)) + 1))
            mine.add(sum(1 << int(u) for u in rng.choice(pool, size=k, replace=False)))
        mine = sorted(mine)
        rng.shuffle(mine)
        sets += mine
        scores += list(-np.round(rng.uniform(1, 40, len(mine)) / grid) * grid)
        offsets.append(len(sets))
    return om.Lists(n, offsets, np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))


READBACK_K = {0: 0, 1: 1, 2: 6, 3: 7, 4: LDS_K, 5: LDS_K + 1, 6: 17, 7: 3}  # by variable; 7 has no empty set; the rest 2


@functools.lru_cache(maxsize=None)
def readback_lists():
    return pooled_lists(63, 3, lambda v: READBACK_K.get(v, 2), lambda v: 60, rooted=(7,), grid=2.0)


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> (Lists, seed, tenure, patience): n5 and n8 of the list path's suite; n33 with tenure 0; n63 with K on
    both sides of the LDS limit and one list of 5,000 draws on a coarse grid."""
    big = {40: LDS_K + 2, 41: LDS_K, 42: LDS_K + 1}
    d = {k: osr.inputs()[k] for k in ("n5", "n8")}
    d["n33"] = (pooled_lists(33, 31, lambda v: 5, lambda v: 40, max_parents=3), 7, 0, 20)
    d["n63"] = (pooled_lists(63, 41, lambda v: big.get(v, 4), lambda v: 5000 if v == 40 else 30, max_parents=6, grid=1.0), 9, 31, 25)
    return d


@functools.lru_cache(maxsize=None)
def reference(name):
    L, seed, tenure, patience = inputs()[name]
    return osr.run([osr.Search(L, seed, c, tenure, patience) for c in range(4)], STEPS)


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _begin(ctx, name, searches, tables=True):
    L, seed, tenure, patience = inputs()[name]
    ctx.order_search_begin(*L.triple(), searches, seed=seed, tenure=tenure, patience=patience, tables=tables)
    return L


def _bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _key(b, i):
    """os_entry_key of osr.best's (value, index): the float32's order-preserving image above 2^32 - 1 - index."""
    if i < 0:
        return 0
    bits = int(np.float32(b).view(np.uint32))
    image = (~bits & 0xFFFFFFFF) if bits >> 31 else bits | 0x80000000
    return (image << 32) | (0xFFFFFFFF - i)


def _status(call, *a, **kw):
    with pytest.raises(ulg.ULGError) as e:
        call(*a, **kw)
    return int(re.search(r"status (\d+)", str(e.value)).group(1)), str(e.value)


@pytest.mark.parametrize("v", sorted(READBACK_K), ids=lambda v: f"K{READBACK_K[v]}")
def test_table_equals_the_best_of_every_subset(ctx, v):
    L = readback_lists()
    ctx.order_search_begin(*L.triple(), 1, init_order=np.arange(62, -1, -1, dtype=np.uint8)[None], tables=True)
    C, keys = ctx.order_search_table(v)
    members = [u for u in range(63) if (C >> u) & 1]
    assert C == int(np.bitwise_or.reduce(L.sets[v])) and len(members) == READBACK_K[v] and len(keys) == 1 << len(members)
    assert all(u > 31 for u in members) and (keys[0] == 0) == (v == 7)
    want = [_key(*osr.best(L, v, sum(1 << u for r, u in enumerate(members) if (x >> r) & 1))) for x in range(len(keys))]
    assert np.array_equal(keys, np.array(want, dtype=np.uint64))
    assert READBACK_K[v] < 6 or len(set(L.sc[v])) < len(L.sc[v])  # 20 values for more sets: ties, the least index decided


@pytest.mark.parametrize("name", ["n5", "n8", "n33", "n63"])
def test_searches_over_tables_equal_the_restatement_and_the_lists(ctx, name):
    L, ref = _begin(ctx, name, 4), reference(name)
    r = ctx.order_search_run(STEPS, trace=True)
    state = ctx.order_search_state()
    for k in KEYS:
        assert np.array_equal(r[k], ref[k]), k
    assert state[3] == STEPS and np.array_equal(state[0], ref["order"]) and np.array_equal(state[1], ref["terms"])
    assert _bits(r["best_score"], ref["best_score"]) and _bits(state[2], ref["score"])
    best = [ctx.order_best(o) for o in (state[0], r["best_order"])]
    assert _bits(best[0][0], state[1]) and np.array_equal(best[1][1], r["best_parents"])
    _begin(ctx, name, 4, tables=False)
    lists = ctx.order_search_run(STEPS, trace=True)
    assert all(_bits(r[k], lists[k]) for k in KEYS)
    assert all(_bits(x, y) for x, y in zip(ctx.order_search_state(), state))
    for (terms, parents), o in zip(best, (state[0], r["best_order"])):  # ulg_order_best with tables against without
        assert all(_bits(x, y) for x, y in zip(ctx.order_best(o), (terms, parents)))


def test_invariance(ctx):
    _begin(ctx, "n33", 64)
    whole = ctx.order_search_run(STEPS, trace=True)
    state = ctx.order_search_state()
    assert all(np.array_equal(whole[k][:, :4] if k in ROWS else whole[k][:4], reference("n33")[k]) for k in KEYS)
    _begin(ctx, "n33", 64)
    a, b = ctx.order_search_run(40, trace=True), ctx.order_search_run(110, trace=True)
    for k in KEYS:
        assert _bits(np.concatenate([a[k], b[k]]) if k in ROWS else b[k], whole[k]), k
    assert all(_bits(x, y) for x, y in zip(ctx.order_search_state(), state))
    _begin(ctx, "n33", 1)
    one = ctx.order_search_run(STEPS, trace=True)
    for k in KEYS:
        assert _bits(one[k], np.ascontiguousarray(whole[k][:, :1] if k in ROWS else whole[k][:1])), k
    ctx.set_option("mcmc_launch_steps", 7)
    _begin(ctx, "n33", 64)
    r = ctx.order_search_run(STEPS, trace=True)
    ctx.set_option("mcmc_launch_steps", 4096)
    assert all(_bits(r[k], whole[k]) for k in KEYS)


def test_refusals(ctx):
    UNSUPPORTED, STATE = 4, 3
    wide = pooled_lists(30, 1, lambda v: 27 if v == 2 else 1, lambda v: 0)  # variable 2: 27 single-parent sets
    code, text = _status(ctx.order_search_begin, *wide.triple(), 2, tables=True)
    assert code == UNSUPPORTED and "variable 2 " in text and str(8 << 27) in text
    assert _status(ctx.order_search_run, 1)[0] == STATE
    ctx.order_search_begin(*wide.triple(), 2, tables=False)  # the lists themselves are fine
    assert _status(ctx.order_search_table, 2)[0] == STATE
    assert ctx.info("search_tables") == 0
    _begin(ctx, "n5", 4)
    assert len(ctx.order_search_table(0)[1]) >= 1
    _begin(ctx, "n5", 4, tables=False)  # off after on: as ever
    assert _status(ctx.order_search_table, 0)[0] == STATE
    r = ctx.order_search_run(STEPS, trace=True)
    assert all(np.array_equal(r[k], reference("n5")[k]) for k in KEYS)
