"""ulg_dag_features on the GPU against tests/dagfeat_ref.py.

Every output is an integer sum: every comparison here is equality.  Weights are seeded random
integers below 2^40 (sums stay below 2^55), so that a fault in one DAG cannot cancel against
another's.

The kernel (csrc/dagfeat.hip) has one form per DAG, a wave64 with lane v holding row v, and two
forms of accumulation: the four n x n tables in LDS up to n = 45 (kDagfeatLdsMaxVars), global
atomics from n = 46 on.  The random sizes stand on both sides (45, 46) besides the sizes where a
32-bit row or a 28-variable limit would end (27 .. 33) and the ends (1, 2, 62, 63).
"""
import math

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so (tests/test_gpu_posterior.py)

import dagfeat_ref as df
import posterior_sample_ref as ps
import synth
import ulg

pytestmark = pytest.mark.gpu

STATUS = {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}
NAMES = ulg.DAG_FEATURES
SIZES = (1, 2, 27, 28, 29, 31, 32, 33, 45, 46, 62, 63)


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _weights(count, seed):
    return np.random.default_rng(seed).integers(0, 1 << 40, size=count, dtype=np.uint64)


def _equal(got, want, names=NAMES):
    assert got["total"] == want["total"] and got["cyclic"] == want["cyclic"], (got["total"], want["total"], got["cyclic"])
    for name in names:
        assert got[name].dtype == np.uint64 and got[name].shape == want[name].shape
        bad = np.argwhere(got[name] != want[name])
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist(), [int(got[name][tuple(i)]) for i in bad[:5]],
                               [int(want[name][tuple(i)]) for i in bad[:5]])


def _same(a, b):
    return a["total"] == b["total"] and a["cyclic"] == b["cyclic"] and all(a[k].tobytes() == b[k].tobytes() for k in NAMES)


def _arr(dags, n):
    return np.array(dags, dtype=np.uint64).reshape(-1, n)


# ---- 1. every DAG of n = 4 and n = 5 -------------------------------------------------------------
_ALL = {}


def _all(n, weighted):
    if (n, weighted) not in _ALL:
        dags = df.all_dags(n)
        w = _weights(len(dags), 40 + n) if weighted else None
        _ALL[(n, weighted)] = (_arr(dags, n), w, df.features(n, dags, w))
    return _ALL[(n, weighted)]


@pytest.mark.parametrize("n,count,weighted", [(4, 543, True), (4, 543, False), (5, 29281, True)])
def test_every_dag_in_one_call(ctx, n, count, weighted):
    dags, w, want = _all(n, weighted)
    assert len(dags) == count
    got = ctx.dag_features(dags, w)
    _equal(got, want)
    assert want["cyclic"] == 0 and want["total"] == (sum(int(x) for x in w) if weighted else count)
    assert want["total"] < 1 << 55


# ---- 2. random DAGs ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("n", SIZES)
def test_random_dags(ctx, n, kind):
    rng = np.random.default_rng(1000 * n + len(kind))
    dags = [df.random_dag(n, kind, rng) for _ in range(200)]
    w = _weights(200, n)
    _equal(ctx.dag_features(_arr(dags, n), w), df.features(n, dags, w))


# ---- 3. the structured graphs at n = 63 ----------------------------------------------------------
def test_structured_graphs(ctx):
    n = 63
    got = {name: ctx.dag_features(_arr([getattr(df, name)(n)], n)) for name in ("chain", "collider_chain", "complete", "star")}
    got["empty"] = ctx.dag_features(np.zeros((1, n), dtype=np.uint64))
    batch = [df.chain(n), df.collider_chain(n), df.complete(n), df.star(n), [0] * n]
    w = _weights(5, 63)
    _equal(ctx.dag_features(_arr(batch, n), w), df.features(n, batch, w))
    for name in ("chain", "collider_chain", "complete", "star"):
        _equal(got[name], df.features(n, [getattr(df, name)(n)]))
    tri = np.triu(np.ones((n, n), dtype=np.uint64), 1)
    assert np.array_equal(got["chain"]["ancestor"], tri) and int(got["chain"]["compelled"].sum()) == 0
    assert int(got["chain"]["edge"].sum()) == 62 and int(got["chain"]["vstruct"].sum()) == 0
    assert np.array_equal(got["collider_chain"]["compelled"], got["collider_chain"]["edge"])  # 60 R1 steps
    assert int(got["collider_chain"]["compelled"].sum()) == 62 and int(got["collider_chain"]["vstruct"].sum()) == 1
    assert np.array_equal(got["complete"]["edge"], tri) and int(got["complete"]["compelled"].sum()) == 0
    assert np.array_equal(got["complete"]["blanket"], tri + tri.T)
    assert np.array_equal(got["star"]["compelled"], got["star"]["edge"]) and int(got["star"]["edge"].sum()) == 62
    assert int(got["star"]["vstruct"].sum()) == math.comb(62, 2) and int(got["star"]["vstruct"][62].sum()) == math.comb(62, 2)
    assert np.array_equal(got["star"]["blanket"], (tri + tri.T))  # every parent a co-parent of every other
    assert got["empty"]["total"] == 1 and all(int(got["empty"][k].sum()) == 0 for k in NAMES)


# ---- 4. cyclic inputs ----------------------------------------------------------------------------
def test_cycles_are_counted_and_add_nothing(ctx):
    two = ctx.dag_features(_arr([df.cycle(2)], 2))
    assert two["cyclic"] == 1 and two["total"] == 0 and all(int(two[k].sum()) == 0 for k in NAMES)
    n = 63
    ring = ctx.dag_features(_arr([df.cycle(n)], n), np.array([7], dtype=np.uint64))
    assert ring["cyclic"] == 1 and ring["total"] == 0 and all(int(ring[k].sum()) == 0 for k in NAMES)
    rng = np.random.default_rng(63)
    small = [0] * n
    small[0], small[1] = 2, 1  # a 2-cycle among 61 isolated variables
    late = df.chain(n)
    late[0] = 1 << 62  # the chain closed into a ring by its last edge
    dags = [df.random_dag(n, "sparse", rng), df.cycle(n), df.collider_chain(n), small, df.random_dag(n, "dense", rng), late,
            df.star(n)]
    w = _weights(len(dags), 64)
    want = df.features(n, dags, w)
    assert want["cyclic"] == 3
    got = ctx.dag_features(_arr(dags, n), w)
    _equal(got, want)
    keep = [0, 2, 4, 6]
    alone = df.features(n, [dags[i] for i in keep], w[keep])
    assert alone["cyclic"] == 0
    alone["cyclic"] = 3
    _equal(got, alone)  # every table is that of the DAGs alone
    # the number, not the weight; and without weights
    plain = ctx.dag_features(_arr(dags, n))
    assert plain["cyclic"] == 3 and plain["total"] == 4


# ---- 5. geometry ---------------------------------------------------------------------------------
def test_grid_and_batching_do_not_change_a_bit(ctx):
    n, count = 12, 5000
    rng = np.random.default_rng(12)
    dags = [df.random_dag(n, "sparse" if k % 2 else "dense", rng) for k in range(count)]
    arr, w = _arr(dags, n), _weights(count, 5000)
    runs = {}
    for grid, launched in ((1, 1), (7, 7), (0, 1250)):  # 4, 28 and 5,000 waves for 5,000 DAGs
        ctx.set_option("dagfeat_grid", grid)
        runs[grid] = ctx.dag_features(arr, w)
        assert ctx.info("dagfeat_grid") == launched
    assert _same(runs[1], runs[7]) and _same(runs[1], runs[0])
    _equal(runs[0], df.features(n, dags, w))
    a, b = ctx.dag_features(arr[:2500], w[:2500]), ctx.dag_features(arr[2500:], w[2500:])
    assert a["total"] + b["total"] == runs[0]["total"] and a["cyclic"] + b["cyclic"] == 0
    assert all(np.array_equal(a[k] + b[k], runs[0][k]) for k in NAMES)
    # the same past the LDS tables: global atomics at n = 46
    n = 46
    dags = [df.random_dag(n, "sparse", rng) for _ in range(300)]
    arr, w = _arr(dags, n), _weights(300, 46)
    ctx.set_option("dagfeat_grid", 3)
    few = ctx.dag_features(arr, w)
    ctx.set_option("dagfeat_grid", 0)
    assert _same(few, ctx.dag_features(arr, w)) and ctx.info("dagfeat_grid") == 75
    with pytest.raises(ulg.ULGError):
        ctx.set_option("dagfeat_grid", -1)
    with pytest.raises(ulg.ULGError):
        ctx.set_option("dagfeat_grid", 65537)


# ---- 6. NULL outputs, count = 0 ------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 63])
def test_every_table_alone_and_none(ctx, n):
    rng = np.random.default_rng(600 + n)
    dags = [df.random_dag(n, "sparse" if k % 3 else "dense", rng) for k in range(40)] + [df.cycle(n)]
    arr, w = _arr(dags, n), _weights(len(dags), 6)
    want = df.features(n, dags, w)
    for name in NAMES:
        got = ctx.dag_features(arr, w, want=(name,))
        assert sorted(got) == sorted([name, "total", "cyclic"])
        _equal(got, want, names=(name,))
    got = ctx.dag_features(arr, w, want=())
    assert got == {"total": want["total"], "cyclic": 1}
    total = np.zeros(1, dtype=np.uint64)  # cyclic may be NULL as well
    rc = ulg.lib().ulg_dag_features(ctx._h, n, len(arr), ulg._ptr(arr), ulg._ptr(w), None, None, None, None, None,
                                    total.ctypes.data_as(ulg.C.POINTER(ulg.C.c_uint64)), None)
    assert rc == 0 and int(total[0]) == want["total"]


def _raw(ctx, n, count, parents, weight=None, null_total=False, fill=0xA5A5A5A5A5A5A5A5, size=5):
    """The C call on outputs filled with a pattern -> (status, the outputs, total, cyclic)."""
    outs = [np.full(size ** 2, fill, dtype=np.uint64) for _ in range(4)] + [np.full(size ** 3, fill, dtype=np.uint64)]
    total, cyclic = ulg.C.c_uint64(12345), ulg.C.c_int64(-7)
    rc = ulg.lib().ulg_dag_features(ctx._h, n, count, None if parents is None else ulg._ptr(parents),
                                    None if weight is None else ulg._ptr(weight), *[ulg._ptr(o) for o in outs],
                                    None if null_total else ulg.C.byref(total), ulg.C.byref(cyclic))
    return rc, outs, total.value, cyclic.value


def test_count_zero_zero_fills(ctx):
    live = ctx.info("device_bytes_live")
    rc, outs, total, cyclic = _raw(ctx, 5, 0, None)
    assert rc == 0 and total == 0 and cyclic == 0 and all(not o.any() for o in outs)
    assert ctx.info("dagfeat_grid") == 0 and ctx.info("device_bytes_live") == live
    assert ulg.lib().ulg_dag_features(ctx._h, 5, 0, None, None, None, None, None, None, None, ulg.C.byref(ulg.C.c_uint64(1)), None) == 0
    got = ctx.dag_features(np.zeros((0, 5), dtype=np.uint64))
    assert got["total"] == 0 and got["cyclic"] == 0 and got["vstruct"].shape == (5, 5, 5) and not got["edge"].any()


# ---- 7. errors -----------------------------------------------------------------------------------
def test_errors_write_nothing(ctx):
    L = ulg.lib()
    n = 5
    good = np.array([[0, 1, 3, 0, 8]], dtype=np.uint64)
    fill = 0xA5A5A5A5A5A5A5A5

    def refused(status, n_, count, parents, **kw):
        rc, outs, total, cyclic = _raw(ctx, n_, count, parents, **kw)
        assert all(np.all(o == np.uint64(fill)) for o in outs) and total == 12345 and cyclic == -7, "an output was written"
        return rc == STATUS[status]

    own, high, far = good.copy(), good.copy(), good.copy()
    own[0, 2] |= np.uint64(1 << 2)
    high[0, 1] |= np.uint64(1 << 5)
    far[0, 4] |= np.uint64(1 << 63)
    two = np.concatenate([good, own])  # the second DAG is the bad one: the first adds nothing either
    live = ctx.info("device_bytes_live")
    assert refused("ARG", n, 1, own) and "own bit" in L.ulg_last_error(ctx._h).decode()
    assert refused("ARG", n, 1, high) and "bit >= n" in L.ulg_last_error(ctx._h).decode()
    assert refused("ARG", n, 1, far) and refused("ARG", n, 2, two)
    assert refused("ARG", 0, 1, good) and refused("ARG", -3, 1, good) and refused("ARG", n, -1, good)
    assert refused("ARG", n, 1, None) and refused("ARG", n, 1, good, null_total=True) and refused("ARG", n, 0, None, null_total=True)
    assert refused("UNSUPPORTED", 64, 1, np.zeros((1, 64), dtype=np.uint64))
    assert refused("UNSUPPORTED", 100, 0, None)
    # the weights: a sum of exactly 2^63 is refused, also one that wraps 64 bits; 2^63 - 1 is taken
    pair = np.concatenate([good, good])
    at = np.array([1 << 62, 1 << 62], dtype=np.uint64)
    assert refused("ARG", n, 2, pair, weight=at) and "2^63" in L.ulg_last_error(ctx._h).decode()
    assert refused("ARG", n, 2, pair, weight=np.array([1 << 63, 1 << 63], dtype=np.uint64))
    assert refused("ARG", n, 1, good, weight=np.array([1 << 63], dtype=np.uint64))
    assert refused("ARG", n, 2, pair, weight=np.array([(1 << 64) - 1, 1], dtype=np.uint64))
    assert ctx.info("device_bytes_live") == live
    assert L.ulg_dag_features(None, n, 1, ulg._ptr(good), None, None, None, None, None, None, ulg.C.byref(ulg.C.c_uint64(0)), None) \
        == STATUS["ARG"]
    below = np.array([1 << 62, (1 << 62) - 1], dtype=np.uint64)
    got = ctx.dag_features(pair, below)
    _equal(got, df.features(n, [[int(x) for x in good[0]]] * 2, below))
    assert got["total"] == (1 << 63) - 1 and int(got["edge"][0, 1]) == (1 << 63) - 1
    with pytest.raises(ulg.ULGError):
        ctx.dag_features(own)
    with pytest.raises(ulg.ULGError):
        ctx.dag_features(good, want=("edges",))
    with pytest.raises(ulg.ULGError):
        ctx.dag_features(good, weight=np.ones(2, dtype=np.uint64))
    # n = 63 is taken where 64 is not, and the call's buffers are its own
    assert ctx.dag_features(np.zeros((1, 63), dtype=np.uint64))["total"] == 1
    assert ctx.info("device_bytes_live") == live


# ---- 8. the call changes nothing else; samples of the sampler --------------------------------------
def test_the_context_is_left_as_it_was(ctx):
    n, N = 6, 200
    X, _ = synth.gaussian_sem(n, N, 4242)
    ctx.load(X, 2.0)
    stored, _ = ctx.score_bge(list(range(n)), [(1 << n) - 1] * n, n - 1)
    lists = ctx.fetch(stored)
    ctx.posterior_from_scores()
    tables = [ctx.posterior_table(w, 0).tobytes() for w in (0, 1, 2)]
    a = ctx.posterior_sample(500, seed=3)
    got = ctx.dag_features(a[0])
    rng = np.random.default_rng(77)
    ctx.dag_features(_arr([df.random_dag(50, "sparse", rng)], 50))  # another n altogether
    _equal(got, df.features(n, a[0]))
    assert got["total"] == 500 and got["cyclic"] == 0  # a sampled graph has an order
    same = lambda x, y: all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x, y))  # noqa: E731
    assert same(lists, ctx.fetch(stored))
    assert tables == [ctx.posterior_table(w, 0).tobytes() for w in (0, 1, 2)]
    assert same(a, ctx.posterior_sample(500, seed=3))


def test_sampler_block_with_uniform_prior_weights(ctx):
    n, offs, sets, scores, K, seed = ps.gpu_inputs()["wide-12"]
    ctx.posterior(offs, sets, scores)
    parents, _, _ = ctx.posterior_sample(K, seed)
    _, le = ctx.dag_linear_extensions(parents)
    w = ulg.uniform_prior_weights(le)
    assert int(w.max()) == 1 << 52 and sum(int(x) for x in w) < 1 << 63
    got = ctx.dag_features(parents, w)
    _equal(got, df.features(n, parents, w))
    other = ulg.Context(0)  # a fresh context: the call needs no loaded data, lists or posterior state
    try:
        assert _same(got, other.dag_features(parents, w))
    finally:
        other.close()
