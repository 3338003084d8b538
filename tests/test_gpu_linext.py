"""ulg_dag_linear_extensions on the GPU against tests/linext_ref.py.

The count is an integer: ext_lo and ext_hi must EQUAL the reference's words in every case.
log_ext is held to math.log of the Python integer within 2 ulp of the double: logl's 1 ulp of
long double and the conversion's 2^-64 are far below one, the final rounding adds 1/2 ulp, and
math.log's own last-bit error the rest.

The kernel has one form (csrc/linext.hip): a lane per (DAG, node of a layer), workgroups of
256 lanes that belong to one DAG.  Its one boundary is the first n whose widest layer takes
more than one workgroup per DAG: C(10, 5) = 252 <= 256 < 462 = C(11, 5).  n = 10 and 11 are
among the random cases and get the empty graph as well.
"""
import math
import time

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so (tests/test_gpu_posterior.py)

import linext_ref as lx
import posterior_sample_ref as ps
import synth
import ulg
from test_linext_ref import all_assignments

pytestmark = pytest.mark.gpu

STATUS = {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _raw(ctx, n, parents, want_hi=True, want_log=True):
    """The C call itself -> (status, lo, hi, log_ext)."""
    p = np.ascontiguousarray(parents, dtype=np.uint64).reshape(-1, n)
    lo = np.zeros(len(p), dtype=np.uint64)
    hi = np.zeros(len(p), dtype=np.uint64)
    le = np.zeros(len(p), dtype=np.float64)
    rc = ulg.lib().ulg_dag_linear_extensions(ctx._h, n, len(p), ulg._ptr(p), ulg._ptr(lo), ulg._ptr(hi) if want_hi else None,
                                             ulg._ptr(le) if want_log else None)
    return rc, lo, hi, le


def _check(ctx, n, dags, want):
    """Words equal, log_ext within 2 ulp, the Python wrapper's integers the same."""
    rc, lo, hi, le = _raw(ctx, n, dags)
    assert rc == 0
    got = [(int(h) << 64) | int(l) for l, h in zip(lo, hi)]
    assert got == [int(w) for w in want]
    for x, w in zip(le, want):
        if w == 0:
            assert x == -np.inf
        else:
            assert lx.ulp_distance(float(x), math.log(int(w))) <= 2, (w, float(x), math.log(int(w)))
    ext, le2 = ctx.dag_linear_extensions(np.array(dags, dtype=np.uint64).reshape(-1, n))
    assert ext == got and le2.tobytes() == le.tobytes()
    # the optional outputs left out: the low words alone are the same
    rc, lo2, hi2, le3 = _raw(ctx, n, dags, want_hi=False, want_log=False)
    assert rc == 0 and lo2.tobytes() == lo.tobytes() and not hi2.any() and not le3.any()


# ---- 1. small n, exhaustively --------------------------------------------------------------------
def test_n1_and_n2(ctx):
    _check(ctx, 1, [[0]], [1])
    _check(ctx, 2, [[0, 0], [0, 1], [2, 0], [2, 1]], [2, 1, 1, 0])  # empty, 0 -> 1, 1 -> 0, the 2-cycle


def test_every_assignment_of_n4(ctx):
    """All 8^4 assignments of parent masks in one call: 543 DAGs, the rest cyclic (count 0)."""
    pars = all_assignments(4)
    want = lx.count_many(4, pars)
    assert len(pars) == 4096 and int((want > 0).sum()) == 543
    _check(ctx, 4, pars, want)
    for i in (0, 77, 1234, 4095):
        assert int(want[i]) == lx.count(4, [int(x) for x in pars[i]])


# ---- 2. random DAGs --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(5, 13)) + [16])
def test_random_dags(ctx, n):
    rng = np.random.default_rng(500 + n)
    dags = [lx.random_dag(n, d, rng) for d in (0.1, 0.4, 0.8)]
    _check(ctx, n, dags, [lx.count(n, par) for par in dags])


@pytest.mark.parametrize("n", [10, 11])
def test_workgroup_boundary(ctx, n):
    """The widest layer in one workgroup per DAG (n = 10) and in two (n = 11): a random DAG, the empty graph."""
    rng = np.random.default_rng(900 + n)
    dag = lx.random_dag(n, 0.3, rng)
    _check(ctx, n, [dag, [0] * n], [lx.count(n, dag), math.factorial(n)])


# ---- 3. the high word --------------------------------------------------------------------------------
def test_high_word(ctx):
    _check(ctx, 20, [[0] * 20], [math.factorial(20)])
    assert math.factorial(20) < 1 << 63
    _check(ctx, 21, [[0] * 21], [math.factorial(21)])  # the smallest shape whose carry reaches hi
    assert math.factorial(21) >> 64 == 2
    forest = lx.random_forest(24, np.random.default_rng(24), roots=0.5)
    want = lx.hook(24, forest)
    assert want >> 64 > 0  # roots = 0.5 keeps the subtrees small enough
    _check(ctx, 24, [forest], [want])


def test_offsets_past_2_to_32_bytes(ctx):
    """n = 28: a table of exactly 2^32 bytes per DAG, so the last entries lie just below 2^32 bytes and the
    batch's zero cell exactly at 2^32; two DAGs, which the default rule gives a batch each.  The file's
    one slow case; its time is printed.  A card without the memory must refuse with
    ULG_ERR_UNSUPPORTED; n = 27 is checked then."""
    n = 28
    forest = lx.random_forest(n, np.random.default_rng(28), roots=0.5)
    dags, want = [[0] * n, forest], [math.factorial(n), lx.hook(n, forest)]
    t0 = time.perf_counter()
    rc, lo, hi, le = _raw(ctx, n, dags)
    dt = time.perf_counter() - t0
    if rc == STATUS["UNSUPPORTED"]:
        print("n = 28 refused: the table does not fit the free device memory; checking n = 27")
        assert "bytes" in ulg.lib().ulg_last_error(ctx._h).decode()
        n = 27
        forest = lx.random_forest(n, np.random.default_rng(27), roots=0.5)
        dags, want = [[0] * n, forest], [math.factorial(n), lx.hook(n, forest)]
        rc, lo, hi, le = _raw(ctx, n, dags)
    assert rc == 0
    print(f"n = {n}, 2 DAGs: {dt:.2f} s, {ctx.info('linext_batches')} batch(es)")
    assert [(int(h) << 64) | int(l) for l, h in zip(lo, hi)] == want
    assert all(lx.ulp_distance(float(x), math.log(w)) <= 2 for x, w in zip(le, want))


# ---- 4. batching -----------------------------------------------------------------------------------
def test_batching(ctx):
    n = 10
    rng = np.random.default_rng(10)
    dags = [lx.random_dag(n, d, rng) for d in (0.0, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0)]
    want = [lx.count(n, par) for par in dags]
    words = []
    for batch, batches in ((1, 7), (2, 4), (3, 3), (0, 1)):
        ctx.set_option("linext_batch", batch)
        assert ctx.info("linext_batch") == batch
        rc, lo, hi, le = _raw(ctx, n, dags)
        assert rc == 0 and ctx.info("linext_batches") == batches
        assert [(int(h) << 64) | int(l) for l, h in zip(lo, hi)] == want
        words.append(lo.tobytes() + hi.tobytes() + le.tobytes())
    assert len(set(words)) == 1
    assert ulg.lib().ulg_dag_linear_extensions(ctx._h, n, 0, None, None, None, None) == 0  # count = 0: no device work
    assert ctx.info("linext_batches") == 0
    with pytest.raises(ulg.ULGError):
        ctx.set_option("linext_batch", -1)


# ---- 5. a sampler block ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense-6", "wide-12"])
def test_sampler_block(ctx, name):
    n, offs, sets, scores, K, seed = ps.gpu_inputs()[name]
    ctx.posterior(offs, sets, scores)
    parents, _, _ = ctx.posterior_sample(K, seed)
    uniq, inv = np.unique(parents, axis=0, return_inverse=True)
    want = [int(x) for x in lx.count_many(n, uniq)[np.asarray(inv).reshape(-1)]]
    ext, le = ctx.dag_linear_extensions(parents)
    raw, le_raw = ctx.dag_linear_extensions(parents, dedupe=False)
    assert ext == want and min(ext) >= 1  # the sampled order is an extension
    assert raw == ext and le_raw.tobytes() == le.tobytes()
    assert int(want[0]) == lx.count(n, [int(x) for x in parents[0]])
    print(f"{name}: {len(uniq)} distinct of {K}")
    # the weights: the function equals its numpy restatement to the bit
    edge, ess = ulg.uniform_prior_edges(parents, le)
    r = np.exp(le.min() - le)
    tot = np.cumsum(r)[-1]
    for v in range(n):
        for u in range(n):
            has = ((parents[:, v] >> np.uint64(u)) & np.uint64(1)) == 1
            assert edge[u, v] == np.cumsum(np.where(has, r, 0.0))[-1] / tot
    assert ess == tot * tot / np.cumsum(r * r)[-1] and 1.0 <= ess <= K


# ---- 6. errors -------------------------------------------------------------------------------------
def test_errors_write_nothing(ctx):
    L = ulg.lib()
    n = 5
    good = np.array([[0, 1, 3, 0, 8]], dtype=np.uint64)
    pattern = np.uint64(0xA5A5A5A5A5A5A5A5)

    def call(n_, count, parents, null_lo=False, null_par=False):
        lo = np.full(4, pattern, dtype=np.uint64)
        hi = np.full(4, pattern, dtype=np.uint64)
        le = np.full(4, 123.25, dtype=np.float64)
        p = np.ascontiguousarray(parents, dtype=np.uint64)
        rc = L.ulg_dag_linear_extensions(ctx._h, n_, count, None if null_par else ulg._ptr(p), None if null_lo else ulg._ptr(lo),
                                         ulg._ptr(hi), ulg._ptr(le))
        assert np.all(lo == pattern) and np.all(hi == pattern) and np.all(le == 123.25), "an output was written"
        return rc

    own = good.copy()
    own[0, 2] |= np.uint64(1 << 2)
    high = good.copy()
    high[0, 1] |= np.uint64(1 << 5)
    far = good.copy()
    far[0, 4] |= np.uint64(1 << 63)
    two = np.concatenate([good, own])  # the second DAG is the bad one: the first is not written either
    assert call(n, 1, own) == STATUS["ARG"] and "own bit" in L.ulg_last_error(ctx._h).decode()
    assert call(n, 1, high) == STATUS["ARG"] and "bit >= n" in L.ulg_last_error(ctx._h).decode()
    assert call(n, 1, far) == STATUS["ARG"]
    assert call(n, 2, two) == STATUS["ARG"]
    assert call(0, 1, good) == STATUS["ARG"]
    assert call(-3, 1, good) == STATUS["ARG"]
    assert call(n, -1, good) == STATUS["ARG"]
    assert call(n, 1, good, null_lo=True) == STATUS["ARG"]
    assert call(n, 1, good, null_par=True) == STATUS["ARG"]
    live = ctx.info("device_bytes_live")
    assert call(29, 1, np.zeros((1, 29), dtype=np.uint64)) == STATUS["UNSUPPORTED"]
    assert call(64, 1, np.zeros((1, 64), dtype=np.uint64)) == STATUS["UNSUPPORTED"]
    assert ctx.info("device_bytes_live") == live
    assert L.ulg_dag_linear_extensions(None, n, 1, ulg._ptr(good), None, None, None) == STATUS["ARG"]
    assert L.ulg_dag_linear_extensions(ctx._h, n, 0, None, None, None, None) == 0
    with pytest.raises(ulg.ULGError):
        ctx.dag_linear_extensions(own)
    # the call's buffers are its own: nothing stays allocated after a success either
    _check(ctx, n, good, [lx.count(n, [int(x) for x in good[0]])])
    assert ctx.info("device_bytes_live") == live


# ---- 7. the call changes nothing else ------------------------------------------------------------
def _same(a, b):
    return all((x is None and y is None) or np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def test_the_context_is_left_as_it_was(ctx):
    n, N = 6, 200
    X, _ = synth.gaussian_sem(n, N, 4242)
    ctx.load(X, 2.0)
    stored, _ = ctx.score_bge(list(range(n)), [(1 << n) - 1] * n, n - 1)
    lists = ctx.fetch(stored)
    ctx.posterior_from_scores()
    tables = [ctx.posterior_table(w, 0).tobytes() for w in (0, 1, 2)]
    a = ctx.posterior_sample(500, seed=3)
    ext, _ = ctx.dag_linear_extensions(a[0])
    rng = np.random.default_rng(77)
    ctx.dag_linear_extensions(np.array([lx.random_dag(9, 0.3, rng)], dtype=np.uint64))  # another n altogether
    assert min(ext) >= 1
    assert _same(lists, ctx.fetch(stored))
    assert tables == [ctx.posterior_table(w, 0).tobytes() for w in (0, 1, 2)]
    assert _same(a, ctx.posterior_sample(500, seed=3))


def test_two_contexts_and_two_calls_agree(ctx):
    n = 12
    rng = np.random.default_rng(1212)
    dags = np.array([lx.random_dag(n, d, rng) for d in (0.05, 0.2, 0.5, 0.9)], dtype=np.uint64)
    a = _raw(ctx, n, dags)
    b = _raw(ctx, n, dags)
    other = ulg.Context(0)  # a fresh context: the call needs no loaded data, lists or posterior state
    try:
        c = _raw(other, n, dags)
    finally:
        other.close()
    assert a[0] == 0 and _same(a[1:], b[1:]) and _same(a[1:], c[1:])
    assert [(int(h) << 64) | int(l) for l, h in zip(a[1], a[2])] == [int(x) for x in lx.count_many(n, dags)]
