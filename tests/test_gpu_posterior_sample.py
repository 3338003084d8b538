"""The posterior sampler on the GPU (ulg_posterior_sample, ulg_posterior_sample_u)
against tests/posterior_sample_ref.py, the contract in Python integers.

The reference is fed the device's own ln alpha and ln f, read back with
ulg_posterior_table, so every log-probability x it forms is the kernel's to the
bit; what may differ is exp alone, and the reference marks every step whose
margin is below what exp's rounding can move (its docstring).  No input here has
such a step (tests/test_posterior_sample_ref.py asserts it for the host's
tables, and each comparison asserts it again for the device's), so parents,
order and the bits of log_weight must EQUAL the reference's everywhere.

The n = 20 case has no reference: what a sample is (a permutation; stored sets
that precede their child; the stated sum) and edge frequencies within 6
binomial standard deviations of the call's own edge posteriors.
"""
import ctypes
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so (tests/test_gpu_posterior.py)

import posterior_ref as pr
import posterior_sample_ref as ps
import synth
import ulg

pytestmark = pytest.mark.gpu

STATUS = {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}
U_MAX = (1 << 64) - 1


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _tables(ctx, n):
    return np.stack([ctx.posterior_table(0, v) for v in range(n)]), ctx.posterior_table(1)


def _same(a, b):
    return all((x is None and y is None) or np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _equals_reference(name, got, ref):
    assert ref["undecided"] == 0, (name, "the reference has an undecided step on the device's tables")
    parents, order, weight = got
    assert parents.dtype == np.uint64 and order.dtype == np.uint8 and weight.dtype == np.float64
    bad = np.flatnonzero((parents != ref["parents"]).any(axis=1) | (order != ref["order"]).any(axis=1))
    assert bad.size == 0, (name, "samples differ", bad[:8])
    assert weight.tobytes() == ref["log_weight"].tobytes(), (name, "log_weight bits differ")


# ---- 1. equality with the reference -----------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.gpu_inputs()))
def test_equals_the_reference(ctx, name):
    """n = 1, 2, 6, 7: the four list kinds and the dynamic-range lists, K = 257 (no multiple of the 4 waves
    of a workgroup).  n = 12, 562 entries per list (two passes over 9 chunks), one list cut to 1, 64
    (the single pass) and 65 entries (the first two-pass list); n = 16, K = 64."""
    n, offs, sets, scores, K, seed = ps.gpu_inputs()[name]
    lz, _, _ = ctx.posterior(offs, sets, scores)
    assert np.isfinite(lz)
    alpha, f = _tables(ctx, n)
    ref = ps.sample(n, offs, sets, scores, alpha, f, ps.draws(seed, 0, K, n))
    got = ctx.posterior_sample(K, seed)
    assert got[0].shape == (K, n) and got[1].shape == (K, n) and got[2].shape == (K,)
    _equals_reference(name, got, ref)
    if name.startswith("cut"):
        keep = int(name[3:name.index("-")])
        assert offs[ps.CUT_VAR + 1] - offs[ps.CUT_VAR] == keep
    # the outputs not asked for are not written
    p2, o2, w2 = ctx.posterior_sample(K, seed, want_order=False, want_weight=False)
    assert o2 is None and w2 is None and p2.tobytes() == got[0].tobytes()


# ---- 2. boundary draws ------------------------------------------------------------------------
def _boundary_lists():
    """n = 6.  Variables 1 .. 4 take positive weight only with both 0 and 5 among their parents and at
    most one more; 0 and 5 only with the empty set or each other.  Every other set lies 100 nats below:
    against a compatible set of ordinary weight its q is exactly 0, and nothing has 0 < q < slack.
      sink steps  while a middle variable is in S, the candidates 0 (first) and 5 (last) have q = 0:
                  without them the middle variables of S \\ v lack a parent (f(S \\ v) is e^-100 down);
      set steps   a middle variable's first compatible entry, the empty set, has q = 0, and so has its
                  last one, S \\ v itself, while that has 4 or 5 members (the first two steps)."""
    n, low = 6, -100.0
    offs, sets, scores = pr.make_lists(n, "dense", 1)
    scores = np.full(len(sets), low, dtype=np.float32)
    ends = (1 << 0) | (1 << 5)
    for v in range(n):
        for i in range(offs[v], offs[v + 1]):
            S = int(sets[i])
            if v in (0, 5):
                if S == 0:
                    scores[i] = 0.0 if v == 0 else 0.25
                elif S == ends & ~(1 << v):
                    scores[i] = 0.5 if v == 0 else 0.75
            elif S & ends == ends and bin(S).count("1") <= 3:
                scores[i] = 0.125 * (i - offs[v]) / 32
    return n, offs, sets, scores


def test_boundary_draws(ctx):
    """U = 0 takes the first candidate of positive q, U = 2^64 - 1 the last; a candidate of q = 0 at either
    end of the candidates is never chosen."""
    n, offs, sets, scores = _boundary_lists()
    lz, _, _ = ctx.posterior(offs, sets, scores)
    assert np.isfinite(lz)
    alpha, f = _tables(ctx, n)
    u = np.zeros((4, n, 2), dtype=np.uint64)
    u[1] = U_MAX
    u[2, :, 0] = U_MAX  # the last sink, the first set
    u[3, :, 1] = U_MAX  # the first sink, the last set
    parents, order, weight = got = ctx.posterior_sample_u(u)
    # by hand (docstring of _boundary_lists; the lists are in make_lists' order: by size, then lexicographic)
    both = 0b100001
    assert list(order[0]) == [5, 0, 4, 3, 2, 1] and list(parents[0]) == [0, both, both, both, both, 0]
    assert list(order[1]) == [0, 5, 1, 2, 3, 4]
    assert list(parents[1]) == [0, both, both | 0b10, both | 0b100, both | 0b1000, 0b1]
    assert list(order[2]) == [0, 5, 1, 2, 3, 4] and list(parents[2]) == [0, both, both, both, both, 0]
    assert list(order[3]) == [5, 0, 4, 3, 2, 1]
    assert list(parents[3]) == [0b100000, both | 0b10000, both | 0b10000, both | 0b10000, both, 0]
    # ... and by the reference's integers: the same choices, zero-weight candidates at both ends of the steps
    ref = ps.sample(n, offs, sets, scores, alpha, f, u)
    assert _same(got, (ref["parents"], ref["order"], ref["log_weight"]))
    S = (1 << n) - 1
    for i in range(n - 1, 1, -1):  # the steps of sample 0 that choose a middle variable
        v = int(order[0, i])
        x = np.array([(f[S ^ (1 << c)] + alpha[c, int(pr.squeeze(S ^ (1 << c), c))]) - f[S] for c in range(n) if (S >> c) & 1])
        q, m = ps.weight_q(x)
        assert q[0] == 0 and q[-1] == 0 and np.all((q == 0) | (q >= 8 * (m + 1)))
        S ^= 1 << v
        lo, hi = offs[v], offs[v + 1]
        idx = lo + np.flatnonzero((sets[lo:hi].astype(np.int64) & ~S) == 0)
        q, m = ps.weight_q(scores[idx].astype(np.float64) - alpha[v, int(pr.squeeze(S, v))])
        assert q[0] == 0 and np.all((q == 0) | (q >= 8 * (m + 1)))
        assert (q[-1] == 0) == (bin(S).count("1") >= 4)
    assert weight[0] == sum(float(scores[offs[v]:offs[v + 1]][list(sets[offs[v]:offs[v + 1]]).index(parents[0, v])]) for v in range(n))


# ---- 3. the draws, ranges, determinism ----------------------------------------------------------
def test_given_draws_equal_the_seeded_call(ctx):
    n, offs, sets, scores, K, seed = ps.gpu_inputs()["sparse-7"]
    ctx.posterior(offs, sets, scores)
    first = (1 << 32) - 100  # the sample index crosses 2^32
    a = ctx.posterior_sample(K, seed, first=first)
    b = ctx.posterior_sample_u(ps.draws(seed, first, K, n))
    assert _same(a, b)
    assert not _same(a, ctx.posterior_sample(K, seed + 1, first=first))
    assert not _same(a, ctx.posterior_sample(K, seed, first=first + 1))


def test_a_range_split_over_calls(ctx):
    n, offs, sets, scores, _, seed = ps.gpu_inputs()["dense-7"]
    ctx.posterior(offs, sets, scores)
    whole = ctx.posterior_sample(1000, seed)
    parts = [ctx.posterior_sample(c, seed, first=f) for f, c in ((0, 1), (1, 499), (500, 500))]
    for j in range(3):
        assert whole[j].tobytes() == np.concatenate([p[j] for p in parts]).tobytes()
    empty = ctx.posterior_sample(0, seed)
    assert empty[0].shape == (0, n) and empty[1].shape == (0, n) and empty[2].shape == (0,)


def test_bit_identical_across_calls_contexts_and_table_layouts(ctx):
    n, offs, sets, scores, K, seed = ps.gpu_inputs()["wide-12"]
    ctx.posterior(offs, sets, scores)
    a = ctx.posterior_sample(K, seed)
    assert _same(a, ctx.posterior_sample(K, seed))
    other = ulg.Context(0)
    try:
        other.set_option("posterior_keep", 1)
        other.posterior(offs, sets, scores)
        assert _same(a, other.posterior_sample(K, seed))
    finally:
        other.close()
    ctx.set_option("posterior_keep", 1)
    ctx.posterior(offs, sets, scores)
    assert _same(a, ctx.posterior_sample(K, seed))


# ---- 4. a large case: what a sample is ------------------------------------------------------------
def test_large_case(ctx):
    n, K = 20, 2000
    offs, sets, scores = pr.make_lists(n, "sparse", 2020, max_parents=3, keep=0.4)
    lz, edge, _ = ctx.posterior(offs, sets, scores)
    parents, order, weight = ctx.posterior_sample(K, seed=20)
    assert np.all(np.sort(order, axis=1) == np.arange(n)), "order is not a permutation"
    pos = np.empty((K, n), dtype=np.int64)
    np.put_along_axis(pos, order.astype(np.int64), np.broadcast_to(np.arange(n), (K, n)), axis=1)
    total = np.zeros(K, dtype=np.float64)
    for v in range(n):
        mine = sets[offs[v]:offs[v + 1]]
        srt = np.argsort(mine)
        at = np.searchsorted(mine[srt], parents[:, v])
        assert np.all(at < len(mine)) and np.all(mine[srt][np.minimum(at, len(mine) - 1)] == parents[:, v]), f"variable {v}: a set not stored"
        total = total + scores[offs[v]:offs[v + 1]][srt][at].astype(np.float64)
        for u in range(n):
            has = ((parents[:, v] >> np.uint64(u)) & np.uint64(1)) == 1
            assert np.all(pos[has, u] < pos[has, v]), f"a parent {u} after its child {v}"
            p = float(edge[u, v])
            sd = np.sqrt(K * p * max(1 - p, 0.0))
            assert abs(int(has.sum()) - K * p) <= 6 * sd + 1e-6, (u, v, int(has.sum()), K * p, sd)
    assert total.tobytes() == weight.tobytes()


# ---- 5. errors ---------------------------------------------------------------------------------------
def test_errors(ctx):
    with pytest.raises(ulg.ULGError) as e:  # before any posterior call
        ctx.posterior_sample(4)
    assert _status(e) == STATUS["STATE"]
    assert ulg.lib().ulg_posterior_sample(ctx._h, 0, 0, 0, None, None, None) == STATUS["STATE"]  # also for count = 0
    n, offs, sets, scores = pr.gpu_inputs()["brute-dense-4"]
    ctx.posterior(offs, sets, scores)
    assert ctx.posterior_sample(4)[0].shape == (4, n)
    for first, count in ((-1, 4), (0, -4), (-1, -1), ((1 << 63) - 2, 4)):
        with pytest.raises(ulg.ULGError) as e:
            ctx.posterior_sample(count, first=first)
        assert _status(e) == STATUS["ARG"], (first, count)
    L = ulg.lib()
    assert L.ulg_posterior_sample(ctx._h, 0, 0, 4, None, None, None) == STATUS["ARG"]  # NULL parents
    assert L.ulg_posterior_sample_u(ctx._h, 4, None, None, None, None) == STATUS["ARG"]
    assert L.ulg_posterior_sample(ctx._h, 0, 0, 0, None, None, None) == 0  # count = 0 asks for nothing
    assert L.ulg_posterior_sample(ctx._h, 0, -1, 0, None, None, None) == STATUS["ARG"]  # ... but first is checked
    # buffers that do not fit: refused before anything is allocated (the pointer is never written)
    live = ctx.info("device_bytes_live")
    dummy = (ctypes.c_uint64 * 1)()
    assert L.ulg_posterior_sample(ctx._h, 0, 0, 1 << 45, dummy, None, None) == STATUS["UNSUPPORTED"]
    assert "bytes" in L.ulg_last_error(ctx._h).decode() and ctx.info("device_bytes_live") == live
    bad = sets.copy()
    bad[offs[2] + 1] |= np.uint64(1 << 2)
    with pytest.raises(ulg.ULGError):  # a failed posterior call leaves nothing to sample
        ctx.posterior(offs, bad, scores)
    with pytest.raises(ulg.ULGError) as e:
        ctx.posterior_sample(4)
    assert _status(e) == STATUS["STATE"]
    n, offs, sets, scores = pr.gpu_inputs()["brute-nolist-4"]  # Z = 0
    assert ctx.posterior(offs, sets, scores)[0] == -np.inf
    for call in (lambda: ctx.posterior_sample(4), lambda: ctx.posterior_sample_u(np.zeros((4, n, 2), dtype=np.uint64))):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS["STATE"] and "-inf" in str(e.value)
    assert ctx.posterior_sample(0)[0].shape == (0, n)  # count = 0 does not look at ln Z


def test_a_posterior_call_frees_the_samples_buffers(ctx):
    """The sampler keeps its device buffers from one call to the next; the next posterior call frees them
    before it sizes its tables, so they never count against it."""
    n, offs, sets, scores, _, seed = ps.gpu_inputs()["dense-7"]
    ctx.posterior(offs, sets, scores)
    live = ctx.info("device_bytes_live")
    K = 100000
    a = ctx.posterior_sample(K, seed)
    ctx.posterior_sample_u(ps.draws(seed, 0, 1000, n))
    held = ctx.info("device_bytes_live") - live
    assert held >= K * (9 * n + 8) + 1000 * 16 * n
    assert ctx.info("device_bytes_live") == live + held and _same(a, ctx.posterior_sample(K, seed))  # reused, not regrown
    ctx.posterior(offs, sets, scores)
    assert ctx.info("device_bytes_live") == live
    assert _same(a, ctx.posterior_sample(K, seed))


# ---- 6. sampling changes nothing else ---------------------------------------------------------------
def test_sampling_leaves_the_context_as_it_was(ctx):
    n, N = 6, 200
    X, _ = synth.gaussian_sem(n, N, 4242)
    ctx.load(X, 2.0)
    stored, _ = ctx.score_bge(list(range(n)), [(1 << n) - 1] * n, n - 1)
    lists = ctx.fetch(stored)
    before = ctx.posterior_from_scores()
    tables = [ctx.posterior_table(w, 0).tobytes() for w in (0, 1, 2)]
    a = ctx.posterior_sample(500, seed=3)
    ctx.posterior_sample_u(ps.draws(3, 0, 10, n))
    assert _same(lists, ctx.fetch(stored))
    assert tables == [ctx.posterior_table(w, 0).tobytes() for w in (0, 1, 2)]
    assert _same(before, ctx.posterior_from_scores())
    assert _same(a, ctx.posterior_sample(500, seed=3))
    # the samples are of these lists: the most probable edge is in most of them
    u, v = np.unravel_index(np.argmax(before[1]), (n, n))
    freq = float((((a[0][:, v] >> np.uint64(u)) & np.uint64(1)) == 1).mean())
    p = float(before[1][u, v])
    assert abs(freq - p) <= 6 * np.sqrt(p * (1 - p) / 500) + 1e-9
