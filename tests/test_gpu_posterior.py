"""Exact model averaging on the GPU (ulg_posterior, ulg_posterior_from_scores,
ulg_posterior_table, option "posterior_keep") against tests/posterior_ref.py.

Reference: the lattice recursion in longdouble, itself held to the sum over all
orderings (tests/test_posterior_ref.py); never the code under test.
Tolerance, log domain (ln Z, table entries, set_logpost), and the same figure
as an absolute bound on the edge probabilities, which are at most 1:
    cap = 8 max(e64, 2^-52 (1 + M))
with e64 what the float64 numpy recursion loses against longdouble on that
input and M the largest finite |value| of the reference's tables.  Every
comparison prints "posterior-observed <family> <input> max <figure> cap <cap> e64 <e64>".
Where a table entry is -inf in the reference it must be -inf on the GPU.

The n = 20 case has no reference: invariants only, within
4 n 2^-52 (1 + M) -- a value of f, b or gamma passes through at most 2 n - 1
dependent logaddexp, each good to 2 ulps of a value of magnitude M.
"""
import re

import numpy as np
import pytest
import torch  # at collection, before any test loads libulg.so: imported after it, torch reports no HIP GPU

import posterior_ref as pr
import synth
import ulg

pytestmark = pytest.mark.gpu

STATUS = {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _log_dev(got, want):
    """Largest |got - want| over the finite entries of want; the -inf patterns must agree."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    want = np.atleast_1d(want)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), "finite / -inf pattern differs"
    assert np.all(got[~fin] == -np.inf) and np.all(want[~fin] == -np.inf)
    return float(np.abs(got[fin].astype(np.longdouble) - want[fin]).max()) if fin.any() else 0.0


def _observed(family, name, worst, cap, e64):
    print(f"posterior-observed {family} {name} max {worst:.3g} cap {cap:.3g} e64 {e64:.3g}")
    assert worst <= cap, (family, name, worst, cap)


def _check_outputs(family, name, got, want, ref):
    """ref: posterior_ref.reference() of the input, for its cap and e64."""
    lz, edge, lp = got
    cap, e64 = ref["cap"], ref["e64"]
    worst = max(_log_dev(lz, want["log_z"]), _log_dev(lp, want["set_logpost"]))
    _observed(family, name, worst, cap, e64)
    de = float(np.abs(edge.astype(np.longdouble) - want["edge"]).max())
    _observed(family + "-edges", name, de, cap, e64)
    assert np.all(np.diag(edge) == 0) and np.all(edge >= 0) and np.all(edge <= 1 + cap)


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- 1. the sum over all orderings ---------------------------------------------------------
@pytest.mark.parametrize("kind", pr.BRUTE_KINDS)
def test_brute_force(ctx, kind):
    """n = 1 .. 7 against the sum over all n! orderings."""
    for n in range(1, 8):
        name = f"brute-{kind}-{n}"
        _, offs, sets, scores = pr.gpu_inputs()[name]
        r = pr.reference(name, n, offs, sets, scores)
        cap = r["cap"]
        want = pr.brute(n, offs, sets, scores)
        lz, edge, lp = got = ctx.posterior(offs, sets, scores)
        assert edge.shape == (n, n) and len(lp) == len(sets)
        if kind == "nolist":  # Z = 0: the call succeeds
            assert lz == -np.inf and np.all(lp == -np.inf) and np.all(edge == 0)
            continue
        _check_outputs("brute", name, got, want, r)
        for v in range(n):
            assert abs(np.exp(lp[offs[v]:offs[v + 1]]).sum() - 1) <= cap + 2.0 ** -52 * (offs[v + 1] - offs[v])
        if kind == "solo":  # the last variable's only set is the empty one
            assert lp[-1] == 0.0 and np.all(edge[:, n - 1] == 0)
        assert ctx.posterior(offs, sets, scores, want_sets=False)[2] is None


# ---- 2. every entry of every table ---------------------------------------------------------
@pytest.mark.parametrize("n", pr.TABLE_NS)
def test_every_table_entry(ctx, n):
    """n - 1 = 9, 10, 11: one below, at and one above the tile kernel's 10 bits; n = 16: bits 10 .. 13 in
    the first strided launch, bit 14 in a second one."""
    name = f"tables-{n}"
    _, offs, sets, scores = pr.gpu_inputs()[name]
    r = pr.reference(name, n, offs, sets, scores)
    ld, cap = r["ld"], r["cap"]
    ctx.set_option("posterior_keep", 1)
    got = ctx.posterior(offs, sets, scores)
    _check_outputs("tables", name, got, ld, r)
    worst = {"alpha": 0.0, "f": 0.0, "b": 0.0, "gamma": 0.0}
    f, b = ctx.posterior_table(1), ctx.posterior_table(2)
    assert len(f) == len(b) == 1 << n
    worst["f"], worst["b"] = _log_dev(f, ld["f"]), _log_dev(b, ld["b"])
    assert f[0] == 0.0 and b[0] == 0.0 and f[-1] == got[0]
    for v in range(n):
        a, g = ctx.posterior_table(0, v), ctx.posterior_table(3, v)
        assert len(a) == len(g) == 1 << (n - 1)
        worst["alpha"] = max(worst["alpha"], _log_dev(a, ld["alpha"][v]))
        worst["gamma"] = max(worst["gamma"], _log_dev(g, ld["gamma"][v]))
    for key, w in worst.items():
        _observed("tables-" + key, name, w, cap, r["e64"])
    assert ctx.info("posterior_bytes") == 8 * (2 * n * (1 << (n - 1)) + 2 * (1 << n))
    # one gamma table reused: the same outputs, and table 3 is not there
    ctx.set_option("posterior_keep", 0)
    again = ctx.posterior(offs, sets, scores)
    assert _same(got, again)
    assert ctx.info("posterior_bytes") == 8 * ((n + 1) * (1 << (n - 1)) + 2 * (1 << n))
    with pytest.raises(ulg.ULGError) as e:
        ctx.posterior_table(3, 0)
    assert _status(e) == STATUS["STATE"]
    assert ctx.posterior_table(0, n - 1).tobytes() == a.tobytes()
    with pytest.raises(ulg.ULGError) as e:
        ctx.posterior_table(0, n)
    assert _status(e) == STATUS["ARG"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.posterior_table(4, 0)
    assert _status(e) == STATUS["ARG"]


# ---- 3. dynamic range ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 9])
def test_dynamic_range(ctx, n):
    """Scores over +-2e4 nats with gaps on both sides of the cut (tests/test_posterior_ref.py checks the
    inputs): no linear-space sum survives these."""
    name = f"dynamic-{n}"
    _, offs, sets, scores = pr.gpu_inputs()[name]
    r = pr.reference(name, n, offs, sets, scores)
    ctx.set_option("posterior_keep", 1)
    got = ctx.posterior(offs, sets, scores)
    assert np.isfinite(got[0]) and abs(got[0]) > 1e3
    _check_outputs("dynamic", name, got, r["ld"], r)
    worst = max(_log_dev(ctx.posterior_table(1), r["ld"]["f"]), _log_dev(ctx.posterior_table(2), r["ld"]["b"]))
    for v in range(n):
        worst = max(worst, _log_dev(ctx.posterior_table(0, v), r["ld"]["alpha"][v]),
                    _log_dev(ctx.posterior_table(3, v), r["ld"]["gamma"][v]))
    _observed("dynamic-tables", name, worst, r["cap"], r["e64"])


# ---- 4. end to end -----------------------------------------------------------------------------
def _end_to_end(ctx, name, n, stored):
    offs, sets, scores = ctx.fetch(stored)
    assert list(offs) == sorted(offs) and len(offs) == n + 1
    ctx.search_from_scores()
    full = [(1 << n) - 1] * n
    before = ctx.astar(edges=full, mode=0, net_text=True)
    a = ctx.posterior_from_scores()
    b = ctx.posterior(offs, sets, scores)
    assert _same(a, b), "posterior_from_scores differs from posterior on the fetched lists"
    r = pr.reference(name, n, offs, sets, scores)
    _check_outputs("e2e", name, a, pr.brute(n, offs, sets, scores), r)
    offs2, sets2, scores2 = ctx.fetch(stored)
    assert _same((offs, sets, scores), (offs2, sets2, scores2))
    after = ctx.astar(edges=full, mode=0, net_text=True)
    assert before["net_text"] == after["net_text"] and before["expanded"] == after["expanded"]
    assert np.float32(before["cost"]).tobytes() == np.float32(after["cost"]).tobytes()
    assert np.array_equal(before["vpar"], after["vpar"])
    return a


def test_end_to_end_bge(ctx):
    n, N = 6, 200
    X, _ = synth.gaussian_sem(n, N, 4242)
    ctx.load(X, 2.0)
    stored, _ = ctx.score_bge(list(range(n)), [(1 << n) - 1] * n, n - 1)
    lz, edge, lp = _end_to_end(ctx, "e2e-bge", n, stored)
    assert np.isfinite(lz) and edge.max() > 0.5  # a SEM with edges: something is nearly certain


def test_end_to_end_bdeu(ctx):
    n, N = 6, 200
    rng = np.random.default_rng(77)
    codes = rng.integers(0, 3, size=(N, n))
    codes[:, 1] = (codes[:, 0] + (rng.random(N) < 0.2)) % 3
    codes[:, 4] = (codes[:, 2] + codes[:, 3] + (rng.random(N) < 0.1)) % 3
    ctx.load_discrete(codes, [3] * n)
    stored, _ = ctx.score_discrete(list(range(n)), [(1 << n) - 1] * n, n - 1, kind=ulg.Context.SCORE_BDEU)
    lz, edge, lp = _end_to_end(ctx, "e2e-bdeu", n, stored)
    assert np.isfinite(lz) and edge[0, 1] + edge[1, 0] > 0.9  # the copied column


# ---- 5. determinism ----------------------------------------------------------------------------
def test_bit_identical_across_calls_and_contexts(ctx):
    name = "tables-12"
    n, offs, sets, scores = pr.gpu_inputs()[name]
    a = ctx.posterior(offs, sets, scores)
    fa = ctx.posterior_table(1)
    b = ctx.posterior(offs, sets, scores)
    assert _same(a, b) and fa.tobytes() == ctx.posterior_table(1).tobytes()
    other = ulg.Context(0)
    try:
        other.set_option("posterior_keep", 1)  # another table layout, the same bits
        c = other.posterior(offs, sets, scores)
        assert _same(a, c) and fa.tobytes() == other.posterior_table(1).tobytes()
        assert other.posterior_table(2).tobytes() == ctx.posterior_table(2).tobytes()
    finally:
        other.close()


def test_a_destroyed_context_gives_its_tables_back(ctx):
    live = ctx.info("device_bytes_live")
    n, offs, sets, scores = pr.gpu_inputs()["tables-12"]
    other = ulg.Context(0)
    try:
        other.set_option("posterior_keep", 1)
        other.posterior(offs, sets, scores)
        assert ctx.info("device_bytes_live") >= live + other.info("posterior_bytes")
    finally:
        other.close()
    assert ctx.info("device_bytes_live") == live


def test_device_lists(ctx):
    name = "brute-sparse-7"
    n, offs, sets, scores = pr.gpu_inputs()[name]
    a = ctx.posterior(offs, sets, scores)
    ds = torch.from_numpy(sets.view(np.int64)).cuda()
    dc = torch.from_numpy(scores).cuda()
    torch.cuda.synchronize()
    b = ctx.posterior(offs, ds.data_ptr(), dc.data_ptr(), device_ptrs=True)
    assert _same(a, b)


# ---- 6. a large case: invariants -----------------------------------------------------------------
def test_large_case_invariants(ctx):
    n = 20
    offs, sets, scores = pr.make_lists(n, "sparse", 2020, max_parents=3, keep=0.4)
    lz, edge, lp = ctx.posterior(offs, sets, scores)
    f, b = ctx.posterior_table(1), ctx.posterior_table(2)
    M = max(float(np.abs(f[np.isfinite(f)]).max()), float(np.abs(b[np.isfinite(b)]).max()))
    tol = 4 * n * 2.0 ** -52 * (1.0 + M)
    print(f"posterior-observed large n20 |b(V) - f(V)| {abs(b[-1] - f[-1]):.3g} tol {tol:.3g} M {M:.6g} sets {len(sets)}")
    assert np.isfinite(lz) and lz == f[-1] and abs(b[-1] - f[-1]) <= tol
    assert np.all(np.isfinite(lp)) and np.all(lp <= tol)
    worst_sum = worst_edge = 0.0
    p = np.exp(lp)
    for v in range(n):
        sl = slice(offs[v], offs[v + 1])
        worst_sum = max(worst_sum, abs(p[sl].sum() - 1))
        for u in range(n):
            has = ((sets[sl] >> np.uint64(u)) & np.uint64(1)) == 1
            worst_edge = max(worst_edge, abs(p[sl][has].sum() - edge[u, v]))
    print(f"posterior-observed large n20 sum-to-one {worst_sum:.3g} edge-vs-sets {worst_edge:.3g}")
    assert worst_sum <= tol + 2.0 ** -52 * 1200 and worst_edge <= tol + 2.0 ** -52 * 1200
    assert np.all(np.diag(edge) == 0)
    assert ctx.info("posterior_bytes") == 8 * ((n + 1) * (1 << (n - 1)) + 2 * (1 << n))
    # alpha of the full predecessor set: the plain sum of the list, in log space
    for v in (0, n - 1):
        a = ctx.posterior_table(0, v)
        x = scores[offs[v]:offs[v + 1]].astype(np.float64)
        want = x.max() + np.log(np.exp(x - x.max()).sum())
        assert abs(a[-1] - want) <= tol


# ---- 7. refusals -----------------------------------------------------------------------------------
def test_too_many_variables(ctx):
    live = ctx.info("device_bytes_live")
    with pytest.raises(ulg.ULGError) as e:
        ctx.posterior(np.zeros(30, dtype=np.int64), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.float32))
    assert _status(e) == STATUS["UNSUPPORTED"] and "bytes" in str(e.value)
    assert ctx.info("device_bytes_live") == live
    with pytest.raises(ulg.ULGError) as e:
        ctx.posterior_table(1)
    assert _status(e) == STATUS["STATE"]


def test_partial_scoring_call(ctx):
    with pytest.raises(ulg.ULGError) as e:
        ctx.posterior_from_scores()
    assert _status(e) == STATUS["STATE"]
    n = 6
    X, _ = synth.gaussian_sem(n, 200, 4242)
    ctx.load(X, 2.0)
    ctx.score_bge([0, 1, 2], [(1 << n) - 1] * 3, 3)
    with pytest.raises(ulg.ULGError) as e:
        ctx.posterior_from_scores()
    assert _status(e) == STATUS["STATE"]


def _bad_lists():
    """name -> (offsets, sets, scores), each wrong in one way (n = 4, or 0)."""
    n, offs, sets, scores = pr.gpu_inputs()["brute-dense-4"]
    out = {}
    out["n-below-1"] = (np.zeros(1, dtype=np.int64), sets, scores)
    o = offs.copy()
    o[2] = o[1] - 1
    out["offsets"] = (o, sets, scores)
    s = sets.copy()
    s[offs[2] + 1] |= np.uint64(1 << 2)
    out["own-bit"] = (offs, s, scores)
    s = sets.copy()
    s[offs[1] + 2] |= np.uint64(1 << 4)
    out["bit-n"] = (offs, s, scores)
    s = sets.copy()
    s[offs[3] + 5] |= np.uint64(1 << 63)
    out["bit-63"] = (offs, s, scores)
    s = sets.copy()
    s[offs[0] + 3] = s[offs[0] + 6]
    out["duplicate"] = (offs, s, scores)
    for key, bad in (("nan", np.nan), ("inf", np.inf), ("minus-inf", -np.inf)):
        c = scores.copy()
        c[offs[3] - 1] = bad
        out[key] = (offs, sets, c)
    return out


@pytest.mark.parametrize("device", [False, True])
def test_bad_lists(ctx, device):
    n, offs, sets, scores = pr.gpu_inputs()["brute-dense-4"]
    good = ctx.posterior(offs, sets, scores)
    for key, (o, s, c) in _bad_lists().items():
        with pytest.raises(ulg.ULGError) as e:
            if device:
                ds, dc = torch.from_numpy(s.view(np.int64)).cuda(), torch.from_numpy(c).cuda()
                torch.cuda.synchronize()
                ctx.posterior(o, ds.data_ptr(), dc.data_ptr(), device_ptrs=True)
            else:
                ctx.posterior(o, s, c)
        assert _status(e) == STATUS["ARG"], key
        # a refused call leaves no tables to read
        if key != "n-below-1" and key != "offsets":
            with pytest.raises(ulg.ULGError) as e:
                ctx.posterior_table(1)
            assert _status(e) == STATUS["STATE"], key
    assert _same(good, ctx.posterior(offs, sets, scores))
