"""The cBIC value on ill-conditioned data: the three Cholesky forms of the
scorer (cbic_set_score for layers 1-8, score_wide_kernel for layers 9-31,
score_sets_kernel) against the long-double reference of tests/cbic_exact.py
and its bound.

  a. score_sets per data class -- benign, x2 = x1 + e noise, x0 = 0.7 x1 -
     1.3 x3 + e noise, an exact duplicate, an affine copy, integer data with
     x3 = x1 + x2 (and an extra duplicate), N = 8 (every |P| >= 7 a perfect
     fit): a resolvable set within the score bound, an unresolvable one at
     +inf or above its floor, NaN if and only if the set touches a constant
     column.  The largest ratios go to cbic_conditioning.json in the
     directory of measured reports (test_gpu_search_dag._report).
  b. the lists of the two exact-dependency inputs through the layer and wide
     kernels: outside the dependencies the stored sets are the Restatement's
     over cbic_exact and the scores lie within the bound; inside them the call
     succeeds, stores no NaN, and keeps the unresolvable rule.
  c. the three forms bit for bit at L = 1 .. 10.

tests/test_cbic_exact.py shows on the CPU that the reference side alone meets
every cap set here."""
import math

import numpy as np
import pytest

import cbic_exact as ce
from test_gpu_search_dag import _report as write_report

pytestmark = pytest.mark.gpu

_report = {"what": "per data class: rss_ratio = the largest |rss - rss_ref| / B1 over the resolvable cases, rss out of "
                   "the kernels' operation order (NumPy FP64, no FMA) over the DEVICE's Gram matrix (the kernels "
                   "return float32 scores only, which resolve rss to 2^-24 |score| / N, far coarser than B1); "
                   "score_ratio = the largest |score_gpu - score_ref| / score bound of score_sets itself; C = 64",
           "classes": {}}


def _write_report():
    write_report("cbic_conditioning", _report, filename="cbic_conditioning.json")


@pytest.mark.parametrize("name", ce.CLASSES)
def test_score_sets_within_the_bound(ulg_ctx, name):
    d = ce.data_class(name)
    cases, refs = ce.class_cases(name), ce.class_reference(name)
    ulg_ctx.load(d["X"], d["lam"])
    got = ulg_ctx.score_sets([v for v, _, _ in cases], [P for _, P, _ in cases])
    G = ulg_ctx.gram()
    N, lam = d["N"], d["lam"]
    rss_ratio = score_ratio = 0.0
    out = out_res = unres = 0
    bad = []
    for (v, P, outside), ref, g in zip(cases, refs, got):
        L = len(ce.members(P, v))
        kind, msg = ce.check_value(g, N, L, lam, ref)
        assert kind != "nan"
        if msg is not None:
            bad.append((v, hex(P), msg))
        B1 = ce.b1(N, L, ref[2])
        B = ce.C_BOUND * B1
        res = kind == "resolvable"
        if res:
            _, rss = ce.restate_fp64(G, N, v, P, lam)
            rss_ratio = max(rss_ratio, abs(float(rss) - float(ref[1])) / B1)
            if not math.isnan(float(g)):
                score_ratio = max(score_ratio, abs(float(g) - ref[0]) / ce.score_bound(N, ref[0], ref[1], B))
        unres += not res
        out += outside
        out_res += outside and res
    print(f"{name}: rss ratio {rss_ratio:.2f} (device Gram), score error / bound {score_ratio:.3f}, "
          f"{unres} of {len(cases)} unresolvable, {out_res} of {out} outside the dependency resolvable")
    _report["classes"][name] = dict(N=N, n=d["n"], cases=len(cases), unresolvable=unres, outside=out,
                                    outside_resolvable=out_res, rss_ratio=rss_ratio, score_ratio=score_ratio,
                                    violations=len(bad))
    _write_report()
    assert not bad, bad[:5]
    assert rss_ratio <= ce.C_BOUND
    if name in ce.CAPPED:
        assert out >= 60 and out_res >= 0.9 * out


def test_nan_if_and_only_if_a_constant_column(ulg_ctx):
    c = ce.constant_case()
    n, k = c["n"], c["constant"]
    ulg_ctx.load(c["X"], c["lam"])
    rng = np.random.default_rng(9791)
    vars_, parents = [], []
    for i in range(120):
        v = int(rng.integers(n))
        others = [x for x in range(n) if x != v]
        P = ce.bits(*rng.choice(others, size=1 + i % 6, replace=False))
        vars_.append(v)
        parents.append(P)
    got = ulg_ctx.score_sets(vars_, parents)
    touches = np.array([v == k or bool((P >> k) & 1) for v, P in zip(vars_, parents)])
    assert 20 <= touches.sum() <= 100
    assert np.array_equal(np.isnan(got), touches)
    ex = ce.Exact(c["X"])
    for v, P, g, t in zip(vars_, parents, got, touches):
        kind, msg = ce.check_value(g, c["N"], len(ce.members(P, v)), c["lam"], ex.cbic(v, P, c["lam"]))
        assert (kind == "nan") == bool(t) and msg is None, (v, hex(P), msg)


@pytest.mark.parametrize("name", ["k4", "k10"])
def test_lists_of_the_dependent_inputs(ulg_ctx, name):
    c = ce.list_case(name)
    want = ce.exact_lists(name)
    ulg_ctx.load(c["X"], c["lam"])
    offs, sets, scores = ulg_ctx.score_all(c["variables"], c["cands"], c["k"])  # the call succeeds
    assert ulg_ctx.info("score_error_word") == 0
    assert not np.isnan(scores).any()
    ex = ce.Exact(c["X"])
    top = 0
    for i, v in enumerate(c["variables"]):
        s, sc = sets[offs[i]:offs[i + 1]], scores[offs[i]:offs[i + 1]]
        if v in c["outside"]:
            w = want[v][0]
            if not np.array_equal(s, w):
                a, b = set(int(x) for x in w), set(int(x) for x in s)
                raise AssertionError(f"variable {v}: stored sets differ: only reference {sorted(a - b)[:8]}, "
                                     f"only gpu {sorted(b - a)[:8]} ({len(w)} vs {len(s)})")
        for P, g in zip(s, sc):
            P = int(P)
            L = len(ce.members(P, v))
            top = max(top, L)
            if L == 0:
                assert g.tobytes() == np.float32(-0.0).tobytes()
                continue
            kind, msg = ce.check_value(g, c["N"], L, c["lam"], ex.cbic(v, P, c["lam"]))
            assert msg is None, (v, hex(P), msg)
            if v in c["outside"]:
                assert kind == "resolvable", (v, hex(P))
    print(f"{name}: {len(sets)} stored sets, largest stored |P| = {top}")


@pytest.mark.parametrize("near", [False, True], ids=["informative", "near_collinear"])
def test_three_forms_bit_for_bit(ulg_ctx, near):
    """Every score the layer kernels (L <= 8) and the wide kernels (L = 9, 10)
    store comes back from score_sets with identical bits."""
    c = ce.forms_case(near)
    v, n = c["v"], c["n"]
    ulg_ctx.load(c["X"], c["lam"])
    offs, sets, scores = ulg_ctx.score_all([v], [(1 << n) - 1], c["k"])
    assert ulg_ctx.info("score_error_word") == 0
    layers = np.array([bin(int(s)).count("1") for s in sets])
    per_layer = np.bincount(layers, minlength=11)
    print(f"stored per layer: {per_layer.tolist()}")
    if not near:
        assert np.all(per_layer[1:11] >= 1)
    else:
        assert np.all(per_layer[1:9] >= 1)
    got = ulg_ctx.score_sets([v] * len(sets), sets)
    nonempty = sets != 0
    diff = np.nonzero(got[nonempty].view(np.uint32) != scores[nonempty].view(np.uint32))[0]
    assert len(diff) == 0, [(hex(int(sets[nonempty][i])), float(scores[nonempty][i]), float(got[nonempty][i]))
                            for i in diff[:5]]
