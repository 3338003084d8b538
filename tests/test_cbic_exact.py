"""The long-double cBIC reference (tests/cbic_exact.py) and its bound, the
parts that need no GPU: the reference against the oracle where both are
defined, the kernels' operation order restated in NumPy FP64 (with the guarded
pivot) against the bound on every data class of test_gpu_cbic_conditioning.py
-- the proof that the reference side alone satisfies every cap the GPU test
sets -- and the lists of the exact-dependency inputs with their decision
margins."""
import functools
import math

import numpy as np
import pytest

import cbic_exact as ce

F32 = np.float32
# five times the 1e-6 the GPU's scores agree with the oracle's to on benign data
MARGIN_CAP = 5e-6


@pytest.mark.parametrize("name", ["benign", "benign_N50"])
def test_cbic_exact_equals_the_oracle_on_full_rank_data(oracle_built, name):
    """Within 1 float32 ulp of Dataset.cbic_raw (the per-row OLS in FP64)."""
    d = ce.data_class(name)
    ds = oracle_built.Dataset(d["X"])
    for (v, P, _), ref in zip(ce.class_cases(name), ce.class_reference(name)):
        assert ref[3] == len(ce.members(P, v))  # full rank
        want = F32(ds.cbic_raw(d["lam"], v, P))
        got = F32(-ref[0])
        assert abs(float(got) - float(want)) <= float(np.spacing(np.abs(want))), (v, hex(P), got, want)


def test_cbic_exact_on_the_empty_set_and_the_own_bit():
    d = ce.data_class("benign")
    ex = ce.Exact(d["X"])
    assert ex.cbic(3, 0, 2.0)[0] == 0.0
    assert ex.cbic(3, ce.bits(3), 2.0)[0] == 0.0
    assert ex.cbic(3, ce.bits(1, 3, 7), 2.0) == ex.cbic(3, ce.bits(1, 7), 2.0)


def test_rank_rule_drops_the_redundant_parent():
    """A duplicate, an affine copy and a sum of two others: the rank is |P| - 1
    and rss equals the set's without the redundant column; the penalty still
    counts |P|."""
    for name, P, Q in (("duplicate", ce.bits(0, 4, 5), ce.bits(0, 4)), ("affine", ce.bits(4, 5, 9), ce.bits(4, 9)),
                       ("integer_sum", ce.bits(1, 2, 3, 8), ce.bits(1, 2, 8))):
        d = ce.data_class(name)
        ex = ce.Exact(d["X"])
        s_p, rss_p, b_p, rank_p = ex.cbic(10, P, d["lam"])
        s_q, rss_q, b_q, rank_q = ex.cbic(10, Q, d["lam"])
        L = len(ce.members(P))
        assert rank_p == L - 1 and rank_q == L - 1
        assert abs(float(rss_p - rss_q)) <= 1e-17 * float(rss_q)
        assert abs((s_q - s_p) - d["lam"] * math.log(d["N"])) <= 1e-9
        # inside the dependency the perfect fit has rss = 0 up to the long-double rounding
    d = ce.data_class("duplicate")
    score, rss, _, _ = ce.cbic_exact(d["X"], 5, ce.bits(4), d["lam"])
    assert float(rss) <= 1e-30 and score > 1000.0


def test_constant_column_is_nan_and_nothing_else_is():
    c = ce.constant_case()
    ex = ce.Exact(c["X"])
    k = c["constant"]
    assert math.isnan(ex.cbic(0, ce.bits(1, k), c["lam"])[0])
    assert math.isnan(ex.cbic(k, ce.bits(1, 2), c["lam"])[0])
    assert math.isfinite(ex.cbic(0, ce.bits(1, 2), c["lam"])[0])


@functools.lru_cache(maxsize=None)
def _restated(name):
    """-> (largest |rss - rss_ref| / B1 over the resolvable cases, cases outside
    the dependency, resolvable ones among them, contract violations)."""
    d = ce.data_class(name)
    G = ce.gram_fp64(d["X"])
    worst, out, out_res, bad = 0.0, 0, 0, []
    for (v, P, outside), ref in zip(ce.class_cases(name), ce.class_reference(name)):
        L = len(ce.members(P, v))
        score, rss = ce.restate_fp64(G, d["N"], v, P, d["lam"])
        B1 = ce.b1(d["N"], L, ref[2])
        res = ce.resolvable(ref[1], ce.C_BOUND * B1)
        if res:
            worst = max(worst, abs(float(rss) - float(ref[1])) / B1)
        msg = ce.check_value(score, d["N"], L, d["lam"], ref)[1]
        if math.isnan(float(score)):
            msg = "NaN"
        if msg is not None:
            bad.append((v, hex(P), msg))
        out += outside
        out_res += outside and res
    return worst, out, out_res, bad


@pytest.mark.parametrize("name", ce.CLASSES)
def test_fp64_restatement_keeps_the_contract(name):
    """The kernels' operation order in NumPy FP64, guarded pivot included: rss
    within C B1 of the long-double value on every resolvable case, the score
    within its bound, an unresolvable set at +inf or above its floor, never
    NaN; and the classes the GPU test caps are at least 90 % resolvable."""
    worst, out, out_res, bad = _restated(name)
    print(f"{name}: largest |rss - rss_ref| / B1 = {worst:.2f} over the resolvable cases; "
          f"{out_res} of {out} cases outside the dependency resolvable")
    assert not bad, bad[:5]
    assert worst <= ce.C_BOUND
    if name in ce.CAPPED:
        assert out >= 60 and out_res >= 0.9 * out


def test_fp64_restatement_ratio_leaves_room_for_the_gpu():
    """The largest ratio over every class, about 9 of the C = 64: the rest is
    for the GPU's Gram matrix (2.4e-15 (N - 1) per entry measured) and FMA
    contraction."""
    worst = max(_restated(name)[0] for name in ce.CLASSES)
    print(f"largest ratio over every class: {worst:.2f}")
    assert worst <= ce.C_BOUND


@pytest.mark.parametrize("name", ["duplicate", "affine", "integer_sum", "integer_sum_dup"])
def test_unguarded_pivot_breaks_the_contract(name):
    """The same operation order without the guard: a pivot that is rounding
    noise gives NaN or an enormous 1 / d on the rank-deficient sets -- the
    contract is one the unguarded factorisation fails."""
    d = ce.data_class(name)
    G = ce.gram_fp64(d["X"])
    bad = 0
    for (v, P, _), ref in zip(ce.class_cases(name), ce.class_reference(name)):
        score, _ = ce.restate_fp64(G, d["N"], v, P, d["lam"], guard=False)
        bad += ce.check_value(score, d["N"], len(ce.members(P, v)), d["lam"], ref)[1] is not None
    assert bad >= 5


@pytest.mark.parametrize("name", ["k4", "k10"])
def test_exact_lists_of_the_dependent_inputs(name):
    """Restatement over cbic_exact for the variables outside the dependencies:
    every score finite, no set with a redundant parent stored on its merit (it
    is dominated by the set without it), and every store decision is at least
    5e-6 relative from its threshold."""
    c = ce.list_case(name)
    lists = ce.exact_lists(name)
    assert sorted(lists) == sorted(c["outside"]) and lists
    for v, (sets, scores, margin) in lists.items():
        print(f"{name} variable {v}: {len(sets)} stored sets, decision margin {margin:.3e}")
        assert margin >= MARGIN_CAP
        assert np.all(np.isfinite(scores))
        for s, sc in zip(sets, scores):
            s = int(s)
            redundant = (s & ce.bits(4, 5)) == ce.bits(4, 5) or (s & ce.bits(1, 2, 3)) == ce.bits(1, 2, 3)
            # the_score >= 0 is stored by the caller whatever its subsets hold (score_calculator.cpp:111)
            assert not redundant or sc < 0, hex(s)
    if name == "k4":
        assert len(c["inside"]) == 5 and len(c["outside"]) == 5


def test_the_oracle_is_no_standard_for_the_dependent_inputs(oracle_built):
    """The oracle's singular pin (+inf for an exactly zero LU pivot, stored at
    -inf by the reference's loop) is unpinned: its list of a variable outside
    the dependencies holds sets the exact lists do not."""
    c = ce.list_case("k4")
    ds = oracle_built.Dataset(c["X"])
    v = c["outside"][0]
    sets, scores = ds.score_variable(c["lam"], v, (1 << c["n"]) - 1, c["k"])
    assert np.isinf(scores).sum() > 0
    assert len(sets) > len(ce.exact_lists("k4")[v][0])


def test_forms_case_stores_every_layer(oracle_built):
    """Ten informative parents: the oracle's list of the child holds all 1024
    sets, so every layer 1 .. 10 stores some."""
    c = ce.forms_case()
    ds = oracle_built.Dataset(c["X"])
    sets, _ = ds.score_variable(c["lam"], c["v"], (1 << c["n"]) - 1, c["k"])
    assert len(sets) == 1024
