"""The ladders' reference (tests/order_mc3_ref.py) held to the mathematics on the CPU, the host arithmetic
(bin/order_mc3_check), and the condition under which the GPU tests demand equality."""
import os
import subprocess

import numpy as np
import pytest

import order_mc3_ref as m3
import order_mcmc_ref as om
from conftest import PKG

LD = np.longdouble


@pytest.mark.parametrize("sub", ("", "san"))
def test_order_mc3_check(sub):
    exe = os.path.join(PKG, "bin", sub, "order_mc3_check")
    if sub and not os.path.exists(exe):
        subprocess.run(["make", "-C", PKG, "bin/san/order_mc3_check"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("name", sorted(om.chain_inputs()))
@pytest.mark.parametrize("R,E", m3.LADDER_CASES)
def test_no_undecided_step_at_any_ladder_input(name, R, E):
    r = m3.ladder_reference(name, R, E)
    print(f"{name} R={R} E={E}: accepted by rung {r['accepted'].sum(axis=0)}, swaps by pair {r['swaps'].sum(axis=0)} of "
          f"{len(r['swap_d'])} rounds; the smallest margin lies {r['min_excess']} units above its slack")
    assert r["undecided"] == 0 and r["records"] == m3.LADDER_STEPS // om.CHAIN_THIN and len(r["swap_d"]) == m3.LADDER_STEPS // E
    assert np.all(np.sort(r["replica"], axis=1) == r["replica"].min(axis=1, keepdims=True) + np.arange(R))
    assert r["swaps"].sum() > 0


def test_no_undecided_step_at_the_statistical_input():
    L = om.stat_inputs()[4][0]
    r = m3.run(L, m3.STAT_SEED, 4096, m3.STAT_BETAS, 1, m3.STAT_T[4], thin=m3.STAT_T[4], want_parents=False)
    assert r["undecided"] == 0 and r["records"] == 1


def test_one_rung_is_the_chains_reference():
    for name, (L, seed) in om.chain_inputs().items():
        a, b = m3.run(L, seed, 3, [1.0], 5, 40, om.CHAIN_THIN), om.run(L, seed, 3, 40, om.CHAIN_THIN)
        for k in ("order", "parents", "log_weight", "log_score"):
            assert np.array_equal(a[k], b[k]), (name, k)
        assert np.array_equal(a["trace_delta"][:, :, 0], b["trace_delta"]) and np.array_equal(a["accepted"][:, 0], b["accepted"])
        assert np.array_equal(a["final_order"][:, 0], b["final_order"]) and a["swap_d"].size == 0


@pytest.mark.parametrize("n", (3, 4))
def test_the_product_law_is_stationary_and_reached(n):
    """mu = pi x pi^0.3 under one step's joint matrix J (moves, then the exchange) and under the moves
    alone (odd rounds consider no pair at R = 2).  Each rule accepts on floor(exp(.) 2^52) of 2^52 values,
    below the exact ratio by less than 2^-52: the flow into a state misses balance by at most 2^-52 times
    probabilities that sum to at most 1.  Then the law after the T steps of the GPU test, from the
    shuffle's uniform start, t = 1 .. T with the exchange at even t."""
    L = om.stat_inputs()[n][0]
    perms, M, J = m3.joint_step(L, m3.STAT_BETAS)
    _, pi, hot = m3.ladder_law(L, m3.STAT_BETAS)
    mu = np.kron(pi, hot)
    assert np.all(M >= 0) and np.all(J >= 0) and float(np.abs(J.sum(axis=1) - 1).max()) < 1e-17
    dev = max(float(np.abs(mu @ J - mu).max()), float(np.abs(mu @ M - mu).max()))
    assert np.array_equal(m3.move_matrix(L, 1.0)[1], om.transition_matrix(L)[1])
    d = np.full(len(mu), LD(1) / len(mu))
    for t in range(1, m3.STAT_T[n] + 1):
        d = d @ (J if t % 2 == 0 else M)
    tv = 0.5 * float(np.abs(d - mu).sum())
    print(f"n = {n}: |mu J - mu| <= {dev:.3g} (2^-52 = {2.0 ** -52:.3g}); total variation {tv:.3g} after {m3.STAT_T[n]} steps")
    assert dev <= 2.0 ** -52 and tv <= 1e-4
