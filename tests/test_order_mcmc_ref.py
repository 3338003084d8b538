"""The order MCMC's reference (tests/order_mcmc_ref.py) held to the mathematics,
on the CPU, and the host arithmetic of csrc/order_mcmc_dev.h
(bin/order_mcmc_check).

  * Detailed balance at n = 3 and 4: the one-step matrix over all n! orders,
    built from the rule's integers (the counts of the 2^32 words behind each
    position, the threshold floor(exp(delta) 2^52) of the 2^52 values of
    U_acc >> 12), against the order posterior pi summed over all n! orders in
    long double.
  * Total variation: P^T from the uniform start (the shuffle's, up to the 2^-32
    grain of its words) is within 1e-4 of pi at the T and inputs the
    statistical tests use -- a condition on those inputs, checked here.
  * The law of the (order, DAG) pairs at n = 3 by Pearson's chi-square.
  * No undecided step at any input and seed of the GPU tests.
  * ulg.order_rhat against its definition.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import order_mcmc_ref as om
import ulg
from conftest import PKG

CHECK = os.path.join(PKG, "bin", "order_mcmc_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "order_mcmc_check")
LD = np.longdouble


def test_order_mcmc_check():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "order_mcmc_check ok" in r.stdout, (r.stdout, r.stderr)


def test_order_mcmc_check_under_sanitizers():
    if not os.path.exists(SAN_CHECK):
        subprocess.run(["make", "-C", PKG, "bin/san/order_mcmc_check"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "order_mcmc_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- the pieces ---------------------------------------------------------------------------
def test_draws_and_moves():
    seed, t, n = 0x299f31d0a4093822, (1 << 32) + 5, 7
    i, j, u = om.moves(seed, t, np.arange(6), n)
    for c in range(6):
        w = om.ps.philox((t & om.M32, t >> 32, c, 0), (seed & om.M32, seed >> 32))
        jp = (w[1] * (n - 1)) >> 32
        assert int(i[c]) == (w[0] * n) >> 32 and int(j[c]) == jp + (jp >= int(i[c])) and int(u[c]) == w[2] | (w[3] << 32)
    assert np.all(i != j)
    for n in (1, 2, 33, 63):
        o = om.shuffle(5, np.arange(40), n)
        assert np.all(np.sort(o, axis=1) == np.arange(n))
    # chain c's order does not depend on which chains are asked for
    assert np.array_equal(om.shuffle(5, np.array([3, 9]), 33), om.shuffle(5, np.arange(40), 33)[[3, 9]])
    for m in (1, 2, 3, 5, 62, 63):
        cnt = om.mulhi_counts(m)
        assert sum(cnt) == 1 << 32 and max(cnt) - min(cnt) <= 1
        edge = np.cumsum([0] + cnt[:-1])
        assert all(((int(e) * m) >> 32) == k and (e == 0 or (((int(e) - 1) * m) >> 32) == k - 1) for k, e in enumerate(edge))


def test_terms_against_a_plain_sum():
    """terms() against the definition ln sum exp in long double, entry by entry, and its special values."""
    for name, L in om.term_cases().items():
        rng = np.random.default_rng(len(name))
        orders = np.array([rng.permutation(L.n) for _ in range(3)])
        a, cap, single = om.order_terms(L, orders)
        pre = om.prefixes(orders)
        for k in range(len(orders)):
            for p in range(L.n):
                v, U = int(orders[k, p]), int(pre[k, p])
                comp = [float(x) for S, x in zip(L.sets[v], L.sc[v]) if int(S) & ~U == 0]
                if not comp:
                    assert a[k, p] == -np.inf
                    continue
                m = max(comp)
                want = LD(m) + np.log(sum((np.exp(LD(x) - LD(m)) for x in comp), LD(0)))
                # the floors: at most one unit of 2^-52 per entry, relative to a sum of at least 1
                assert abs(a[k, p] - want) <= len(comp) * 2.0 ** -52 + 2 * np.spacing(abs(float(want))), (name, k, p)
                assert cap[k, p] > 0 and single[k, p] == (len(comp) == 1)
                if len(comp) == 1:
                    assert a[k, p] == LD(comp[0])
    # the carry: 4200 entries at the maximum
    L = om.term_cases()["lengths-63"]
    a, _, _ = om.terms(L, [7], [np.uint64((1 << 63) - 1) & ~np.uint64(1 << 7)])
    assert abs(float(a[0]) - (3.5 + math.log(4200))) < 0.2 and float(a[0]) >= 3.5 + math.log(4200)


def test_the_gpu_term_orders_reach_the_carry():
    """The condition the GPU term test rests on: among the (order, position) pairs it scores on "lengths-63"
    there are, for each long list, pairs whose T is 2^64 or more (T_hi = 1: the two-word reduction and the
    term's high word are exercised there), and pairs just below 2^64 with T_hi = 0 on the same list."""
    orders = om.term_orders("lengths-63")
    L = om.term_cases()["lengths-63"]
    sums = []
    a, _, _ = om.order_terms(L, orders, sums)
    T = np.array(sums, dtype=object).reshape(orders.shape)
    assert len(orders) == 36 and np.all(np.sort(orders, axis=1) == np.arange(L.n))
    for v in om.LONG_VARS:
        mine = T[orders == v]
        over = [int(x) for x in mine if x >= 1 << 64]
        assert len(over) >= 2 and all(x >> 64 == 1 and x >= 4200 << 52 for x in over)
        assert any(1 << 63 <= x < 1 << 64 for x in mine)
        print(f"variable {v}: {len(over)} scored pairs with T_hi = 1, the largest T = {max(over) / 2.0 ** 64:.4f} x 2^64; "
              f"the largest below: {max(int(x) for x in mine if x < 1 << 64) / 2.0 ** 64:.4f} x 2^64")
    # every other pair stays in one word
    assert all(int(x) < 1 << 64 for x in T[~np.isin(orders, om.LONG_VARS)])
    for name in om.term_cases():
        assert len(np.unique(om.term_orders(name), axis=0)) == len(om.term_orders(name))


# ---- detailed balance, mixing ------------------------------------------------------------
_MATRIX = {}


def _matrix(n):
    if n not in _MATRIX:
        L = om.stat_inputs()[n][0]
        perms, num, den = om.transition_matrix(L)
        _, pi = om.order_law(L)
        _MATRIX[n] = (perms, num, den, pi)
    return _MATRIX[n]


@pytest.mark.parametrize("n", (3, 4))
def test_detailed_balance(n):
    """pi_k P_kl = pi_l P_lk.  The move k -> l and its reverse use the same two positions, so the words'
    counts behind them are the same integers and cancel; what is left is the acceptance.  With
    delta = ln pi_l - ln pi_k < 0 the rule accepts k -> l on q = floor(exp(delta) 2^52) of 2^52 values and
    l -> k always: pi_k q 2^-52 is within pi_k 2^-52 (the floor) of pi_k exp(delta) = pi_l, beyond what
    long double moves exp, the terms' sums and pi (each a few units of 2^-64 relative; 2^-58 is taken).
    Hence, with g_kl = P's proposal mass of the pair (the counts over 2^64),
        |pi_k P_kl - pi_l P_lk| <= g_kl (max(pi_k, pi_l) 2^-52 + min(pi_k, pi_l) 2^-58).
    Rows sum to 1 exactly: the numerators are integers over 2^116 and the diagonal is the non-negative rest."""
    perms, num, den, pi = _matrix(n)
    L = om.stat_inputs()[n][0]
    ci, cj = om.mulhi_counts(n), om.mulhi_counts(n - 1)
    assert len(perms) == math.factorial(n) and abs(float(pi.sum()) - 1) < 1e-15 and np.all(pi > 0)
    worst = 0.0
    for k, row in enumerate(num):
        assert sum(row) == den and row[k] >= 0 and all(x >= 0 for x in row)
        assert sum(1 for x in row if x) <= 1 + n * (n - 1) // 2
        for l in range(k + 1, len(perms)):
            if not (row[l] or num[l][k]):
                continue
            (i, j) = [p for p in range(n) if perms[k][p] != perms[l][p]]
            g = LD(ci[i] * cj[j - 1] + ci[j] * cj[i]) / LD(2.0 ** 64)
            lhs, rhs = pi[k] * (LD(row[l]) / LD(den)), pi[l] * (LD(num[l][k]) / LD(den))
            bound = g * (max(pi[k], pi[l]) * LD(2.0 ** -52) + min(pi[k], pi[l]) * LD(2.0 ** -58))
            assert abs(lhs - rhs) <= bound, (n, perms[k], perms[l], float(lhs), float(rhs), float(bound))
            worst = max(worst, float(abs(lhs - rhs) / bound))
    print(f"detailed balance n = {n}: {len(perms)} orders, the largest deviation is {worst:.3f} of its bound; lists {L.offsets[-1]} entries")


@pytest.mark.parametrize("n", sorted(om.stat_inputs()))
def test_chains_have_mixed_at_the_step_the_statistical_tests_record(n):
    perms, num, den, pi = _matrix(n)
    T = om.stat_inputs()[n][2]
    P = np.array([[float(LD(x) / LD(den)) for x in row] for row in num])
    d = np.full(len(perms), 1.0 / len(perms))
    for _ in range(T):
        d = d @ P
    tv = 0.5 * float(np.abs(d - pi.astype(np.float64)).sum())
    print(f"n = {n}: total variation {tv:.3g} after {T} steps from the uniform start; acceptance under pi "
          f"{float(((1 - np.diag(P)) * pi.astype(np.float64)).sum()):.3f}; smallest pi {float(pi.min()):.3g}")
    assert tv <= 1e-4


_STAT_RUNS = {}


def _stat_run(n):
    if n not in _STAT_RUNS:
        L, seed, T, chains = om.stat_inputs()[n]
        _STAT_RUNS[n] = om.run(L, seed, chains, T, thin=T)
    return _STAT_RUNS[n]


def test_order_dag_pairs_follow_their_exact_law():
    L, seed, T, K = om.stat_inputs()[3]
    r = _stat_run(3)
    assert r["records"] == 1 and r["undecided"] == 0
    counts = {}
    for o, p in zip(r["order"][0], r["parents"][0]):
        key = (tuple(int(x) for x in o), tuple(int(x) for x in p))
        counts[key] = counts.get(key, 0) + 1
    om.chi_square("pairs-3", counts, om.pair_law(L), K, ulg.chi2_log_sf)


# ---- the GPU tests' condition -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(om.chain_inputs()))
def test_no_undecided_step_at_any_chain_input(name):
    L, seed = om.chain_inputs()[name]
    r = om.chain_reference(name)
    steps = om.CHAIN_STEPS * om.CHAIN_MAX
    print(f"{name}: {steps} steps ({int(r['accepted'].sum())} accepted) and {r['records'] * om.CHAIN_MAX * L.n} picks, "
          f"the smallest margin lies {r['min_excess']} units above its slack; the largest delta cap {r['trace_cap'].max():.3g}")
    assert r["undecided"] == 0
    assert r["records"] == om.CHAIN_STEPS // om.CHAIN_THIN
    # what a record is: a permutation, stored sets that precede their child, the stated sums
    assert np.all(np.sort(r["order"], axis=2) == np.arange(L.n))
    assert 0 < r["accepted"].sum() < steps
    for c in (0, om.CHAIN_MAX - 1):
        pred, w = 0, np.zeros(L.n)
        for p in range(L.n):
            v, e = int(r["order"][-1, c, p]), int(r["entry"][-1, c, p])
            assert L.offsets[v] <= e < L.offsets[v + 1] and int(L.sets_all[e]) == int(r["parents"][-1, c, v])
            assert int(L.sets_all[e]) & ~pred == 0
            w[v] = float(L.scores_all[e])
            pred |= 1 << v
        tot = 0.0
        for v in range(L.n):
            tot += w[v]
        assert tot == r["log_weight"][-1, c]
    # a run split in two, and a run of fewer chains, are the same chains
    a = om.run(L, seed, 3, 50, om.CHAIN_THIN)
    b = om.run(L, seed, 3, om.CHAIN_STEPS - 50, om.CHAIN_THIN, t0=50, state=a["final_order"])
    assert np.array_equal(np.concatenate([a["order"], b["order"]]), r["order"][:, :3])
    assert np.array_equal(np.concatenate([a["parents"], b["parents"]]), r["parents"][:, :3])
    assert np.array_equal(a["accepted"] + b["accepted"], r["accepted"][:3])


@pytest.mark.parametrize("n", sorted(om.stat_inputs()))
def test_no_undecided_step_at_any_statistical_input(n):
    r = _stat_run(n)
    print(f"n = {n}: the smallest margin lies {r['min_excess']} units above its slack")
    assert r["undecided"] == 0


# ---- R-hat ---------------------------------------------------------------------------------------
def test_order_rhat():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(50, 8))
    R, C = x.shape
    mc = x.mean(axis=0)
    W = x.var(axis=0, ddof=1).mean()
    B = R * mc.var(ddof=1)
    want = math.sqrt(((R - 1) / R * W + B / R) / W)
    assert abs(ulg.order_rhat(x) - want) < 1e-12
    assert ulg.order_rhat(x + np.arange(C) * 10.0) > 5  # chains that sit apart
    assert math.isnan(ulg.order_rhat(x[:1])) and math.isnan(ulg.order_rhat(x[:, :1])) and math.isnan(ulg.order_rhat(np.zeros((5, 3))))
    with pytest.raises(ulg.ULGError):
        ulg.order_rhat(np.zeros(5))
