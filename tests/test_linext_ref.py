"""The linear-extension count's reference (tests/linext_ref.py) held to the mathematics, on the
CPU; the host arithmetic of csrc/linext_dev.h (bin/linext_check); and the mathematics of the
reweighting (ulg.uniform_prior_edges) on samples of tests/posterior_sample_ref.py.

The reweighting test: n = 4, full lists (all 8 subsets of the other three variables for each
variable), scores N(0, 1.5^2) in nats, K = 10^5 samples of the reference sampler, one seed fixed
below before its samples were looked at.  The law of a sampled DAG is q(G) = ext(G) w(G) / Z, the
target u(G) = w(G) / Z', w(G) = prod_v w_v(Pa_v), both over the 543 DAGs of n = 4.  For the
indicator phi of an edge, the self-normalised estimate sum r phi / sum r with r = 1 / ext has mean
mu = sum_G u(G) phi(G) and asymptotic variance (the delta method)
  sigma^2 = sum_G q(G) r(G)^2 (phi(G) - mu)^2 / (K (sum_G q(G) r(G))^2).
Every ordered pair must lie within 5 sigma of mu; and the unweighted frequency of at least one
pair must NOT (else the correction would not be needed on this input).
"""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import linext_ref as lx
import posterior_ref as pr
import posterior_sample_ref as ps
import ulg
from conftest import PKG

CHECK = os.path.join(PKG, "bin", "linext_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "linext_check")

REWEIGHT_SEED = 20081  # fixed before any sample of it was drawn
REWEIGHT_K = 100000


# ---- the host arithmetic ---------------------------------------------------------------------
def test_linext_check():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "linext_check ok" in r.stdout, (r.stdout, r.stderr)


def test_linext_check_under_sanitizers():
    if not os.path.exists(SAN_CHECK):
        subprocess.run(["make", "-C", PKG, "bin/san/linext_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "linext_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- the recursion ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 8))
def test_recursion_equals_brute_force(n):
    rng = np.random.default_rng(100 + n)
    dags = [lx.random_dag(n, d, rng) for d in (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0) for _ in range(3)]
    want = [lx.brute(n, par) for par in dags]
    assert [lx.count(n, par) for par in dags] == want
    assert all(w >= 1 for w in want)
    assert [int(x) for x in lx.count_many(n, dags)] == want


def _chain(nodes, par):
    for a, b in zip(nodes, nodes[1:]):
        par[b] = 1 << a


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 11])
def test_closed_forms(n):
    par = [0] * n
    _chain(list(range(n)), par)
    assert lx.count(n, par) == 1
    _chain(list(range(n))[::-1], par := [0] * n)
    assert lx.count(n, par) == 1
    assert lx.count(n, [0] * n) == math.factorial(n)
    for a in range(1, n):  # two disjoint chains, interleaved at will
        par = [0] * n
        nodes = [int(v) for v in np.random.default_rng(n * 31 + a).permutation(n)]
        _chain(nodes[:a], par)
        _chain(nodes[a:], par)
        assert lx.count(n, par) == math.comb(n, a)
    rng = np.random.default_rng(7 * n)
    for _ in range(4):
        par = lx.random_forest(n, rng)
        assert lx.count(n, par) == lx.hook(n, par)
    if n <= 7:
        assert lx.hook(n, par) == lx.brute(n, par)


def test_cycles_count_zero():
    assert lx.count(2, [0b10, 0b01]) == 0
    assert lx.count(3, [0b100, 0b001, 0b010]) == 0
    assert lx.count(6, [0, 0b100000, 0b000010, 0b000100, 0b001000, 0b010000]) == 0  # 1 -> 2 -> 3 -> 4 -> 5 -> 1
    assert lx.count(5, [0, 0b00001, 0b01010, 0b00100, 0b00001]) == 0  # 2 <-> 3 below a root
    assert lx.brute(3, [0b100, 0b001, 0b010]) == 0


def all_assignments(n):
    """Every assignment of a parent mask without the own bit to each variable: (2^(n-1))^n rows."""
    per = [[sum(((i >> j) & 1) << u for j, u in enumerate([u for u in range(n) if u != v])) for i in range(1 << (n - 1))]
           for v in range(n)]
    return np.array(list(itertools.product(*per)), dtype=np.uint64)


@pytest.mark.parametrize("n,dags", [(1, 1), (2, 3), (3, 25), (4, 543), (5, 29281)])
def test_number_of_acyclic_graphs(n, dags):
    pars = all_assignments(n)
    found = sum(int((lx.count_many(n, pars[i:i + 65536]) > 0).sum()) for i in range(0, len(pars), 65536))
    assert found == dags


# ---- the reweighting -------------------------------------------------------------------------
def _reweight_lists(n=4):
    rng = np.random.default_rng(REWEIGHT_SEED)
    offs, sets, _ = pr.make_lists(n, "dense", 1)
    return offs, sets, rng.normal(0.0, 1.5, size=len(sets)).astype(np.float32)


def test_reweighting_recovers_the_uniform_prior_posterior():
    n, K = 4, REWEIGHT_K
    offs, sets, scores = _reweight_lists(n)
    t = pr.lattice(n, offs, sets, scores, dtype=np.float64)
    s = ps.sample(n, offs, sets, scores, t["alpha"], t["f"], ps.draws(REWEIGHT_SEED, 0, K, n))
    parents = s["parents"]
    # the sampled DAGs' counts, duplicates removed
    uniq, inv = np.unique(parents, axis=0, return_inverse=True)
    ext = lx.count_many(n, uniq)[np.asarray(inv).reshape(-1)]
    assert ext.min() >= 1
    log_ext = np.log(ext.astype(np.float64))
    edge, ess = ulg.uniform_prior_edges(parents, log_ext)
    # the exact laws over the 543 DAGs
    sc = scores.astype(np.float64)
    pars = all_assignments(n)
    cnt = lx.count_many(n, pars)
    keep = cnt > 0
    assert int(keep.sum()) == 543
    pars, cnt = pars[keep], cnt[keep].astype(np.float64)
    where = [{int(S): i for i, S in enumerate(sets[offs[v]:offs[v + 1]], start=int(offs[v]))} for v in range(n)]
    w = np.array([math.exp(sum(sc[where[v][int(row[v])]] for v in range(n))) for row in pars])
    q, u, r = cnt * w / (cnt * w).sum(), w / w.sum(), 1.0 / cnt
    qr = (q * r).sum()
    worst, worst_raw, beyond = 0.0, 0.0, 0
    for a in range(n):
        for b in range(n):
            if a == b:
                assert edge[a, b] == 0.0
                continue
            phi = ((pars[:, b] >> np.uint64(a)) & np.uint64(1)).astype(np.float64)
            mu = (u * phi).sum()
            sigma = math.sqrt((q * r * r * (phi - mu) ** 2).sum() / (K * qr * qr))
            dev = abs(edge[a, b] - mu) / sigma
            raw = abs(((parents[:, b] >> np.uint64(a)) & np.uint64(1)).mean() - mu) / sigma
            worst, worst_raw = max(worst, dev), max(worst_raw, raw)
            beyond += raw > 5.0
            assert dev <= 5.0, (a, b, edge[a, b], mu, sigma, dev)
    print(f"reweighting: worst deviation {worst:.2f} sigma over 12 pairs, ESS {ess:.0f} of {K}; "
          f"unweighted: worst {worst_raw:.1f} sigma, {beyond} pairs beyond 5")
    assert beyond >= 1, "the unweighted frequencies are within the bound everywhere: this input needs no correction"
    assert 1.0 <= ess <= K


def test_uniform_prior_edges_contract():
    parents = np.array([[0, 1], [2, 0], [0, 1], [0, 0]], dtype=np.uint64)
    log_ext = np.log(np.array([1.0, 1.0, 1.0, 2.0]))
    edge, ess = ulg.uniform_prior_edges(parents, log_ext)
    r = np.array([1.0, 1.0, 1.0, 0.5])
    assert edge[0, 1] == (r[0] + r[2]) / r.sum() and edge[1, 0] == r[1] / r.sum() and edge[0, 0] == 0.0
    assert ess == r.sum() ** 2 / (r * r).sum()
    with pytest.raises(ulg.ULGError):
        ulg.uniform_prior_edges(parents, np.array([0.0, 0.0, -np.inf, 0.0]))  # a count of 0
    with pytest.raises(ulg.ULGError):
        ulg.uniform_prior_edges(parents, log_ext[:3])
