"""CPU tests of the partition MCMC's restatement (tests/partition_mcmc_ref.py): the
Hastings ratios, the stationary law and what the GPU tests take for granted."""
import numpy as np
import pytest

import order_mcmc_ref as om
import partition_mcmc_ref as pm

LD = np.longdouble


@pytest.mark.parametrize("n,count", [(3, 13), (4, 75)])
def test_detailed_balance_and_the_dag_law(n, count):
    """This test decides the rho's: with the brute-force pi over all DAGs, pi(S) K(S, S') = pi(S') K(S', S)."""
    L = om.make_lists(n, 300 + n, sd=1.5)
    states, K, log_pi = pm.transition_matrix(L)
    assert len(states) == count  # every ordered partition is reached from the flat one
    par, w, part, _ = pm.dag_table(L)
    assert len(par) == {3: 25, 4: 543}[n]
    index = {S: i for i, S in enumerate(states)}
    where = np.array([index[tuple(pm.from_part_of(list(row)))] for row in part])
    pi = np.array([float(w[where == i].sum() / w.sum()) for i in range(count)])
    assert np.all(pi > 0) and abs(pi.sum() - 1) < 1e-12
    # the chain's law prod_v T_v is the DAGs' mass by partition ...
    chain = np.exp(log_pi - log_pi.max())
    assert np.abs(chain / chain.sum() - pi).max() < 1e-12
    # ... and a DAG drawn from its partition's eligible sets has probability prod_v w_v / sum
    for k in range(len(par)):
        S = list(states[where[k]])
        pairs = pm.pairs(S, n)
        assert all(pm.eligible(np.array([par[k, v]], dtype=np.uint64), *pairs[v])[0] for v in range(n))
    cond = np.array([float(w[k] / w[where == where[k]].sum()) for k in range(len(par))])
    assert np.abs(pi[where] * cond - (w / w.sum()).astype(np.float64)).max() < 1e-12
    assert np.abs(K.sum(axis=1) - 1).max() < 1e-12 and K.min() >= 0
    flow = pi[:, None] * K
    assert np.abs(flow - flow.T).max() < 1e-12
    reach = np.linalg.matrix_power((K > 0).astype(np.float64) + np.eye(count), count) > 0
    assert reach.all()  # irreducible
    assert np.abs(pi @ K - pi).max() < 1e-12


@pytest.mark.parametrize("n", sorted(pm.STAT))
def test_the_statistical_inputs_have_mixed(n):
    """After T steps from the flat state the law is within 1e-4 of pi in total variation; at n = 5 the
    order-modular edge posterior misses the uniform-prior one by more than 10 binomial standard deviations of
    4096 draws on some edge, so a test at 5 can tell the two priors apart."""
    L, _, T, chains = pm.STAT[n]
    states, K, log_pi = pm.transition_matrix(L)
    pi = np.exp(log_pi - log_pi.max())
    pi /= pi.sum()
    law = np.linalg.matrix_power(K, T)[states.index(((1 << n) - 1,))]
    assert 0.5 * np.abs(law - pi).sum() < 1e-4
    if n == 5:
        par, w, _, ext = pm.dag_table(L)
        assert len(par) == 29281
        uniform, modular = pm.edge_matrix(par, w, n), pm.edge_matrix(par, w * ext, n)
        sd = np.sqrt(np.maximum(uniform * (1 - uniform), 1e-300) / chains)
        print("largest gap between the priors, in standard deviations:", (np.abs(uniform - modular) / sd).max())
        assert (np.abs(uniform - modular) / sd).max() > 10


@pytest.mark.parametrize("name", sorted(pm.chain_inputs()))
def test_the_chain_inputs_cover_the_moves(name):
    """No undecided step; every move kind and every no-op case within the traced steps; on the sparse lists a
    rejection by a -inf term and a sum of weights past 2^64."""
    ref = pm.chain_reference(name)
    assert ref["undecided"] == 0 and ref["min_excess"] > 0
    want = {"swap", "swap-noop", "topart", "topart-noop", "togap", "togap-noop", "split", "split-noop", "join", "join-noop"}
    assert want <= ref["labels"], want - ref["labels"]
    assert ref["accepted"].min() > 0
    if name.startswith("sparse"):
        assert "-inf" in ref["labels"] and ref["max_T"] >= 1 << 64
    if name == "sparse-63":
        assert ref["parts"].max() == 63  # tau up to 126
    print(name, "mean |D| =", np.mean(ref["sizes"]), "accepted", ref["accepted"])
