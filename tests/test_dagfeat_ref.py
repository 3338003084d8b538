"""The structural features' reference (tests/dagfeat_ref.py) held to the definitions, on the CPU;
the host side of csrc/dagfeat_dev.h (bin/dagfeat_check); ulg.uniform_prior_weights; and one
statistical check of what the whole pipeline means.

The statistical check: n = 4, full lists (all 8 subsets of the other three variables for each
variable), scores N(0, 1.5^2) in nats.  The order-modular posterior gives the pair (order, G) the
weight prod_v w_v(Pa_v) when the order is a linear extension of G, so the exact probability of a
feature phi is the sum of the weights of the pairs whose DAG has it over the sum of all 24 * 64
pairs' weights.  Against it: the means of phi over K = 20,000 draws of the reference sampler
(tests/posterior_sample_ref.py), one seed fixed below; every ordered pair (u, v) within 5 standard
deviations sqrt(p (1 - p) / K), for phi = "u ~> v" and phi = "u -> v compelled".
"""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import dagfeat_ref as df
import posterior_ref as pr
import posterior_sample_ref as ps
import ulg
from conftest import PKG

CHECK = os.path.join(PKG, "bin", "dagfeat_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "dagfeat_check")

PIPELINE_SEED = 29029  # picked on the CPU; the draws are those of ps.draws(PIPELINE_SEED, 0, K, 4)
PIPELINE_K = 20000


# ---- the host side of the rules ----------------------------------------------------------------
def test_dagfeat_check():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dagfeat_check ok" in r.stdout, (r.stdout, r.stderr)


def test_dagfeat_check_under_sanitizers():
    if not os.path.exists(SAN_CHECK):
        subprocess.run(["make", "-C", PKG, "bin/san/dagfeat_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "dagfeat_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- the essential graph against the definition ------------------------------------------------
@pytest.mark.parametrize("n,dags,classes", [(3, 25, 11), (4, 543, 185), (5, 29281, 8782)])
def test_meek_closure_equals_the_class_definition(n, dags, classes):
    want, found = df.class_compelled(n)
    assert len(df.all_dags(n)) == dags and found == classes
    wrong = [p for p in df.all_dags(n) if df.essential(n, p) != want[p]]
    assert wrong == []


def test_essential_graph_of_known_shapes():
    n = 63
    assert df.essential(n, df.chain(n)) == [0] * n
    assert df.essential(n, df.collider_chain(n)) == df.collider_chain(n)  # 60 R1 steps down the chain
    assert df.essential(n, df.complete(n)) == [0] * n
    assert df.essential(n, df.star(n)) == df.star(n)
    assert len(df.vstructs(n, df.star(n))) == math.comb(62, 2)
    # R2 alone: 0 -> 1 -> 2 compelled by 3 -> 1's collider makes 0 -> 2 compelled through 1
    par = [0, 0b1001, 0b0011, 0]  # 0 -> 1 <- 3, 1 -> 2, 0 -> 2
    assert df.essential(4, par) == df.class_compelled(4)[0][tuple(par)]


# ---- the closure against reachability by matrix powers ------------------------------------------
def _reach(n, par):
    A = np.array([[(par[v] >> u) & 1 for v in range(n)] for u in range(n)], dtype=np.int64)  # A[u, v] = u -> v
    R, P = np.zeros_like(A), np.eye(n, dtype=np.int64)
    for _ in range(n):
        P = ((P @ A) > 0).astype(np.int64)
        R |= P
    return [sum(1 << u for u in range(n) if R[u, v]) for v in range(n)]


def test_closure_equals_reachability():
    rng = np.random.default_rng(4)
    assert list(df.all_dags(4)) == [p for p in df.all_assignments(4) if not df.is_cyclic(4, p)]  # the sift is the search
    for p in df.all_dags(4):
        assert df.ancestors(4, p) == _reach(4, p)
    for n in (1, 2, 7, 20, 33, 63):
        for kind in ("sparse", "dense"):
            par = df.random_dag(n, kind, rng)
            assert df.ancestors(n, par) == _reach(n, par) and not df.is_cyclic(n, par)
    assert df.ancestors(63, df.chain(63)) == [(1 << v) - 1 for v in range(63)]
    assert df.is_cyclic(2, df.cycle(2)) and df.is_cyclic(63, df.cycle(63))
    assert df.ancestors(3, df.cycle(3)) == _reach(3, df.cycle(3)) == [7, 7, 7]


def test_features_sums_and_cycles():
    """features(): the weights multiply, the cyclic graphs are counted and add nothing."""
    dags = [df.collider_chain(4), df.cycle(4), df.chain(4), df.collider_chain(4)]
    f = df.features(4, dags, [3, 1000, 5, 4])
    assert f["total"] == 12 and f["cyclic"] == 1
    assert f["edge"][0, 2] == 7 and f["edge"][0, 1] == 5 and f["edge"][3, 0] == 0
    assert f["compelled"][0, 2] == 7 and f["compelled"][2, 3] == 7 and f["compelled"][0, 1] == 0
    assert f["ancestor"][0, 3] == 12 and f["ancestor"][1, 3] == 12 and f["ancestor"][3, 0] == 0
    assert f["blanket"][0, 1] == 12 and f["blanket"][1, 0] == 12 and f["blanket"][0, 3] == 0
    assert f["vstruct"][2, 0, 1] == 7 and int(f["vstruct"].sum()) == 7
    g = df.features(4, dags)
    assert g["total"] == 3 and g["edge"][0, 2] == 2


# ---- the integer weights -----------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2 ** 10, 2 ** 10 + 1, 2 ** 20])
def test_uniform_prior_weights_sum_below_2_63(K):
    q = ulg.uniform_prior_weights(np.zeros(K))  # the worst case: every weight the largest
    bits = min(52, 62 - math.ceil(math.log2(K))) if K > 1 else 52
    assert q.dtype == np.uint64 and q.shape == (K,) and all(int(x) == 1 << bits for x in q[[0, K // 2, K - 1]])
    assert sum(int(x) for x in np.unique(q)) * K == K << bits < 2 ** 63


def test_uniform_prior_weights_contract():
    le = np.log(np.array([2.0, 1.0, 8.0, 1.0]))
    q = [int(x) for x in ulg.uniform_prior_weights(le)]  # exp rounds: a unit or two of 2^-52 either way
    assert q[1] == q[3] == 1 << 52 and abs(q[0] - (1 << 51)) <= 2 and abs(q[2] - (1 << 49)) <= 2
    q = ulg.uniform_prior_weights(np.array([0.0, 53 * math.log(2.0) + 1e-9, 700.0]))
    assert [int(x) for x in q] == [1 << 52, 0, 0]  # below 2^-52 of the largest: drops out
    for bad in ([0.0, -np.inf], [0.0, np.nan], [np.inf]):
        with pytest.raises(ulg.ULGError):
            ulg.uniform_prior_weights(np.array(bad))
    with pytest.raises(ulg.ULGError):
        ulg.uniform_prior_weights(np.zeros((2, 2)))


# ---- the pipeline's meaning --------------------------------------------------------------------
def test_sampled_path_and_compelled_frequencies_match_the_exact_posterior():
    n, K = 4, PIPELINE_K
    rng = np.random.default_rng(PIPELINE_SEED)
    offs, sets, _ = pr.make_lists(n, "dense", 1)
    scores = rng.normal(0.0, 1.5, size=len(sets)).astype(np.float32)
    # exact: every (order, DAG) pair
    sc = scores.astype(np.float64)
    where = [{int(S): i for i, S in enumerate(sets[offs[v]:offs[v + 1]], start=int(offs[v]))} for v in range(n)]
    feats = {}
    Z = 0.0
    p_anc, p_cmp = np.zeros((n, n)), np.zeros((n, n))
    pairs = 0
    for order in itertools.permutations(range(n)):
        before = [sum(1 << u for u in order[:order.index(v)]) for v in range(n)]
        choices = [[S for S in where[v] if S & ~before[v] == 0] for v in range(n)]
        for par in itertools.product(*choices):
            if par not in feats:
                feats[par] = (df.ancestors(n, par), df.essential(n, par))
            anc, cmp_ = feats[par]
            wgt = math.exp(sum(sc[where[v][par[v]]] for v in range(n)))
            Z += wgt
            pairs += 1
            for v in range(n):
                for u in df.members(anc[v]):
                    p_anc[u, v] += wgt
                for u in df.members(cmp_[v]):
                    p_cmp[u, v] += wgt
    assert pairs == 24 * 64 and len(feats) == 543
    p_anc, p_cmp = p_anc / Z, p_cmp / Z
    # sampled
    t = pr.lattice(n, offs, sets, scores, dtype=np.float64)
    s = ps.sample(n, offs, sets, scores, t["alpha"], t["f"], ps.draws(PIPELINE_SEED, 0, K, n))
    f = df.features(n, s["parents"])
    assert f["total"] == K and f["cyclic"] == 0
    worst = 0.0
    for name, p in (("ancestor", p_anc), ("compelled", p_cmp)):
        for u in range(n):
            for v in range(n):
                if u == v:
                    assert f[name][u, v] == 0
                    continue
                assert 0.0 < p[u, v] < 1.0
                dev = abs(int(f[name][u, v]) / K - p[u, v]) / math.sqrt(p[u, v] * (1.0 - p[u, v]) / K)
                worst = max(worst, dev)
                assert dev <= 5.0, (name, u, v, int(f[name][u, v]) / K, p[u, v], dev)
    print(f"paths and compelled edges: worst deviation {worst:.2f} sigma over 24 entries")
