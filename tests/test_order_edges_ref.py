"""The reference of ulg_order_edges (tests/order_edges_ref.py) held to the
mathematics, on the CPU, and the host arithmetic of csrc/order_edges_dev.h
(bin/order_edges_check, and bin/san/order_edges_check under ASan + UBSan).

  * The identity the estimator rests on: the per-order values, weighted by the
    exact order law over all n! orders, give the exact edge matrix
    (posterior_ref.brute) within (cap + 1) 2^-40.
  * An order of probability 0 adds nothing and is counted.
  * Every input of the GPU tests: no cap near 2^39, N <= T, g <= 2^40, the
    "equal" inputs' values to the bit.
  * The variance claim of the GPU's statistical test on the reference's own
    chains.
  * ulg.order_edge_posterior against its definition.
"""
import os
import subprocess

import numpy as np
import pytest

import order_edges_ref as oe
import order_mcmc_ref as om
import posterior_ref as pr
import ulg
from conftest import PKG

CHECK = os.path.join(PKG, "bin", "order_edges_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "order_edges_check")
LD = np.longdouble


def test_order_edges_check():
    if not os.path.exists(CHECK):
        pytest.skip("bin/order_edges_check is not built")
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "order_edges_check ok" in r.stdout, (r.stdout, r.stderr)


def test_order_edges_check_under_sanitizers():
    if not os.path.exists(SAN_CHECK):
        subprocess.run(["make", "-C", PKG, "bin/san/order_edges_check"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "order_edges_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


IDENTITY = {"full-5": lambda: om.make_lists(5, 505), "k3-6": lambda: om.make_lists(6, 606, max_parents=3),
            "dynamic-6": lambda: om.term_cases()["dynamic-6"]}


@pytest.mark.parametrize("name", sorted(IDENTITY))
def test_order_average_is_the_exact_edge_matrix(name):
    L = IDENTITY[name]()
    perms, pi = om.order_law(L)
    ref = oe.order_edges(L, np.array(perms, dtype=np.int64))
    assert np.all(pi[ref["dead"]] == 0)  # an order of probability 0 has weight 0 in the law too
    mean = (pi[:, None, None] * ref["g"].astype(LD)).sum(axis=0) / LD(oe.FULL)
    want = pr.brute(L.n, *L.triple())["edge"]
    cap = ref["cap"].max(axis=0)
    dev = np.abs(mean.astype(np.float64) - want)
    print(f"order-edges-identity {name}: largest deviation {dev.max():.3g}, largest cap {cap.max()} units")
    assert np.all(dev <= (cap + 1) * 2.0 ** -oe.EDGE_BITS), (name, dev.max())


def test_an_order_of_probability_zero_adds_nothing():
    L = om.term_cases()["dynamic-6"]
    orders = np.array([[1, 0, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]], dtype=np.uint8)  # variable 1 has no empty set
    ref = oe.order_edges(L, orders)
    assert list(ref["dead"]) == [True, False] and not ref["g"][0].any() and ref["exact"][0].all()
    assert ref["g"][1, 0, 1] == oe.FULL  # every entry of variable 1 compatible with {0} is {0} itself
    assert np.array_equal(oe.group_sum(ref["g"], 1)[0], ref["g"][1])


@pytest.mark.parametrize("name", sorted(oe.gpu_inputs()))
def test_gpu_inputs_are_decidable(name):
    """No value sits where its cap would let 0 and 2^40 be confused; the reference's own invariants."""
    L, orders = oe.gpu_inputs()[name]
    ref = oe.reference(name)
    g, cap = ref["g"].astype(np.int64), ref["cap"]
    print(f"order-edges-inputs {name}: {len(orders)} orders, {int(ref['dead'].sum())} of probability 0, largest cap {cap.max()} units")
    assert cap.max() < 1 << 12 and np.all(g <= oe.FULL) and np.all(g >= 0)
    assert np.all((g[ref["exact"]] == 0) | (g[ref["exact"]] == oe.FULL))
    n = L.n
    assert not g[:, np.arange(n), np.arange(n)].any()
    # an entry that is not exact lies strictly between the two: neither end is within its cap's reach of the other
    loose = ~ref["exact"]
    assert np.all(cap[loose] >= 3) and np.all(cap[~loose] == 0)
    if name == "dynamic-6":
        assert ref["dead"].sum() >= 1 and np.array_equal(ref["dead"], orders[:, 0] == 1)  # variable 1 lists no empty set
    if name.startswith("equal-"):
        last = n - 1
        pre = om.prefixes(orders)
        for k in range(len(orders)):
            p = int(np.flatnonzero(orders[k] == last)[0])
            want = np.zeros((n, n), dtype=np.int64)
            for u in range(n):
                if (int(pre[k, p]) >> u) & 1:
                    want[u, last] = oe.FULL // 2
            assert np.array_equal(g[k], want) and ref["exact"][k][:, :last].all()
        # the carry: variable n - 1 last sums past 2^64 in N as well as in T
        _, _, _, _, N, T = oe.row(L, last, (1 << last) - 1)
        assert T == 1 << (52 + last) and T >= 1 << 65 and all(x == T // 2 and x >= 1 << 64 for x in N[:last])


def test_rao_blackwell_variance_is_below_the_indicator_on_the_reference_chains():
    L, orders, parents = oe.stat_orders_reference()
    ref = oe.order_edges(L, orders)
    assert not ref["dead"].any()
    rb, ind = oe.variances(ref["g"], parents)
    print(f"order-edges-variance reference: Rao-Blackwell {rb:.4f}, indicator {ind:.4f} (summed over the edges)")
    assert rb < ind


def test_order_edge_posterior():
    rng = np.random.default_rng(5)
    n, G = 4, 5
    counts = np.array([3, 0, 2, 4, 1])
    e = (rng.integers(0, oe.FULL, size=(G, n, n), dtype=np.uint64) * counts[:, None, None].astype(np.uint64))
    mean, se = ulg.order_edge_posterior(e, counts)
    tot = np.zeros((n, n), dtype=object)
    for g in range(G):
        tot = tot + e[g].astype(object)
    assert np.array_equal(mean, np.array([[float(int(x)) / (float(oe.FULL) * 10.0) for x in r] for r in tot]))
    m = np.stack([e[g] / (float(oe.FULL) * counts[g]) for g in (0, 2, 3, 4)])
    want = np.sqrt(((m - m.mean(axis=0)) ** 2).sum(axis=0) / (4 * 3))
    assert np.allclose(se, want, rtol=1e-12, atol=0)
    one = ulg.order_edge_posterior(e[0], 3)
    assert one.shape == (n, n) and np.array_equal(one, e[0] / (float(oe.FULL) * 3.0))
    same = np.tile(e[:1], (3, 1, 1))
    mean, se = ulg.order_edge_posterior(same, [3, 3, 3])
    assert np.array_equal(mean, one) and not se.any()
    _, se = ulg.order_edge_posterior(e[:2], counts[:2])  # one group that counts: no standard error
    assert np.isnan(se).all()
    for bad_e, bad_c in ((e, counts[:3]), (e, [0] * G), (e, [-1, 1, 1, 1, 1]), (e[0, :2], 3), (np.ones((2, n, n), dtype=np.uint64), [1, 0])):
        with pytest.raises(ulg.ULGError):
            ulg.order_edge_posterior(bad_e, bad_c)
