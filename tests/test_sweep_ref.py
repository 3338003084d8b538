"""CPU tests that hold tests/sweep_ref.py, the reference the GPU order-graph
sweep is compared with node by node (test_gpu_sweep_exact.py).

fl32(x + c) is monotone in x, so the layer DP's g(goal) is also the minimum
over all m! orders of the sequential float32 sum: a brute force over
permutations, with bs() by a direct scan of the lists, shares no structure
with the reference (no lattice, no zeta transform, no layers, no ordkey)."""
import itertools
from math import comb

import numpy as np
import pytest

import sweep_ref as sr


def _bs_scan(offsets, sets, costs, v, P):
    """(cost, parents) of the first stored subset of P in (cost, file order);
    python floats compare -0.0 == 0.0, so signed zeros tie onto the index."""
    best = None
    for i in range(int(offsets[v]), int(offsets[v + 1])):
        s = int(sets[i])
        if s & ~P == 0:
            k = (float(costs[i]), i)
            if best is None or k < best:
                best = k
    return (np.float32(best[0]), int(sets[best[1]])) if best else (sr.FLT_MAX, 0)


def _brute(n, offsets, sets, costs, rows):
    memo = {}
    best = None
    for perm in itertools.permutations(range(n)):
        g, P, ok = np.float32(0.0), 0, True
        for v in perm:
            if rows is not None and P != 0 and (P & rows[v]) == 0:
                ok = False
                break
            if (v, P) not in memo:
                memo[(v, P)] = _bs_scan(offsets, sets, costs, v, P)[0]
            g = np.float32(g + memo[(v, P)])
            P |= 1 << v
        if ok and (best is None or g < best):
            best = g
    return best


def _tie_costs(rng, k):
    return rng.integers(-5, 1, k).astype(np.float32) * np.float32(0.5)


@pytest.mark.parametrize("skeleton", [False, True])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6, 7])
def test_goal_cost_is_the_minimum_over_all_orders(m, skeleton):
    for seed in range(20):
        rng = np.random.default_rng(1000 * m + seed)
        cost = sr.float_costs if seed % 2 == 0 else _tie_costs
        offsets, sets, costs = sr.make_lists(m, [list(range(m))] * m, rng, 6, cost)
        rows = None
        if skeleton:  # any rows, symmetric or not; some leave no admissible order
            rows = [int(rng.integers(0, 1 << m)) & ~(1 << v) for v in range(m)]
            if seed % 3 == 0:
                rows = [r & int(rng.integers(0, 1 << m)) for r in rows]
        cv = list(range(m))
        res = sr.sweep(m, cv, sr.bs_tables(m, offsets, sets, costs, cv), rows)
        want = _brute(m, offsets, sets, costs, rows)
        if want is None:
            assert res["order"] is None and res["cost"] == sr.FLT_MAX, (m, seed)
            continue
        assert res["cost"].tobytes() == want.tobytes(), (m, seed, float(res["cost"]), float(want))
        # the returned chain is one of those orders and sums to that cost
        g, P = np.float32(0.0), 0
        for v in res["order"]:
            assert rows is None or P == 0 or P & rows[v]
            c, par = _bs_scan(offsets, sets, costs, v, P)
            assert res["parents"][v] == par
            g = np.float32(g + c)
            P |= 1 << v
        assert g.tobytes() == want.tobytes()


def test_bs_tables_equal_oracle_bestscore(oracle_built):
    n = 8
    for seed, cost in ((1, sr.float_costs), (2, _tie_costs)):
        rng = np.random.default_rng(seed)
        offsets, sets, costs = sr.make_lists(n, [list(range(n))] * n, rng, 25, cost)
        if seed == 2:
            costs[::3] = np.float32(-0.0)  # signed zeros among the ties
        S = oracle_built.Search(n, offsets, sets, costs)
        cv = list(range(n))
        cost_t, par_t = sr.bs_tables(n, offsets, sets, costs, cv)
        for v in range(n):
            for P in range(1 << n):
                c, par = S.bestscore(v, P)
                assert np.float32(c) == cost_t[v][P] and par == int(par_t[v][P]), (v, P)
                c2, par2 = _bs_scan(offsets, sets, costs, v, P)
                assert np.float32(c) == c2 and par == par2, (v, P)


def test_bs_tables_ignore_sets_outside_the_component():
    n = 6
    rng = np.random.default_rng(3)
    offsets, sets, costs = sr.make_lists(n, [list(range(n))] * n, rng, 12, sr.float_costs)
    cv = [1, 3, 4]
    cost_t, par_t = sr.bs_tables(n, offsets, sets, costs, cv)
    for j, v in enumerate(cv):
        for Pc in range(8):
            P = sum(1 << cv[b] for b in range(3) if (Pc >> b) & 1)
            c, par = _bs_scan(offsets, sets, costs, v, P)
            assert cost_t[j][Pc].tobytes() == c.tobytes() and int(par_t[j][Pc]) == par


def _int_costs(rng, k):
    return rng.integers(1, 200, k).astype(np.float32)


def _ring_skeleton(n, chords):
    rows = [0] * n
    for a, b in [(i, (i + 1) % n) for i in range(n)] + chords:
        rows[a] |= 1 << b
        rows[b] |= 1 << a
    return rows


@pytest.mark.parametrize("n", [10, 12])
@pytest.mark.parametrize("sparse", [False, True])
def test_integer_costs_equal_oracle_astar_exactly(oracle_built, n, sparse):
    """Integer costs: every float sum is exact, so the exact-order A* and the
    layer DP must agree on the optimal cost to the bit."""
    rng = np.random.default_rng(40 + n)
    if sparse:
        rows = _ring_skeleton(n, [(0, n // 2), (2, n - 3)])
        pools = [[p for p in range(n) if (rows[v] >> p) & 1] for v in range(n)]
    else:
        rows = [(1 << n) - 1] * n
        pools = [list(range(n))] * n
    offsets, sets, costs = sr.make_lists(n, pools, rng, 30, _int_costs)
    ref = oracle_built.Search(n, offsets, sets, costs).astar(edges=rows)
    assert ref["rc"] == 0
    res, _ = sr.search(n, offsets, sets, costs, rows)
    assert len(res) == 1
    assert res[0]["cost"].tobytes() == np.float32(ref["cost"]).tobytes()
    if sparse:
        assert (res[0]["leaves"][1:] == sr.UNREACHED).any()


def test_layer_order_is_colex_rank():
    m = 6
    layers = sr.layer_nodes(m)
    assert [len(x) for x in layers] == [comb(m, d) for d in range(m + 1)]
    assert sorted(int(t) for x in layers for t in x) == list(range(1 << m))
    for d, nodes in enumerate(layers):
        for pos, T in enumerate(nodes):
            elems = [b for b in range(m) if (int(T) >> b) & 1]
            assert len(elems) == d
            assert sum(comb(a, i + 1) for i, a in enumerate(elems)) == pos, (d, pos, int(T))


def test_ordkey_order_and_signed_zero():
    f = np.array([-3.5, -0.0, 0.0, 1e-30, 2.0, 3e38], dtype=np.float32)
    k = sr.ordkey(f)
    assert k[1] == k[2] and list(k) == sorted(k)
    back = sr.ord_cost(k)
    assert back[1].tobytes() == np.float32(0.0).tobytes()
    assert back[[0, 3, 4, 5]].tobytes() == f[[0, 3, 4, 5]].tobytes()


def test_shard_keys_format():
    m = 4
    rng = np.random.default_rng(5)
    offsets, sets, costs = sr.make_lists(m, [list(range(m))] * m, rng, 5, sr.float_costs)
    cv = list(range(m))
    rows = [0b0010, 0b0101, 0b1010, 0b0100]  # a path: {0, 2} and others are unreached
    res = sr.sweep(m, cv, sr.bs_tables(m, offsets, sets, costs, cv), rows)
    keys = sr.shard_keys(res)
    for d in range(1, m + 1):
        for T, k in zip(res["layers"][d], keys[d]):
            if res["leafpos"][T] == sr.UNREACHED:
                assert int(k) == sr.UNREACHED_KEY
            else:
                assert int(k) & 0xFF == res["leafpos"][T]
                assert sr.ord_cost(np.uint32(int(k) >> 8)).tobytes() == res["g"][T].tobytes()
    assert res["leafpos"][0b0101] == sr.UNREACHED and res["leafpos"][0b0011] != sr.UNREACHED
