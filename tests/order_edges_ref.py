"""The contract of ulg_order_edges (include/ulg.h, "edge term"; the kernel is
csrc/order_edges.hip) restated in Python integers and numpy.longdouble.  No
GPU, no project binding.  It reuses order_mcmc_ref's Lists, prefixes, weight_q
and caps.

  row      for variable v with predecessor set U: m = the maximum of float64(s_i)
           over the compatible entries (P_i subset of U); q_i = floor(exp(s_i - m)
           2^52), exp in long double here; T = sum q_i and, for u in U, N_u = the
           sum of q_i over the compatible entries with u in P_i: Python integers.
           g(u -> v) = floor(N_u 2^40 / T) in integers: the ratio itself, without
           the contract's two conversions and its FP64 division, which the cap
           below allows for.  No compatible entry: the order has probability 0
           and adds nothing anywhere.

What the device may differ by, and the cap the GPU tests hold it to; it is not
measured on the device.

CAP.  The device's exp moves each counted q by at most 8 units (ULP_ALLOWANCE,
as order_mcmc_ref's term cap argues: 4 ulp of exp, each at most a unit below
2^52, one for the floor, 8 taken).  With k counted entries N' = N + a and
T' = T + b with |a|, |b| <= 8 k, so
    |N'/T' - N/T| = |a T - b N| / (T T') <= 16 k / T'
and T' >= T - 8 k >= T (1 - 2^-36) (T >= 2^52, k < 2^13 here): 16 k / T up to
a factor that the last "+ 2" below absorbs many times over.  The two
conversions y(.) round once each per word and once in their add, the division
once: at most 2^-50 relative together, on a ratio of at most 1.  The floor
moves the value by less than one unit, and so does this module's own.  So the
device's g lies within
    cap = ceil(2^40 (16 k / T + 2^-50)) + 2
units of g here.  T >= 2^52 makes the first term at most k 2^-8: the cap is 3
units wherever fewer than 256 entries count, and tests/test_order_edges_ref.py
prints the largest over the tests' inputs and asserts that none comes near
2^39, where 0 and 2^40 could be taken for one another.
EXACT.  Where one entry is compatible, or all compatible entries agree on u
(every one holds it, or none does), N_u is T or 0 whatever the weights are:
the tests demand g = 2^40 or 0 to the bit.  So is every entry of a row
outside U, the diagonal, and every entry of an order of probability 0.
"""
import math
from fractions import Fraction

import numpy as np

import order_mcmc_ref as om

LD = np.longdouble
U64 = np.uint64
EDGE_BITS = 40
FULL = 1 << EDGE_BITS
MAX_ORDERS = 1 << 22

_BITS = {}  # id(Lists) -> per variable the (entries, n) membership matrix, uint64 0/1
_ROWS = {}  # (id(Lists), v, U) -> row()


def _bits(L, v):
    key = id(L)
    if key not in _BITS:
        _BITS[key] = (L, {})  # L kept alive: an id is not reused while this holds it
    per = _BITS[key][1]
    if v not in per:
        per[v] = ((L.sets[v][:, None] >> np.arange(L.n, dtype=U64)[None, :]) & U64(1)).astype(U64)
    return per[v]


def row(L, v, U):
    """-> (g: list of n Python ints, cap: int, exact: bool (n), dead: bool, N: list of n ints, T: int) for
    variable v with predecessor mask U (module docstring).  dead: no compatible entry; g is then all 0."""
    key = (id(L), int(v), int(U))
    if key in _ROWS:
        return _ROWS[key]
    n = L.n
    S, sc = L.sets[v], L.sc[v]
    compat = (S & ~U64(U)) == U64(0) if len(S) else np.zeros(0, dtype=bool)
    if not compat.any():
        out = ([0] * n, 0, np.ones(n, dtype=bool), True, [0] * n, 0)
        _ROWS[key] = out
        _bits(L, v)  # holds L
        return out
    m = sc[compat].max()
    q, val = om.weight_q(np.where(compat, sc.astype(LD) - LD(m), LD(-np.inf)))  # an incompatible entry weighs 0
    q = q.astype(U64)
    k = int((val >= 0.5).sum())
    B = _bits(L, v)
    hi, lo = q >> U64(32), q & U64(om.M32)
    T = (int(hi.sum(dtype=U64)) << 32) + int(lo.sum(dtype=U64))
    Nh, Nl = hi @ B, lo @ B  # below 2^13 entries of at most 2^32 each: exact in uint64
    N = [(int(h) << 32) + int(l) for h, l in zip(Nh, Nl)]
    assert T >= om.ONE and all(x <= T for x in N)
    g = [(x << EDGE_BITS) // T for x in N]
    cap = math.ceil(Fraction((16 * k) << EDGE_BITS, T) + Fraction(1, 1 << 10)) + 2
    holds = B[compat].sum(axis=0)
    exact = (holds == 0) | (holds == int(compat.sum()))
    for u in range(n):
        if exact[u]:
            assert g[u] in (0, FULL)
    out = (g, cap, exact, False, N, T)
    _ROWS[key] = out
    return out


def order_edges(L, orders):
    """The per-order tables of orders int (K, n): dict of g uint64 (K, n, n) with g[k, u, v] = g(u -> v) of
    order k (all 0 for an order of probability 0), cap int64 (K, n, n), exact bool (K, n, n), dead bool (K)."""
    orders = np.asarray(orders, dtype=np.int64)
    K, n = orders.shape
    pre = om.prefixes(orders)
    g = np.zeros((K, n, n), dtype=U64)
    cap = np.zeros((K, n, n), dtype=np.int64)
    exact = np.ones((K, n, n), dtype=bool)
    dead = np.zeros(K, dtype=bool)
    for k in range(K):
        rows = [row(L, int(orders[k, p]), int(pre[k, p])) for p in range(n)]
        if any(r[3] for r in rows):
            dead[k] = True
            continue
        for p, r in enumerate(rows):
            v = int(orders[k, p])
            g[k, :, v] = np.array(r[0], dtype=U64)
            cap[k, :, v] = np.where(r[2], 0, r[1])
            exact[k, :, v] = r[2]
    return {"g": g, "cap": cap, "exact": exact, "dead": dead}


def group_sum(g, groups):
    """The tables of ulg_order_edges from per-order ones: order k into group k mod groups; uint64 (groups, n, n)."""
    K, n = g.shape[0], g.shape[1]
    out = np.zeros((groups, n, n), dtype=U64)
    for r in range(groups):
        out[r] = g[r::groups].sum(axis=0, dtype=U64)
    return out


def equal_lists(n, score=-2.5):
    """"equal-n": variable n - 1 lists all 2^(n-1) subsets of the others at one score, every other variable the
    empty set alone.  With n - 1 at position p >= 1 the 2^p compatible subsets weigh 2^52 each and half of
    them hold any given predecessor: g(u -> n-1) = 2^39 to the bit, whatever exp does (exp(0) = 1).  Last,
    at n = 14: N_u = 4096 2^52 = 2^64 (hi = 1, lo = 0), T = 2^65; at n = 15: N_u = 2^65, T = 2^66."""
    offs = list(range(n)) + [n - 1 + (1 << (n - 1))]
    sets = [0] * (n - 1) + list(range(1 << (n - 1)))
    scores = [0.25 * v for v in range(n - 1)] + [score] * (1 << (n - 1))
    return om.Lists(n, np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))


def equal_orders(n):
    """Variable n - 1 last (after the others ascending, and descending), at every position p = 0 .. n - 2 after
    the first p others, and two random orders; uint8, distinct rows."""
    last = n - 1
    others = list(range(last))
    rng = np.random.default_rng(1400 + n)
    orders = [others + [last], others[::-1] + [last]] + [others[:p] + [last] + others[p:] for p in range(last)]
    orders += [list(rng.permutation(n)) for _ in range(2)]
    return np.unique(np.array(orders, dtype=np.uint8), axis=0)


CONTRACT_CASES = ("full-1", "full-2", "full-5", "sparse-33", "sparse-63", "lengths-63", "dynamic-6")
EQUAL_SIZES = (14, 15)
_INPUTS = None
_REF = {}


def gpu_inputs():
    """name -> (Lists, orders uint8 (K, n)): every deterministic input of tests/test_gpu_order_edges.py -- the
    term cases with their orders, "equal-14" and "equal-15", and "all-5": all 120 orders of full-5."""
    global _INPUTS
    if _INPUTS is None:
        import itertools
        out = {name: (om.term_cases()[name], om.term_orders(name)) for name in CONTRACT_CASES}
        for n in EQUAL_SIZES:
            out[f"equal-{n}"] = (equal_lists(n), equal_orders(n))
        out["all-5"] = (om.term_cases()["full-5"], np.array(list(itertools.permutations(range(5))), dtype=np.uint8))
        _INPUTS = out
    return _INPUTS


def reference(name):
    """order_edges() of gpu_inputs()[name], computed once and shared."""
    if name not in _REF:
        L, orders = gpu_inputs()[name]
        _REF[name] = order_edges(L, orders)
    return _REF[name]


def stat_orders_reference():
    """The reference's own chains of the statistical test: order_mcmc_ref.stat_inputs()[6], one record at its
    step T -> (Lists, orders uint8 (chains, n), parents uint64 (chains, n))."""
    L, seed, T, chains = om.stat_inputs()[6]
    r = om.run(L, seed, chains, T, thin=T)
    return L, r["order"][0], r["parents"][0]


def variances(g, parents):
    """(sum over the edges of the empirical variance across orders of g / 2^40, the same of the 0/1 indicator
    [u in Pa_v] of `parents` uint64 (K, n)), ddof = 1, float64."""
    K, n = parents.shape
    x = g.astype(np.float64) / FULL
    ind = ((parents[:, None, :] >> np.arange(n, dtype=U64)[None, :, None]) & U64(1)).astype(np.float64)  # [k, u, v]
    return float(x.var(axis=0, ddof=1).sum()), float(ind.var(axis=0, ddof=1).sum())
