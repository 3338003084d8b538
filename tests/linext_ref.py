"""The number of linear extensions of a DAG (ulg_dag_linear_extensions, include/ulg.h) in Python
integers: the reference of tests/test_gpu_linext.py.

  c(0) = 1,  c(S) = sum over v in S with Pa_v subset of S \\ v of c(S \\ v),  ext(G) = c(V)

c(S) is the number of orderings of S in which every member's parents come first: 0 when S is
not closed under parents, hence ext = 0 for a graph with a directed cycle.  A DAG is a list par
of n parent masks, par[v] = the parents of v.

count         the recursion, S in numeric order, Python integers throughout
count_many    the same for many DAGs of one n at once, in numpy uint64 (n <= 20: 20! < 2^63)
brute         all n! orders (n <= 8)
hook          n! / prod_v (size of v's subtree) for a rooted forest
"""
import itertools
import math

import numpy as np


def count(n, par):
    c = [0] * (1 << n)
    c[0] = 1
    for S in range(1, 1 << n):
        t, m = 0, S
        while m:
            b = m & -m
            if par[b.bit_length() - 1] & ~S == 0:
                t += c[S ^ b]
            m ^= b
        c[S] = t
    return c[-1]


def count_many(n, pars):
    """count for every row of pars (D, n) at once, in numpy uint64 (n <= 20: 20! < 2^63) -> uint64 (D)."""
    assert n <= 20
    pars = np.asarray(pars, dtype=np.uint64).astype(np.int64).reshape(-1, n)
    c = np.zeros((pars.shape[0], 1 << n), dtype=np.uint64)
    c[:, 0] = 1
    for S in range(1, 1 << n):
        for v in range(n):
            if (S >> v) & 1:
                c[:, S] += np.where(pars[:, v] & ~S == 0, c[:, S ^ (1 << v)], np.uint64(0))
    return c[:, -1].copy()


def brute(n, par):
    assert n <= 8
    total = 0
    for perm in itertools.permutations(range(n)):
        seen, ok = 0, True
        for v in perm:
            if par[v] & ~seen:
                ok = False
                break
            seen |= 1 << v
        total += ok
    return total


def random_dag(n, density, rng):
    """A DAG along a random order: each earlier variable is a parent with probability `density`."""
    order = rng.permutation(n)
    par = [0] * n
    for i, v in enumerate(order):
        for u in order[:i]:
            if rng.random() < density:
                par[int(v)] |= 1 << int(u)
    return par


def random_forest(n, rng, roots=0.2):
    """Every variable has at most one parent, earlier in a random order."""
    order = [int(v) for v in rng.permutation(n)]
    par = [0] * n
    for i, v in enumerate(order):
        if i and rng.random() >= roots:
            par[v] = 1 << order[int(rng.integers(0, i))]
    return par


def hook(n, par):
    """n! / prod_v |subtree of v| for a rooted forest (each par[v] has at most one bit)."""
    assert all(bin(p).count("1") <= 1 for p in par)
    size = [1] * n
    for v in range(n):  # v adds one to every ancestor
        u = v
        while par[u]:
            u = par[u].bit_length() - 1
            size[u] += 1
    q, rem = divmod(math.factorial(n), math.prod(size))
    assert rem == 0
    return q


def words(x):
    return x & ((1 << 64) - 1), x >> 64


def ulp_distance(a, b):
    """Doubles between a and b (both finite and of one sign, or equal)."""
    if a == b:
        return 0
    ia, ib = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return abs(int(ia) - int(ib))
