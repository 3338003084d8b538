"""ulg_dag_features' contract (include/ulg.h) restated on Python integers and sets.  No GPU, no
project binding, and none of the row formulas of csrc/dagfeat_dev.h: the closure is a search, the
blanket and the v-structures are their definitions, and the essential graph is Meek's rules R1-R3
on sets of neighbours.  essential() is in turn held to the definition of a compelled edge -- the
same direction in every DAG with the same skeleton and v-structures -- by class_compelled(), for
every DAG of n = 4 and n = 5 (tests/test_dagfeat_ref.py).

A DAG is a sequence par of n Python integers, par[v] = the parent mask of v."""
import functools
import itertools

import numpy as np

TABLES = ("edge", "ancestor", "blanket", "compelled")


def members(mask):
    out = []
    while mask:
        low = mask & -mask
        out.append(low.bit_length() - 1)
        mask ^= low
    return out


def ancestors(n, par):
    """anc[v] = the mask of the u with a directed path of at least one edge u ~> v, by search."""
    anc = []
    for v in range(n):
        seen, stack = 0, members(par[v])
        while stack:
            u = stack.pop()
            if not (seen >> u) & 1:
                seen |= 1 << u
                stack.extend(members(par[u]))
        anc.append(seen)
    return anc


def is_cyclic(n, par):
    return any((a >> v) & 1 for v, a in enumerate(ancestors(n, par)))


def children(n, par):
    return [sum(1 << v for v in range(n) if (par[v] >> u) & 1) for u in range(n)]


def blanket(n, par):
    ch = children(n, par)
    out = []
    for v in range(n):
        b = par[v] | ch[v]
        for c in members(ch[v]):
            b |= par[c]
        out.append(b & ~(1 << v))
    return out


def vstructs(n, par):
    """The triples (v, u, w), u < w: u -> v <- w with u, w not adjacent."""
    out = []
    for v in range(n):
        for u, w in itertools.combinations(members(par[v]), 2):
            if not ((par[u] >> w) & 1 or (par[w] >> u) & 1):
                out.append((v, u, w))
    return out


def skeleton(n, par):
    return frozenset(frozenset((u, v)) for v in range(n) for u in members(par[v]))


def essential(n, par):
    """D[v] = the mask of the compelled parents of v: the edges of the v-structures, closed under
    Meek's rules R1-R3 on sets (dp: compelled parents, dc: compelled children, un: undirected
    neighbours, adj: all neighbours)."""
    ch = children(n, par)
    adj = [set(members(par[v] | ch[v])) for v in range(n)]
    dp = [set() for _ in range(n)]
    dc = [set() for _ in range(n)]
    for v, u, w in vstructs(n, par):
        for x in (u, w):
            dp[v].add(x)
            dc[x].add(v)
    un = [adj[v] - dp[v] - dc[v] for v in range(n)]
    changed = True
    while changed:
        changed = False
        for c in range(n):
            for a in sorted(un[c]):
                r1 = any(x != c and x not in adj[c] for x in dp[a])
                r2 = bool(dc[a] & dp[c])
                r3 = any(k2 not in adj[k1] for k1, k2 in itertools.combinations(sorted(un[a] & dp[c]), 2))
                if r1 or r2 or r3:
                    assert (par[c] >> a) & 1, "a rule oriented an edge against the DAG"
                    dp[c].add(a)
                    dc[a].add(c)
                    un[c].discard(a)
                    un[a].discard(c)
                    changed = True
    return [sum(1 << u for u in dp[v]) for v in range(n)]


def all_assignments(n):
    """Every assignment of a parent mask without the own bit to each variable, as tuples."""
    per = [[sum(((i >> j) & 1) << u for j, u in enumerate([u for u in range(n) if u != v])) for i in range(1 << (n - 1))]
           for v in range(n)]
    return itertools.product(*per)


@functools.lru_cache(maxsize=None)
def all_dags(n):
    """Every DAG of n labelled variables (543 at n = 4, 29,281 at n = 5), as a tuple of tuples."""
    rows = np.array(list(all_assignments(n)), dtype=np.uint64)  # 2^(n (n-1)) of them: sifted by a Warshall pass on columns
    anc, one = rows.copy(), np.uint64(1)
    for k in range(n):
        anc |= ((anc >> np.uint64(k)) & one) * anc[:, k:k + 1]
    cyclic = np.zeros(len(rows), dtype=bool)
    for v in range(n):
        cyclic |= ((anc[:, v] >> np.uint64(v)) & one).astype(bool)
    return tuple(tuple(int(x) for x in row) for row in rows[~cyclic])


@functools.lru_cache(maxsize=None)
def class_compelled(n):
    """The definition, by enumeration: ({DAG: D}, number of classes).  Two DAGs are equivalent iff they
    have the same skeleton and v-structures; u -> v of G is compelled iff every member of G's class has it."""
    classes = {}
    for p in all_dags(n):
        classes.setdefault((skeleton(n, p), frozenset(vstructs(n, p))), []).append(p)
    out = {}
    for group in classes.values():
        common = [functools.reduce(lambda x, y: x & y, (p[v] for p in group)) for v in range(n)]
        for p in group:
            out[p] = common
    return out, len(classes)


def features(n, dags, weight=None):
    """-> dict: edge, ancestor, blanket, compelled uint64 (n, n), vstruct uint64 (n, n, n), total and cyclic
    Python ints: the sums of ulg_dag_features over the acyclic graphs of `dags`, in Python integers."""
    tabs = {name: [[0] * n for _ in range(n)] for name in TABLES}
    vs = {}
    total = cyclic = 0
    for k, par in enumerate(dags):
        par = [int(x) for x in par]
        q = 1 if weight is None else int(weight[k])
        anc = ancestors(n, par)
        if any((a >> v) & 1 for v, a in enumerate(anc)):
            cyclic += 1
            continue
        total += q
        for name, rows in (("edge", par), ("ancestor", anc), ("blanket", blanket(n, par)), ("compelled", essential(n, par))):
            t = tabs[name]
            for v in range(n):
                for u in members(rows[v]):
                    t[u][v] += q
        for key in vstructs(n, par):
            vs[key] = vs.get(key, 0) + q
    out = {name: np.array(t, dtype=np.uint64).reshape(n, n) for name, t in tabs.items()}
    out["vstruct"] = np.zeros((n, n, n), dtype=np.uint64)
    for key, x in vs.items():
        out["vstruct"][key] = x
    out["total"], out["cyclic"] = total, cyclic
    return out


def random_dag(n, kind, rng):
    """'sparse': at most 2 parents each; 'dense': each earlier variable of a random order is a parent with
    probability 1/2.  The order is random, so parents are not the lower-numbered variables."""
    order = [int(x) for x in rng.permutation(n)]
    par = [0] * n
    for i, v in enumerate(order):
        if kind == "sparse":
            for u in rng.choice(order[:i], size=min(i, int(rng.integers(0, 3))), replace=False) if i else []:
                par[v] |= 1 << int(u)
        else:
            for u in order[:i]:
                if rng.random() < 0.5:
                    par[v] |= 1 << u
    return par


def chain(n):
    return [0] + [1 << (v - 1) for v in range(1, n)]


def collider_chain(n):
    """0 -> 2 <- 1, 2 -> 3 -> ... -> n-1"""
    return [0, 0, 0b11] + [1 << (v - 1) for v in range(3, n)]


def complete(n):
    return [(1 << v) - 1 for v in range(n)]


def star(n):
    """every other variable a parent of n - 1"""
    return [0] * (n - 1) + [(1 << (n - 1)) - 1]


def cycle(n):
    return [1 << ((v - 1) % n) for v in range(n)]
