"""Plain numpy reference of the GPU order-graph sweep (csrc/search_gpu.hip).

No GPU, no project binding: parent-set lists in, every node's cost and argmin
out, bit for bit what the sweep's contract says.

    g(empty) = 0
    g(T)     = min over the elements a_0 < a_1 < ... of T, j ascending, first
               strict minimum, of fl32(g(T \\ a_j) + bs(a_j, T \\ a_j))
               over predecessors P = T \\ a_j that are reached and, with a
               skeleton, allowed: P is empty or meets rows[a_j]
    leaf(T)  = that j (255 and g = FLT_MAX if no predecessor qualifies)
    expanded = components + reached nodes of layers 1 .. m-1 of each

bs(v, P) is the cost of the first stored set of v, in (cost, file order),
that is a subset of P; -0 folds onto +0 in that order (ordkey).

A component's nodes are the subsets of its m variables as m-bit masks over
the variables in ascending order ("compact" masks).  The kernels store a
layer's nodes in colex rank; among sets of one size colex order is the
numeric order of the masks, which is how layer_nodes() produces it -- without
the binomial sums the kernels rank with (test_sweep_ref.py ties the two).
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
UNREACHED = 255
UNREACHED_KEY = 0xFFFFFFFFFF
_NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def ordkey(f):
    """float32 -> uint32 whose unsigned order is the float order, -0 onto +0."""
    f = np.array(f, dtype=np.float32, ndmin=1)
    f[f == 0] = np.float32(0.0)
    u = f.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ord_cost(k):
    """Inverse of ordkey."""
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def popcounts(m):
    """popcount of every m-bit mask."""
    pc = np.zeros(1 << m, dtype=np.int64)
    for b in range(m):
        pc[1 << b:2 << b] = pc[:1 << b] + 1
    return pc


def layer_nodes(m):
    """Per layer d = 0..m: the compact masks of size d in colex (= numeric) order."""
    pc = popcounts(m)
    order = np.argsort(pc, kind="stable")  # ascending masks within a popcount
    bounds = np.concatenate([[0], np.cumsum(np.bincount(pc, minlength=m + 1))])
    return [order[bounds[d]:bounds[d + 1]] for d in range(m + 1)]


def global_masks(m, comp_vars):
    """Compact mask -> mask over the variables (uint64)."""
    g = np.zeros(1 << m, dtype=np.uint64)
    for b in range(m):
        g[1 << b:2 << b] = g[:1 << b] | np.uint64(1 << int(comp_vars[b]))
    return g


def bs_tables(n, offsets, sets, costs, comp_vars):
    """bs(v, P) for every variable v of the component and every compact P.

    Returns (cost, parents): float32 [m, 2^m] (FLT_MAX where no stored set
    fits) and uint64 [m, 2^m], the winning stored set as a mask over the
    variables (0 where none).  Stored sets with a parent outside the
    component never fit a P inside it and are ignored.  Entries whose P
    contains v are filled like the others; the sweep never reads them."""
    m = len(comp_vars)
    offsets = np.asarray(offsets, dtype=np.int64)
    sets = np.asarray(sets, dtype=np.uint64)
    costs = np.asarray(costs, dtype=np.float32)
    comp = 0
    for v in comp_vars:
        comp |= 1 << int(v)
    cost = np.empty((m, 1 << m), dtype=np.float32)
    par = np.zeros((m, 1 << m), dtype=np.uint64)
    for j, v in enumerate(comp_vars):
        b, e = int(offsets[v]), int(offsets[v + 1])
        s = sets[b:e]
        inside = (s & np.uint64(~comp & 0xFFFFFFFFFFFFFFFF)) == 0
        idx = np.nonzero(inside)[0]
        compact = np.zeros(len(idx), dtype=np.int64)
        for bit, var in enumerate(comp_vars):
            compact |= ((s[idx] >> np.uint64(int(var))) & np.uint64(1)).astype(np.int64) << bit
        key = (ordkey(costs[b:e][idx]).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
        t = np.full(1 << m, _NOKEY, dtype=np.uint64)
        np.minimum.at(t, compact, key)
        for bit in range(m):  # subset minimum: fold every mask's bit-cleared twin into it
            v3 = t.reshape(-1, 2, 1 << bit)
            np.minimum(v3[:, 1, :], v3[:, 0, :], out=v3[:, 1, :])
        none = t == _NOKEY
        cost[j] = ord_cost((t >> np.uint64(32)).astype(np.uint32))
        cost[j][none] = FLT_MAX
        win = (t & np.uint64(0xFFFFFFFF)).astype(np.int64)
        win[none] = 0
        par[j] = s[win] if len(s) else 0
        par[j][none] = 0
    return cost, par


def sweep(m, comp_vars, bs, rows=None, near_rel=None):
    """The layer DP in float32.  bs = bs_tables(...)'s pair; rows (optional)
    = skeleton rows indexed by variable: leaf v may follow P only if P is
    empty or P & rows[v] != 0 (the test layer_pull_kernel<false> applies per
    predecessor, astar_main.cpp:305-313).

    Returns a dict:
      g        float32 [2^m] by compact mask (FLT_MAX = unreached)
      leafpos  uint8   [2^m] by compact mask (255 = unreached; node 0: 255)
      leaves   uint8   [2^m] in the kernels' (layer, colex rank) order
      layers   layer_nodes(m)
      nmin     uint8   [2^m] by compact mask: how many qualifying leaves attain the minimum
      reached  reached nodes in layers 1 .. m-1
      chain    compact bit added at each step from the root (None: no goal)
      order    the variables in that order (None: no goal)
      parents  {variable: parent set bs returns for its prefix} (None: no goal)
      cost     g(goal)
      near     (only with near_rel) per layer 0..m, the number of nodes with
               two qualifying candidates that differ in their bits but by at
               most near_rel relative -- what a relative tolerance cannot see
    """
    cost_t, par_t = bs
    layers = layer_nodes(m)
    g = np.full(1 << m, FLT_MAX, dtype=np.float32)
    leafpos = np.full(1 << m, UNREACHED, dtype=np.uint8)
    nmin = np.zeros(1 << m, dtype=np.uint8)
    g[0] = np.float32(0.0)
    glob = global_masks(m, comp_vars) if rows is not None else None
    near = [0] * (m + 1)
    for d in range(1, m + 1):
        T = layers[d]
        allc = np.full((len(T), m), np.inf, dtype=np.float32) if near_rel is not None else None
        best = np.full(len(T), FLT_MAX, dtype=np.float32)
        bestj = np.full(len(T), UNREACHED, dtype=np.uint8)
        cnt = np.zeros(len(T), dtype=np.uint8)
        for b in range(m):  # ascending bit = ascending position j within every T
            has = ((T >> b) & 1) == 1
            Tb = T[has]
            P = Tb ^ (1 << b)
            gp = g[P]
            ok = gp < FLT_MAX
            if rows is not None:
                ok &= (P == 0) | ((glob[P] & np.uint64(int(rows[int(comp_vars[b])]))) != 0)
            cand = (gp + cost_t[b][P]).astype(np.float32)
            cur_best, cur_j = best[has], bestj[has]
            take = ok & ((cur_j == UNREACHED) | (cand < cur_best))
            j = popcounts_below(Tb, b)
            cur_cnt = cnt[has]
            cur_cnt[ok & ~take & (cand == cur_best)] += 1
            cur_cnt[take] = 1
            cur_best[take] = cand[take]
            cur_j[take] = j[take]
            best[has], bestj[has], cnt[has] = cur_best, cur_j, cur_cnt
            if allc is not None:
                allc[has, b] = np.where(ok, cand, np.float32(np.inf))
        if allc is not None and d >= 2:
            allc.sort(axis=1)
            lo, hi = allc[:, :-1].astype(np.float64), allc[:, 1:].astype(np.float64)
            with np.errstate(invalid="ignore"):
                close = np.isfinite(hi) & (hi != lo) & (hi - lo <= near_rel * np.abs(lo))
            near[d] = int(close.any(axis=1).sum())
        hit = bestj != UNREACHED
        g[T] = np.where(hit, best, FLT_MAX)
        leafpos[T] = bestj
        nmin[T] = cnt
    reached = int(sum(int((leafpos[layers[d]] != UNREACHED).sum()) for d in range(1, m)))
    out = {"g": g, "leafpos": leafpos, "nmin": nmin, "leaves": leafpos[np.concatenate(layers)], "layers": layers,
           "reached": reached, "cost": g[(1 << m) - 1], "chain": None, "order": None, "parents": None, "near": near}
    T = (1 << m) - 1
    chain = [0] * m
    for d in range(m, 0, -1):
        j = int(leafpos[T])
        if j == UNREACHED:
            return out
        bit = [b for b in range(m) if (T >> b) & 1][j]
        chain[d - 1] = bit
        T ^= 1 << bit
    out["chain"] = chain
    out["order"] = [int(comp_vars[b]) for b in chain]
    parents, P = {}, 0
    for b in chain:
        parents[int(comp_vars[b])] = int(par_t[b][P])
        P |= 1 << b
    out["parents"] = parents
    return out


def popcounts_below(T, b):
    """Number of set bits of each mask in T below bit b (the position of b in T)."""
    low = T & ((1 << b) - 1)
    j = np.zeros(len(T), dtype=np.uint8)
    for q in range(b):
        j += ((low >> q) & 1).astype(np.uint8)
    return j


def shard_keys(res):
    """Per layer 1..m (index 0 unused: None) the all-reduced keys
    ulg_sweep_shard_layer's contract gives: (ordkey(g) << 8) | j, or
    0xFFFFFFFFFF where the node is unreached (include/ulg.h)."""
    keys = [None]
    for T in res["layers"][1:]:
        j = res["leafpos"][T].astype(np.uint64)
        k = (ordkey(res["g"][T]).astype(np.uint64) << np.uint64(8)) | j
        keys.append(np.where(j == UNREACHED, np.uint64(UNREACHED_KEY), k))
    return keys


def make_lists(n, pools, rng, nsets, cost, empty_cost=None, sizes=(1, 3), cover=False):
    """Synthetic parent-set lists for ulg_search_load: per variable the empty
    set first, then (cover) every single parent of pools[v], then up to
    `nsets` distinct random sets of sizes[0]..sizes[1] parents drawn from
    pools[v] (duplicates dropped, as a merged .pss has none).  cost(rng, k)
    returns k float32 costs; empty_cost likewise for the empty sets.
    Returns (offsets, sets, costs)."""
    offsets, sets, costs = [0], [], []
    for v in range(n):
        pool = [int(p) for p in pools[v] if p != v]
        mine = [0]
        if cover:
            mine += [1 << p for p in pool]
        if pool:
            for _ in range(nsets):
                k = int(rng.integers(sizes[0], min(sizes[1], len(pool)) + 1)) if len(pool) >= sizes[0] else len(pool)
                s = 0
                for p in rng.choice(len(pool), size=k, replace=False):
                    s |= 1 << pool[int(p)]
                if s not in mine:
                    mine.append(s)
        c = np.asarray(cost(rng, len(mine)), dtype=np.float32)
        if empty_cost is not None:
            c[0] = np.float32(empty_cost(rng, 1)[0])
        sets += mine
        costs.append(c)
        offsets.append(len(sets))
    return (np.asarray(offsets, dtype=np.int64), np.asarray(sets, dtype=np.uint64),
            np.concatenate(costs).astype(np.float32))


def float_costs(rng, k):
    """Costs with fractional digits at a C2-like magnitude."""
    return (rng.random(k) * 4000.0 + 1000.0).astype(np.float32)


def components(rows, n):
    """The skeleton's components in the order the search takes them (by
    lowest variable; row i's set bits are followed from i, as given)."""
    seen, comps = 0, []
    for v in range(n):
        if (seen >> v) & 1:
            continue
        comp, stack = 1 << v, [v]
        seen |= comp
        while stack:
            cur = stack.pop()
            for i in range(n):
                if not (seen >> i) & 1 and (int(rows[cur]) >> i) & 1:
                    seen |= 1 << i
                    comp |= 1 << i
                    stack.append(i)
        comps.append([i for i in range(n) if (comp >> i) & 1])
    return comps


_memo = {}


def search(n, offsets, sets, costs, rows=None, near_rel=None):
    """The whole GPU-mode search: every component swept in the search's order,
    the filter applied to every component (on a component the skeleton is
    complete on it filters nothing, which is why the kernels skip it there).
    Returns (per-component sweep results, expanded).  Results are computed
    once per input and shared: callers must not modify them."""
    import hashlib
    h = hashlib.sha256()
    for a in (np.asarray(offsets, dtype=np.int64), np.asarray(sets, dtype=np.uint64),
              np.asarray(costs, dtype=np.float32)):
        h.update(a.tobytes())
    key = (n, h.hexdigest(), None if rows is None else tuple(int(r) for r in rows), near_rel)
    if key not in _memo:
        comps = components(rows, n) if rows is not None else [list(range(n))]
        res = [sweep(len(cv), cv, bs_tables(n, offsets, sets, costs, cv), rows, near_rel) for cv in comps]
        for r in res:
            for a in (r["g"], r["leafpos"], r["leaves"]):
                a.setflags(write=False)
        _memo[key] = (res, len(comps) + sum(r["reached"] for r in res))
    return _memo[key]
