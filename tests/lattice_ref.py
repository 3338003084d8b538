"""The best-score lattice and the static pattern database, restated in plain
Python / numpy: the reference the device-built tables are held to, entry by
entry (test_gpu_lattice_exact.py).  No HIP and no oracle in here; the module
is itself checked against brute force and the C oracle in test_lattice_ref.py.

The contract

Lattice.  Variable v has a list of stored parent sets in file order, each with
a float32 cost.  best(v, S) stable-sorts the list by cost -- the IEEE compare,
so -0 == +0, and file order breaks ties (SparseParentList with the pinned N7
tie rule) -- and returns the first set that is a subset of S as (cost,
parents), or (FLT_MAX, 0) if there is none.  table(v, scope) is the dense
form: D_v = the union of v's stored sets inside scope (the empty set for v
outside scope), and for every S inside D_v, in pext(S, D_v) order, the best
stored subset of S among the stored sets inside D_v.

Pattern database.  pdb(pd_count, ancestors, scc) forms the groups as
consecutive scc variables, ceil(float(|scc|) / pd_count) each (trailing groups
may be empty).  Per group, pd[R] for every R inside the group comes from the
reverse BFS of static_pattern_database.cpp:176-247 in float32: a layer's
keys are visited in ascending R, each key's leaves in ascending index, the
leaf's score is best(leaf, (scc \\ (R \\ leaf)) | ancestors), newG = score +
pd[R \\ leaf], and newG replaces the stored value iff oldG == 0 or newG < oldG.
(That rule makes the value depend on the visiting order once a partial sum is
exactly 0; the reference iterates an unordered_map, so the order is pinned
here as the C oracle pins it.)  h(S) and `complete` are :145-174.

Limits of the contract
  * costs are any float32 except NaN;
  * duplicate sets within a variable are already merged;
  * values are compared as bit patterns after mapping -0.0 to +0.0 on both
    sides (same_bits / fold_zero): the reference's compare cannot tell the
    zeros apart and no search result depends on the sign.
"""
import math

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
_U64_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
_U32_NONE = np.uint32(0xFFFFFFFF)


# ---- order key -----------------------------------------------------------------
def order_key(costs):
    """float32 -> uint32 whose unsigned order is the IEEE order of the floats,
    with -0 folded onto +0.  IEEE binary32 is sign-magnitude: among non-negative
    values the bit pattern grows with the value, among negative ones it falls,
    so non-negative patterns get the top bit set and negative ones are
    complemented.  No NaN.  0xFFFFFFFF is free (it would be the NaN 0x7FFFFFFF)
    and stands for 'no entry'."""
    c = np.ascontiguousarray(costs, dtype=np.float32)
    assert not np.isnan(c).any(), "the contract excludes NaN costs"
    u = c.view(np.uint32).copy()
    u[c == 0] = 0
    neg = (u >> np.uint32(31)) == 1
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_cost(keys):
    """Inverse of order_key; 'no entry' reads as FLT_MAX."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    top = (k >> np.uint32(31)) == 1
    u = np.where(top, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    out = u.view(np.float32).copy()
    out[k == _U32_NONE] = FLT_MAX
    return out


def fold_zero(a):
    """Bit patterns of float32 values with -0.0 mapped to +0.0."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    return u


def same_bits(a, b):
    return np.array_equal(fold_zero(a), fold_zero(b))


# ---- bit helpers ---------------------------------------------------------------
def bits_of(mask):
    return [b for b in range(64) if (int(mask) >> b) & 1]


def pext(x, mask):
    """Vectorised pext: the bits of x at the set positions of mask, packed."""
    x = np.asarray(x, dtype=np.uint64)
    r = np.zeros(x.shape, dtype=np.uint64)
    for k, b in enumerate(bits_of(mask)):
        r |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(k)
    return r


def pdep(r, mask):
    r = np.asarray(r, dtype=np.uint64)
    x = np.zeros(r.shape, dtype=np.uint64)
    for k, b in enumerate(bits_of(mask)):
        x |= ((r >> np.uint64(k)) & np.uint64(1)) << np.uint64(b)
    return x


def _subset_min(arr, m):
    """In place: arr[S] = min over T subset of S of arr[T] (S, T as m-bit indices)."""
    for b in range(m):
        a = arr.reshape(-1, 2, 1 << b)
        np.minimum(a[:, 1, :], a[:, 0, :], out=a[:, 1, :])
    return arr


class Lattice:
    """Parent-set lists (offsets[n+1], sets, costs in file order) and the
    reference answers over them."""

    def __init__(self, n, offsets, sets, costs):
        self.n = int(n)
        self.offs = np.ascontiguousarray(offsets, dtype=np.int64)
        self.sets = np.ascontiguousarray(sets, dtype=np.uint64)
        self.costs = np.ascontiguousarray(costs, dtype=np.float32)
        assert not np.isnan(self.costs).any()
        self.all = (1 << self.n) - 1
        self._sorted = {}
        self._tables = {}
        self._bs = {}
        self.pd_count = 0

    def list_of(self, v):
        return self.sets[self.offs[v]:self.offs[v + 1]], self.costs[self.offs[v]:self.offs[v + 1]]

    # ---- best ------------------------------------------------------------------
    def _sorted_list(self, v):
        if v not in self._sorted:
            s, c = self.list_of(v)
            # a stable sort of the floats themselves: numpy orders with <, under
            # which -0 and +0 are equal, so file order decides between them
            order = np.argsort(c, kind="stable")
            self._sorted[v] = (s[order], c[order])
        return self._sorted[v]

    def best(self, v, S):
        s, c = self._sorted_list(v)
        hit = np.nonzero((s & ~np.uint64(S)) == 0)[0]
        if hit.size == 0:
            return FLT_MAX, 0
        return c[hit[0]], int(s[hit[0]])

    def best_many(self, vs, Ss):
        """best for arrays of (v, S): (float32 costs, uint64 parents)."""
        vs = np.asarray(vs, dtype=np.int64)
        Ss = np.asarray(Ss, dtype=np.uint64)
        costs = np.full(len(vs), FLT_MAX, dtype=np.float32)
        par = np.zeros(len(vs), dtype=np.uint64)
        for v in np.unique(vs):
            s, c = self._sorted_list(int(v))
            q = np.nonzero(vs == v)[0]
            if s.size == 0:
                continue
            for lo in range(0, len(q), 4096):
                qi = q[lo:lo + 4096]
                fit = (s[None, :] & ~Ss[qi][:, None]) == 0
                first = fit.argmax(axis=1)
                ok = fit[np.arange(len(qi)), first]
                costs[qi[ok]] = c[first[ok]]
                par[qi[ok]] = s[first[ok]]
        return costs, par

    # ---- table -----------------------------------------------------------------
    def support(self, v, scope=None):
        scope = self.all if scope is None else int(scope)
        if not (scope >> v) & 1:
            return 0
        s, _ = self.list_of(v)
        inside = s[(s & ~np.uint64(scope)) == 0]
        return int(np.bitwise_or.reduce(inside)) if inside.size else 0

    def table(self, v, scope=None, cost_only=None):
        """(D_v, float32 costs[2^m], uint64 parents[2^m] or None): the dense
        table over the subsets of D_v in pext(S, D_v) order.  The uint64 form
        carries (order key << 32 | file index) through the subset-min, which
        gives the set behind each cost as well; cost_only (the default for
        m > 20) runs it over the uint32 order keys alone."""
        D = self.support(v, scope)
        m = bin(D).count("1")
        if cost_only is None:
            cost_only = m > 20
        s, c = self.list_of(v)
        keep = np.nonzero((s & ~np.uint64(D)) == 0)[0]
        idx = pext(s[keep], D).astype(np.int64)
        key = order_key(c[keep])
        if cost_only:
            arr = np.full(1 << m, _U32_NONE, dtype=np.uint32)
            np.minimum.at(arr, idx, key)
            _subset_min(arr, m)
            return D, key_cost(arr), None
        arr = np.full(1 << m, _U64_NONE, dtype=np.uint64)
        np.minimum.at(arr, idx, (key.astype(np.uint64) << np.uint64(32)) | keep.astype(np.uint64))
        _subset_min(arr, m)
        none = arr == _U64_NONE
        costs = key_cost(np.where(none, _U32_NONE, (arr >> np.uint64(32)).astype(np.uint32)))
        fi = (arr & np.uint64(0xFFFFFFFF)).astype(np.int64)
        par = np.where(none, np.uint64(0), s[np.where(none, 0, fi)] if s.size else np.uint64(0)).astype(np.uint64)
        return D, costs, par

    def _cost_lookup(self, v, Ss):
        """best(v, S).cost for an array of S through the (cached) full table
        where that is small, else by the list scan."""
        D = self.support(v)
        if bin(D).count("1") > 20:
            return self.best_many(np.full(len(Ss), v), Ss)[0]
        if v not in self._tables:
            self._tables[v] = self.table(v)[1]
        return self._tables[v][pext(np.asarray(Ss, dtype=np.uint64) & np.uint64(D), D).astype(np.int64)]

    # ---- pattern database --------------------------------------------------------
    @staticmethod
    def groups_of(pd_count, scc):
        var = bits_of(scc)
        size = int(math.ceil(np.float32(len(var)) / np.float32(pd_count)))
        groups = []
        for g in range(pd_count):
            grp = 0
            for b in var[g * size:(g + 1) * size]:
                grp |= 1 << b
            groups.append(grp)
        return groups

    def _leaf_scores(self, grp, ancestors, scc):
        """bs[R, j] = best(leaf_j, (scc \\ (R \\ leaf_j)) | ancestors).cost for leaf_j in R."""
        memo = (int(grp), int(ancestors), int(scc))
        if memo in self._bs:
            return self._bs[memo]
        pos = bits_of(grp)
        s = len(pos)
        R = pdep(np.arange(1 << s, dtype=np.uint64), grp)
        bs = np.zeros((1 << s, s), dtype=np.float32)
        for j, leaf in enumerate(pos):
            removed = R & ~np.uint64(1 << leaf)
            choices = (np.uint64(scc) & ~removed) | np.uint64(ancestors)
            bs[:, j] = self._cost_lookup(leaf, choices)
        self._bs = {memo: bs}  # the last group's only: 2^s x s floats
        return bs

    def pdb_group_bfs(self, grp, ancestors, scc):
        """pd[R] (pext(R, grp) order) by the reverse BFS as written: layer by
        layer, keys in ascending R, leaves in ascending index."""
        pos = bits_of(grp)
        s = len(pos)
        bs = self._leaf_scores(grp, ancestors, scc)
        pd = np.zeros(1 << s, dtype=np.float32)
        prev = {0: np.float32(0)}
        with np.errstate(over="ignore", invalid="ignore"):
            for _layer in range(s + 1):
                cur = {}
                for r in sorted(prev):
                    value = prev[r]
                    for j in range(s):
                        if (r >> j) & 1:
                            continue  # leaf j is no longer in the subnetwork
                        nr = r | (1 << j)
                        newG = np.float32(bs[nr, j] + value)
                        oldG = cur.get(nr, np.float32(0))
                        cur[nr] = newG if (oldG == 0 or newG < oldG) else oldG
                    pd[r] = value
                prev = cur
        return pd

    def pdb_group_fold(self, grp, ancestors, scc):
        """The same values, a layer at a time: a target R receives its
        candidates from the keys R \\ leaf in ascending order, i.e. from its
        leaves in descending index, so the keep rule is folded over the
        leaves from the highest down, for every R of the layer at once."""
        pos = bits_of(grp)
        s = len(pos)
        bs = self._leaf_scores(grp, ancestors, scc)
        pd = np.zeros(1 << s, dtype=np.float32)
        idx = np.arange(1 << s, dtype=np.int64)
        layer_of = np.zeros(1 << s, dtype=np.int64)
        for j in range(s):
            layer_of += (idx >> j) & 1
        with np.errstate(over="ignore", invalid="ignore"):
            for layer in range(1, s + 1):
                R = idx[layer_of == layer]
                cur = np.zeros(len(R), dtype=np.float32)
                for j in range(s - 1, -1, -1):
                    has = ((R >> j) & 1) == 1
                    newG = (bs[R, j] + pd[R ^ (1 << j)]).astype(np.float32)
                    take = has & ((cur == 0) | (newG < cur))
                    cur = np.where(take, newG, cur)
                pd[R] = cur
        return pd

    def pdb(self, pd_count, ancestors=0, scc=None, bfs_up_to=8):
        """Builds the groups and their tables; self.groups, self.pd[g]."""
        scc = self.all if scc is None else int(scc)
        assert pd_count >= 1 and not (ancestors & scc)
        self.pd_count, self.ancestors, self.scc = pd_count, int(ancestors), scc
        self.groups = self.groups_of(pd_count, scc)
        self.pd = []
        for grp in self.groups:
            small = bin(grp).count("1") <= bfs_up_to
            self.pd.append((self.pdb_group_bfs if small else self.pdb_group_fold)(grp, ancestors, scc))
        return self.groups, self.pd

    def h(self, S):
        """(h, complete) of StaticPatternDatabase::h."""
        remaining = ~int(S) & self.all
        h = np.float32(0)
        with np.errstate(over="ignore", invalid="ignore"):
            for grp, pd in zip(self.groups, self.pd):
                vs = grp & remaining
                val = pd[int(pext(np.uint64(vs), grp))]
                if vs == remaining:
                    return val, 1
                h = np.float32(h + val)
        return h, 0

    def h_many(self, Ss):
        """h for an array of S: (float32 h, int32 complete)."""
        Ss = np.asarray(Ss, dtype=np.uint64)
        remaining = ~Ss & np.uint64(self.all)
        h = np.zeros(len(Ss), dtype=np.float32)
        comp = np.zeros(len(Ss), dtype=np.int32)
        with np.errstate(over="ignore", invalid="ignore"):
            for grp, pd in zip(self.groups, self.pd):
                vs = remaining & np.uint64(grp)
                val = pd[pext(vs, grp).astype(np.int64)]
                hit = (comp == 0) & (vs == remaining)
                h = np.where(comp == 1, h, np.where(hit, val, (h + val).astype(np.float32)))
                comp[hit] = 1
        return h, comp

    def zero_sum_share(self):
        """Share of the candidate sums newG of the last pdb() that are exactly 0."""
        zero = total = 0
        with np.errstate(over="ignore", invalid="ignore"):
            for grp, pd in zip(self.groups, self.pd):
                s = bin(grp).count("1")
                if s == 0:
                    continue
                bs = self._leaf_scores(grp, self.ancestors, self.scc)
                R = np.arange(1 << s, dtype=np.int64)
                for j in range(s):
                    has = ((R >> j) & 1) == 1
                    newG = (bs[R, j] + pd[R ^ (1 << j)])[has]
                    zero += int((newG == 0).sum())
                    total += int(has.sum())
        return zero / max(total, 1)


# ---- case generator ------------------------------------------------------------
def _costs_of(kind, count, rng, span=(-3, 3)):
    if kind == "ints":
        c = rng.integers(span[0], span[1] + 1, count).astype(np.float32)
        flip = (c == 0) & (rng.random(count) < 0.5)
        c[flip] = np.float32(-0.0)
        return c
    if kind == "wide":
        u = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
        nan = ((u >> np.uint32(23)) & np.uint32(0xFF) == 0xFF) & ((u & np.uint32(0x7FFFFF)) != 0)
        u[nan] &= np.uint32(0xFF800000)  # a NaN pattern becomes the infinity of its sign
        special = np.array([0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x00000002,
                            0x00000000, 0x80000000], dtype=np.uint32)
        k = min(count, len(special))
        if k:
            u[rng.choice(count, k, replace=False)] = special[:k]
        return u.view(np.float32).copy()
    if kind == "real":
        x = 200.0 + 300.0 * rng.random(count) + rng.normal(0.0, 1.0, count)
        return np.array([float("%f" % float(np.float32(v))) for v in x], dtype=np.float32)
    raise ValueError(kind)


def make_lists(n, specs, seed, kind=None):
    """Synthetic lists for ulg_search_load.  specs[v] is None (an empty list)
    or a dict: support (mask of candidate parents, v excluded), count (random
    sets), max_size (largest random set), kind ('ints' | 'wide' | 'real';
    the `kind` argument overrides it), span (range of the 'ints' costs,
    default (-3, 3)), empty (store the empty set; default
    True), crafted (default True; 'span' = D_v alone), dense (default True)
    and must (parents that every stored set holds, the empty set included).  With crafted,
    these sets are added where they exist: D_v itself, the lowest and the
    highest singleton, and for m > 14 the sets at table index t * 2^14 and
    t * 2^14 + 16383 for the first, one middle and the last tile t; with dense
    and m >= 14, 1500 sets that fall into one (the middle) tile.  The random
    sets alone need not span the support: D_v itself pins it.  File order is
    shuffled.  Returns (offsets, sets, costs, crafted) with crafted[v] the
    crafted sets of v (queries are aimed at them)."""
    rng = np.random.default_rng(seed)
    offs = [0]
    all_sets, all_costs, crafted = [], [], []
    for v in range(n):
        sp = specs[v] if v < len(specs) else None
        if sp is None:
            offs.append(offs[-1])
            crafted.append([])
            continue
        D = int(sp["support"])
        assert not (D >> v) & 1 and D >> n == 0
        pos = bits_of(D)
        m = len(pos)
        idx = set()
        if sp.get("empty", True):
            idx.add(0)
        cnt, k = int(sp.get("count", 0)), min(int(sp.get("max_size", 3)), m)
        if cnt and m:
            size = rng.integers(1, k + 1, cnt)
            pick = np.argsort(rng.random((cnt, m)), axis=1)[:, :k]
            for i in range(cnt):
                idx.add(sum(1 << int(b) for b in pick[i, :size[i]]))
        mine = []
        if sp.get("crafted", True) == "span" and m:
            mine += [(1 << m) - 1]  # D_v alone: nothing else pins the support
        elif sp.get("crafted", True) and m:
            mine += [(1 << m) - 1, 1, 1 << (m - 1)]
            if m > 14:
                tiles = 1 << (m - 14)
                for t in sorted({0, tiles // 2, tiles - 1}):
                    mine += [x for x in (t << 14, (t << 14) + 16383) if x]
        if sp.get("dense", True) and m >= 14:
            t = (1 << (m - 14)) // 2
            mine += [(t << 14) + int(r) for r in rng.choice(1 << 14, 1500, replace=False) if (t << 14) + int(r)]
        idx.update(mine)
        if sp.get("must"):  # every stored set holds these parents
            mm = int(pext(np.uint64(sp["must"]), D))
            idx, mine = {i | mm for i in idx}, [i | mm for i in mine]
        idx = np.array(sorted(idx), dtype=np.uint64)
        rng.shuffle(idx)
        all_sets.append(pdep(idx, D))
        all_costs.append(_costs_of(kind or sp.get("kind", "ints"), len(idx), rng, sp.get("span", (-3, 3))))
        crafted.append([int(x) for x in pdep(np.array(sorted(set(mine)), dtype=np.uint64), D)])
        offs.append(offs[-1] + len(idx))
    sets = np.concatenate(all_sets) if all_sets else np.zeros(0, dtype=np.uint64)
    costs = np.concatenate(all_costs) if all_costs else np.zeros(0, dtype=np.float32)
    return np.array(offs, dtype=np.int64), sets.astype(np.uint64), costs.astype(np.float32), crafted


def queries(n, lat, crafted, count, seed, only=None):
    """(variable, S) pairs: every pair when n <= 12, else `count` random ones
    (over the variables `only`, default all); plus, per variable, every
    crafted set, its complement inside D_v, 0 and the all-ones mask."""
    rng = np.random.default_rng(seed)
    allm = (1 << n) - 1
    if n <= 12:
        vs = np.repeat(np.arange(n), 1 << n)
        Ss = np.tile(np.arange(1 << n, dtype=np.uint64), n)
    else:
        vs = rng.integers(0, n, count) if only is None else rng.choice(np.asarray(only), count)
        Ss = rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, count, dtype=np.uint64)
        Ss &= np.uint64(allm)
        # half of them inside the variable's support, where the answers vary
        sup = np.array([lat.support(v) for v in range(n)], dtype=np.uint64)
        inside = rng.random(count) < 0.5
        Ss[inside] &= sup[vs[inside]]
    ev, es = [], []
    for v in range(n):
        D = lat.support(v)
        for c in crafted[v]:
            ev += [v, v]
            es += [c, D & ~c]
        ev += [v, v]
        es += [0, allm]
    return (np.concatenate([vs, np.array(ev, dtype=np.int64)]).astype(np.int32),
            np.concatenate([Ss, np.array(es, dtype=np.uint64)]).astype(np.uint64))


# 'ints' cost ranges of the PDB cases, by position in the component: mostly
# non-negative (best cost 0 more often than not) with every sixth variable
# reaching -1, so that many partial sums are exactly 0 and others lie on
# either side of it -- the inputs on which the keep rule depends on the order
PDB_SPANS = [(0, 2), (0, 1), (0, 3), (0, 2), (0, 1), (-1, 2)]


def pdb_lists(n, kind, seed, no_empty=None, at=None, count=3, must=None, N=None):
    """Lists for a PDB case: n variables, each with every other one as a
    candidate parent, the empty set and `count` random sets of up to 3
    parents each -- few enough that the best cost moves with the parents on
    offer.  must = a parent (position) that every set of the no_empty
    variables holds: outside scc | ancestors it leaves them no admissible set.  `at` places
    them at these bit positions of an N-variable problem (the other variables
    have empty lists); no_empty = position(s) of variables that do not store
    the empty set.  Returns (N, offsets, sets, costs)."""
    pos = list(range(n)) if at is None else list(at)
    N = n if N is None else N
    no_empty = () if no_empty is None else (no_empty if isinstance(no_empty, (tuple, list)) else (no_empty,))
    specs = [None] * N
    for i, v in enumerate(pos):
        sup = sum(1 << b for b in pos if b != v)
        specs[v] = dict(support=sup, count=count, max_size=3, empty=(i not in no_empty), dense=False, crafted=False,
                        span=PDB_SPANS[i % len(PDB_SPANS)])
        if must is not None and i in no_empty:
            specs[v]["must"] = 1 << pos[must]
    return (N,) + make_lists(N, specs, seed, kind=kind)[:3]
