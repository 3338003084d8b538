"""The order search's contract (include/ulg.h, "Order search"; the kernels are
csrc/order_search.hip) restated in plain Python: numpy float64 for every sum,
Python integers for the stamps, masks and draws, order_mcmc_ref's Philox and
shuffle.  No GPU, no project binding.

Every value of the contract is a maximum of float32 scores or a fixed FP64
expression of such (two adds and a subtract for a gain, one add for S, an
ascending sum after a kick), with no transcendental: the device must give the
same bits, and the GPU tests ask for equality.

Search keeps the swaps' would-be terms cached, as the kernel does; fresh_gains()
recomputes every gain from the lists (tests/test_order_search_ref.py holds the
two equal at every step).  `events` collects what a search has met: "aspiration"
(a tabu swap taken), "nonimproving" (gain <= 0), "stuck" (no admissible swap),
"kick", "undone".
"""
import numpy as np

import order_mcmc_ref as om

NO_MOVE = 255
F = np.float64


def best(L, v, U):
    """b_v(U) and the least list index that attains it: (float64, int), (-inf, -1) without a compatible entry."""
    ok = (L.sets[v] & ~np.uint64(U)) == 0
    if not ok.any():
        return F(-np.inf), -1
    sc = np.where(ok, L.sc[v], -np.inf)
    i = int(np.argmax(sc))  # the first maximum
    return F(sc[i]) + F(0.0), i  # -0 reads +0


def order_best(L, order):
    """(terms float64 (n), parents by variable: Python ints) of one order."""
    terms, parents, U = np.zeros(L.n), [0] * L.n, 0
    for p, v in enumerate(order):
        terms[p], i = best(L, int(v), U)
        parents[int(v)] = int(L.sets[int(v)][i]) if i >= 0 else 0
        U |= 1 << int(v)
    return terms, parents


class Search:
    def __init__(self, L, seed, c, tenure, patience, order=None):
        self.L, self.n, self.seed, self.c, self.tenure, self.patience = L, L.n, seed, c, tenure, patience
        self.order = [int(v) for v in (om.shuffle(seed, [c], L.n)[0] if order is None else order)]
        self.t = self.idle = self.moves = self.kicks = 0
        self.stamp, self.events = {}, set()
        self._full()
        if not np.all(np.isfinite(self.term)):
            raise ValueError("the initial order has a -inf term")
        self.S = self.S_best = self._sum()
        self._keep_best()

    def _pre(self, p):
        U = 0
        for v in self.order[:p]:
            U |= 1 << v
        return U

    def _side(self, p):
        """The (term, entry) pairs positions p, p+1 would hold after swap p."""
        x, y, U = self.order[p], self.order[p + 1], self._pre(p)
        return [best(self.L, y, U), best(self.L, x, U | (1 << y))]

    def _full(self):
        both = [best(self.L, v, self._pre(p)) for p, v in enumerate(self.order)]
        self.term, self.ent = [b for b, _ in both], [i for _, i in both]
        self.cand = [self._side(p) for p in range(self.n - 1)]

    def _sum(self):
        S = F(0.0)
        for x in self.term:
            S = S + x
        return S

    def _keep_best(self):
        self.best_order, self.best_ent = list(self.order), list(self.ent)

    def best_parents(self):
        par = [0] * self.n
        for v, i in zip(self.best_order, self.best_ent):
            par[v] = int(self.L.sets[v][i])
        return par

    @staticmethod
    def _gain(cand, t0, t1):
        return (cand[0][0] + cand[1][0]) - (t0 + t1)

    def gains(self):
        return [self._gain(self.cand[p], self.term[p], self.term[p + 1]) for p in range(self.n - 1)]

    def fresh_gains(self):
        return [self._gain(self._side(p), self.term[p], self.term[p + 1]) for p in range(self.n - 1)]

    def step(self):
        """One step -> (applied gain, position), (-inf, NO_MOVE) when nothing moved."""
        self.t += 1
        if self.n == 1:
            return F(-np.inf), NO_MOVE
        gains, pick, pick_tabu = self.gains(), -1, False
        for p, g in enumerate(gains):
            x, y = sorted(self.order[p:p + 2])
            st = self.stamp.get((x, y), 0)
            tabu = st != 0 and st >= self.t - self.tenure
            if not np.isfinite(g) or (tabu and not self.S + g > self.S_best):
                continue
            if pick < 0 or g > gains[pick]:
                pick, pick_tabu = p, tabu
        g, pos = F(-np.inf), NO_MOVE
        if pick >= 0:
            p, g, pos = pick, gains[pick], pick
            self.events |= ({"aspiration"} if pick_tabu else set()) | ({"nonimproving"} if g <= 0 else set())
            old = [(self.term[p], self.ent[p]), (self.term[p + 1], self.ent[p + 1])]
            (self.term[p], self.ent[p]), (self.term[p + 1], self.ent[p + 1]) = self.cand[p]
            self.cand[p] = old  # the reverse swap gives back the terms just left
            self.stamp[tuple(sorted(self.order[p:p + 2]))] = self.t
            self.order[p], self.order[p + 1] = self.order[p + 1], self.order[p]
            self.S = self.S + g
            self.moves += 1
            for q in (p - 1, p + 1):
                if 0 <= q < self.n - 1:
                    self.cand[q] = self._side(q)
        else:
            self.events.add("stuck")
        if self.S > self.S_best:
            self.S_best, self.idle = self.S, 0
            self._keep_best()
        else:
            self.idle += 1
        if self.idle >= self.patience:
            self._kick()
        return g, pos

    def _kick(self):
        self.order = list(self.best_order)
        for k in range(max(2, self.n // 4)):
            w = om._draw(self.seed, self.t, [self.c], 1 + k)
            i = int(om.mulhi32(w[0], self.n)[0])
            j = int(om.mulhi32(w[1], self.n - 1)[0])
            j += j >= i
            self.order[i], self.order[j] = self.order[j], self.order[i]
        self._full()
        bad = not np.all(np.isfinite(self.term))
        if bad:  # undone: back on the best order
            self.order = list(self.best_order)
            self._full()
        else:
            self.kicks += 1
        self.events.add("undone" if bad else "kick")
        self.stamp, self.S, self.idle = {}, self._sum(), 0
        if not bad:
            if self.S > self.S_best:
                self.S_best = self.S
                self._keep_best()
            else:
                self.idle = 1


def run(searches, steps):
    """`steps` steps of every Search of the list -> the binding's dict of this call."""
    C, n = len(searches), searches[0].n
    tg, tp = np.zeros((steps, C)), np.zeros((steps, C), dtype=np.uint8)
    for c, s in enumerate(searches):
        for k in range(steps):
            tg[k, c], tp[k, c] = s.step()
    return {"trace_gain": tg, "trace_pos": tp, "best_score": np.array([s.S_best for s in searches]),
            "best_order": np.array([s.best_order for s in searches], dtype=np.uint8).reshape(C, n),
            "best_parents": np.array([s.best_parents() for s in searches], dtype=np.uint64).reshape(C, n),
            "moves": np.array([s.moves for s in searches], dtype=np.int64),
            "kicks": np.array([s.kicks for s in searches], dtype=np.int64),
            "order": np.array([s.order for s in searches], dtype=np.uint8).reshape(C, n),
            "terms": np.array([s.term for s in searches]).reshape(C, n), "score": np.array([s.S for s in searches])}


# ---- the tests' inputs ---------------------------------------------------------------
def random_lists(n, seed, per_var, max_parents, rooted=(), grid=0.25, high=False):
    """Structureless lists: per variable the empty set (not for the variables of `rooted`: each of their sets
    holds a parent) and random sets of 1 .. max_parents parents, duplicates dropped; scores on a coarse grid, so that values tie.  high:
    the parents are drawn from the upper half of the variables (above bit 31 for n > 33)."""
    rng = np.random.default_rng(seed)
    offsets, sets, scores = [0], [], []
    for v in range(n):
        pool = [u for u in range(n // 2 if high else 0, n) if u != v]
        mine = set() if v in rooted else {0}
        for _ in range(per_var(v) if callable(per_var) else per_var):
            k = int(rng.integers(1, max_parents + 1))
            mine.add(sum(1 << int(u) for u in rng.choice(pool, size=min(k, len(pool)), replace=False)))
        mine = sorted(mine)
        rng.shuffle(mine)
        sets += mine
        scores += list(-np.round(rng.uniform(1, 40, len(mine)) / grid) * grid)
        offsets.append(len(sets))
    return om.Lists(n, offsets, np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))


def full_lists(n, seed, max_parents):
    """Every parent set of at most max_parents parents, random scores: the reachability input."""
    rng = np.random.default_rng(seed)
    offsets, sets, scores = [0], [], []
    for v in range(n):
        mine = [P for P in range(1 << n) if not (P >> v) & 1 and bin(P).count("1") <= max_parents]
        sets += mine
        scores += list(-rng.uniform(1, 40, len(mine)))
        offsets.append(len(sets))
    return om.Lists(n, offsets, np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))


def inputs():
    """name -> (Lists, seed, tenure, patience): n = 5 (lists shorter than a wave, two variables without the empty set:
    orders with a -inf term; a long tenure), n = 8 (the reachability input), n = 33 (tenure 0, parents above bit 31),
    n = 63 (one list of 5,000 entries on a coarse grid, parents above bit 31)."""
    return {
        "n5": (random_lists(5, 13, 6, 2, rooted=(0, 1)), 24, 1 << 20, 6),
        "n8": (full_lists(8, 21, 2), 5, 4, 32),
        "n33": (random_lists(33, 31, 40, 3, high=True), 7, 0, 20),
        "n63": (random_lists(63, 41, lambda v: 5000 if v == 40 else 30, 4, grid=1.0, high=True), 9, 31, 25),
    }
