"""Inputs, samples and by-construction facts for the wide cBIC layers past 19
parents (tests/test_gpu_wide_shapes.py; tests/test_wide_shapes.py proves the
claims below on the CPU).

The design.  N = 256 records, lambda = 2 (one penalty = 2 ln 256 = 11.09).
Every column is built from an orthonormal basis of the space orthogonal to the
constant vector, so the sample correlations are exact, not merely expected:

  * "strong" columns x_i: unit vectors with pairwise sample correlation
    RHO = 0.02 exactly (basis times the Cholesky factor of the equicorrelation
    matrix);
  * a target y = sum_i beta_i x_i + sigma q over ITS strong columns, q a basis
    vector of its own, beta_i = beta (1 + 0.02 u_i) with u_i spread over
    [-1, 1] (so no two sets tie), scaled so that all its strong columns
    together leave 10 % of its variance.  With equal weights the residual
    after k of ms columns is R_k = 1 - 0.9 k (1 + (ms - 1) RHO) / (ms (1 + (k -
    1) RHO)), and N ln(R_k / R_k+1) is smallest at k = 0: 14.0 at ms = 25, 17.7
    at ms = 20, against the penalty 11.09.  So every strong column, added to
    any set of the others, gains more than one penalty: every junk-free set is
    stored, by none of its subsets dominated;
  * "junk" columns: further basis vectors, exactly orthogonal to every other
    column and to the targets.  Adding one leaves rss unchanged (to rounding)
    and costs one penalty.  They sit at the lowest candidate indices, so the
    recursion (which removes entries in ascending order) takes the junk out
    of a set first and meets its junk-free subset, which dominates it, within
    a few steps;
  * a "spare" column 0 (one more basis vector) where variable 0 is to be absent
    from the candidates.

What is stored, by construction.  A set P = S + J (S strong, J junk, J not
empty) has ts(P) = ts(S) + |J| penalties.  If ts(P) < 0 its subset S is
present with -ts(S) > -ts(P): dominated.  If ts(P) > 0 the reference's
calculateScore returns before the recursion and the caller stores the set
with the negative value -ts(P) (score_calculator.cpp:111) -- the small sets
whose strong part has not yet earned |J| penalties.  So the stored sets are
exactly: every junk-free set, and every set with junk whose own ts is
positive.  (Not "exactly the junk-free ones": the store rule of sets with
ts >= 0 adds the second kind.)  ts depends on the strong part almost only
through |S|; sign_classes() shows no (|S|, |J|) class comes near ts = 0.

Each column is finally scaled and shifted (x (1 + c / 8) + c for column c) so
that the normalisation has work to do."""
import functools
import math

import numpy as np

N_REC = 256
LAM = 2.0
RHO = 0.02
LEFT = 0.10  # variance of a target left by all its strong columns ...
# ... unless its number of strong columns is listed here: picked so that no
# (|S|, |J|) class has ts within 0.5 of zero (sign_classes; the CPU file asserts it)
LEFT_BY_MS = {9: 0.13, 11: 0.08, 14: 0.06, 17: 0.09, 18: 0.13, 19: 0.09, 21: 0.07, 22: 0.12}
SPREAD = 0.004
WALK_BUDGET = 10 ** 5


def bits(vs):
    m = 0
    for v in vs:
        m |= 1 << int(v)
    return m


def _basis(ncols, seed):
    """ncols orthonormal vectors of length N_REC, all orthogonal to the constant vector."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N_REC, ncols + 1))
    A[:, 0] = 1.0
    Q, _ = np.linalg.qr(A)
    Q2, _ = np.linalg.qr(Q)  # a second pass: orthogonal to rounding
    return Q2[:, 1:]


def _build(n, strong, targets, seed):
    """strong: the strong columns; targets: {column: its strong columns}; every
    other column is a basis vector of its own (junk or spare)."""
    Q = _basis(n, seed)
    X = np.zeros((N_REC, n))
    ms = len(strong)
    E = np.full((ms, ms), RHO) + (1.0 - RHO) * np.eye(ms)
    Xs = Q[:, :ms] @ np.linalg.cholesky(E).T
    for k, c in enumerate(strong):
        X[:, c] = Xs[:, k]
    used = ms
    for c in range(n):
        if c in strong:
            continue
        if c in targets:
            own = targets[c]
            k = len(own)
            u = np.array([((7 * i) % k) / max(k - 1, 1) * 2.0 - 1.0 for i in range(k)])
            w = 1.0 + SPREAD * u
            part = Xs[:, [strong.index(s) for s in own]] @ w
            left = LEFT_BY_MS.get(k, LEFT)
            beta2 = (1.0 - left) / float(part @ part)
            X[:, c] = math.sqrt(beta2) * part + math.sqrt(left) * Q[:, used]
        else:
            X[:, c] = Q[:, used]
        used += 1
    for c in range(n):
        X[:, c] = X[:, c] * (1.0 + c / 8.0) + c
    return X


# name -> (m, junk columns, where variable 0 is: "junk", "strong" or "absent")
SINGLE = {
    "m20_j3_zero_junk": (20, 3, "junk"),
    "m20_j3_zero_absent": (20, 3, "absent"),
    "m21_all": (21, 0, "strong"),
    "m21_j2_zero_junk": (21, 2, "junk"),
    "m21_j2_zero_absent": (21, 2, "absent"),
    "m22_all": (22, 0, "strong"),
    "m22_j4_zero_junk": (22, 4, "junk"),
    "m24_all": (24, 0, "strong"),
    "m24_j3_zero_junk": (24, 3, "junk"),
    "m24_j3_zero_absent": (24, 3, "absent"),
    "m25_all": (25, 0, "strong"),
    "m25_j4_zero_junk": (25, 4, "junk"),
    "m25_j3_zero_absent": (25, 3, "absent"),
    # the CPU file's full-oracle-list proofs of the same design
    "m12_all": (12, 0, "strong"),
    "m12_j3_zero_junk": (12, 3, "junk"),
    "m12_j2_zero_absent": (12, 2, "absent"),
    "m14_all_zero_absent": (14, 0, "absent"),
    "m14_j3_zero_junk": (14, 3, "junk"),
    "m14_j4_zero_absent": (14, 4, "absent"),
}
GPU_SINGLE = [k for k in SINGLE if int(k[1:3]) >= 20]
CPU_FULL = [k for k in SINGLE if int(k[1:3]) <= 14]
MIXED = "mixed_m12_m24_m25"


class Case:
    """One input: X, the target variables, their candidate masks, and per
    target the junk and strong columns."""

    def __init__(self, name, X, variables, cands, junk, strong):
        self.name, self.X, self.n = name, X, X.shape[1]
        self.variables, self.cands = list(variables), [int(c) for c in cands]
        self.junk = [sorted(j) for j in junk]
        self.strong = [sorted(s) for s in strong]
        self.mv = [len(j) + len(s) for j, s in zip(self.junk, self.strong)]
        self.k = max(self.mv)
        x = X - X.mean(axis=0)
        Z = x / np.sqrt((x * x).sum(axis=0) / (N_REC - 1))
        self.G = Z.T @ Z
        self.pen = LAM * math.log(N_REC)
        self._ts = {}

    def z(self, i):
        return bool(self.cands[i] & 1)

    def junk_mask(self, i):
        return bits(self.junk[i])

    def ts(self, i, P):
        """The set's own score the_score (BIC_OLS.cpp:366) in FP64 from the Gram
        matrix: design arithmetic (signs and margins), not a test reference."""
        P = int(P)
        key = (i, P)
        if key not in self._ts:
            v = self.variables[i]
            pv = [c for c in range(self.n) if (P >> c) & 1]
            if not pv:
                self._ts[key] = 0.0
            else:
                g = self.G[pv, v]
                rss = self.G[v, v] - g @ np.linalg.solve(self.G[np.ix_(pv, pv)], g)
                self._ts[key] = N_REC * math.log(rss / N_REC) + self.pen * len(pv)
        return self._ts[key]

    def stored(self, i, P):
        """By construction: junk-free, or the set's own ts is positive."""
        return not (int(P) & self.junk_mask(i)) or self.ts(i, P) > 0.0

    def lookup(self, i):
        """The finished list of variable i as wide_walk_ref.decide_walk reads it."""
        def f(T):
            return np.float32(-self.ts(i, T)) if self.stored(i, T) else None
        return f

    def expected_count(self, i):
        """Stored sets of variable i, given that ts has one sign per (|S|, |J|)
        class (sign_classes)."""
        ms, nj = len(self.strong[i]), len(self.junk[i])
        tot = 1 << ms
        for (k, j), (lo, hi) in self.sign_classes(i).items():
            assert lo * hi > 0 or k + j == 0
            if j >= 1 and lo > 0:
                tot += math.comb(ms, k) * math.comb(nj, j)
        return tot

    def sign_classes(self, i):
        """{(k strong, j junk): (min ts, max ts)} over the two extreme strong
        parts of each size (the k lightest and the k heaviest weights) and 30
        random ones: ts varies inside a class only by the 2 % weight spread."""
        s, jn = self.strong[i], self.junk[i]
        k_ = len(s)
        order = sorted(range(k_), key=lambda t: ((7 * t) % k_))
        rng = np.random.default_rng(77)
        out = {}
        for k in range(0, k_ + 1):
            parts = [bits(s[t] for t in order[:k]), bits(s[t] for t in order[k_ - k:])]
            parts += [bits(rng.choice(s, size=k, replace=False)) for _ in range(30)]
            base = [self.ts(i, p) for p in parts]
            for j in range(0, len(jn) + 1):
                out[(k, j)] = (min(base) + j * self.pen, max(base) + j * self.pen)
        return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name == MIXED:
        # junk 0..3, strong 4..24, targets 25 (12 strong, variable 0 no candidate),
        # 26 (3 junk + 21 strong = 24), 27 (4 junk + 21 strong = 25)
        strong = list(range(4, 25))
        tg = {25: strong[:12], 26: strong, 27: strong}
        X = _build(28, strong, tg, 9900)
        junk = [[], [0, 1, 2], [0, 1, 2, 3]]
        st = [tg[25], tg[26], tg[27]]
        return Case(name, X, [25, 26, 27], [bits(j + s) for j, s in zip(junk, st)], junk, st)
    m, nj, zero = SINGLE[name]
    first = 1 if zero == "absent" else 0
    junk = list(range(first, first + nj))
    strong = list(range(first + nj, first + m))
    v = first + m
    X = _build(v + 1, strong, {v: strong}, 9900 + sorted(SINGLE).index(name))
    return Case(name, X, [v], [bits(junk + strong)], [junk], [strong])


def sample_sets(c, i):
    """The sets of variable i that the tests re-decide one by one: every set of
    the top three layers; per layer 9 .. m - 3, 40 random sets with variable 0
    and 40 without (80 without where variable 0 is no candidate); 200 further
    stored sets (junk-free ones, of 9 and more members where there are 13 strong columns).  Seeded: the CPU file bounds the
    walks of exactly these sets."""
    rng = np.random.default_rng(4100 + i)
    cand = [u for u in range(c.n) if (c.cands[i] >> u) & 1]
    m = len(cand)
    full = bits(cand)
    out = [full] + [full ^ (1 << a) for a in cand]
    out += [full ^ (1 << a) ^ (1 << b) for x, a in enumerate(cand) for b in cand[x + 1:]]
    rest = [u for u in cand if u != 0]
    for L in range(9, m - 2):
        for with0 in (True, False):
            for _ in range(40):
                if with0 and c.z(i):
                    out.append(1 | bits(rng.choice(rest, size=L - 1, replace=False)))
                else:
                    out.append(bits(rng.choice(rest, size=min(L, len(rest)), replace=False)))
    out = list(dict.fromkeys(out))
    s, seen, more = c.strong[i], set(out), 0
    while more < 200:  # 200 further stored sets, none drawn twice
        L = int(rng.integers(9 if len(s) >= 13 else 1, len(s)))
        P = bits(rng.choice(s, size=L, replace=False))
        if P not in seen:
            seen.add(P)
            out.append(P)
            more += 1
    return out
