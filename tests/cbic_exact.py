"""A long-double reference of the cBIC value and the error bound the GPU's
FP64 Cholesky is held to ("cBIC accuracy contract").

cbic_exact(X, v, P, lam) -> (score, rss, beta_norm2, rank):
  * every column is normalised in np.longdouble as the reference does
    (BIC_OLS.cpp:66-97): minus its mean, divided by the sample standard
    deviation (N - 1) of the centred column;
  * the parent columns are orthogonalised in index order by modified
    Gram-Schmidt applied twice; a column whose squared residual is at most
    2^-100 of its own squared norm is dependent and dropped (a deviation below
    about 1e-15 of the column, the input's own FP64 rounding);
  * rss = the squared norm of the child's residual, beta_norm2 = |beta|^2 of
    the least-squares coefficients on the kept columns;
  * score = -(N ln(rss / N) + lam ln(N) |P|): the penalty counts |P|, not the
    rank, as the kernels and the reference do (BIC_OLS.cpp:366).

The bound.  B1 = (L + 1) u (N - 1) (1 + |beta|^2) with u = 2^-53, L = |P| is
the first-order error of rss out of a Cholesky factorisation of the FP64 Gram
matrix of normalised columns (diagonal N - 1); B = C B1 with C = 64 leaves a
factor of about seven over what the kernels' operation order needs in plain
FP64 (test_cbic_exact.py records its ratio) for the GPU's Gram matrix and FMA
contraction.  A set is resolvable when rss > 2 B; its score then lies within
score_bound().  An unresolvable set's rss may come out as anything in
[0, 3 B]: its score is +inf or at least unresolvable_floor().

Also here, shared by the CPU and the GPU tests: the seeded data classes, the
(variable, parent set) cases per class, the NumPy FP64 restatement of the
kernels' operation order with its guarded pivot, and the exact-dependency
inputs whose lists the layer and wide kernels must reproduce.
"""
import functools
import math

import numpy as np

import synth

LD = np.longdouble
F32 = np.float32
U = 2.0 ** -53
C_BOUND = 64.0
RANK_RULE = LD(2) ** -100
TAU = 32.0  # the kernels' pivot guard: s <= TAU (L + 1) u (N - 1) marks column j dependent (G[j, j] = N - 1)


def bits(*vs):
    m = 0
    for v in vs:
        m |= 1 << int(v)
    return m


def members(P, skip=-1):
    return [i for i in range(64) if (int(P) >> i) & 1 and i != skip]


class Exact:
    """One dataset, normalised once in long double."""

    def __init__(self, X):
        x = np.asarray(X, dtype=np.float64).astype(LD)
        self.N, self.n = x.shape
        with np.errstate(invalid="ignore", divide="ignore"):
            c = x - x.sum(axis=0) / LD(self.N)
            d = c - c.sum(axis=0) / LD(self.N)
            sd = np.sqrt((d * d).sum(axis=0) / LD(self.N - 1))
            self.Z = c / sd  # a constant column: 0 / 0, NaN throughout

    def cbic(self, v, P, lam):
        pv = members(P, v)
        L = len(pv)
        N = self.N
        if L == 0:
            return 0.0, LD(N - 1), 0.0, 0  # BIC_OLS.cpp:302-305
        with np.errstate(invalid="ignore", divide="ignore"):
            Q, A = [], []
            for j in pv:
                a = self.Z[:, j].copy()
                norm2 = a @ a
                for _ in range(2):
                    for q in Q:
                        a = a - (q @ a) * q
                r2 = a @ a
                if r2 <= RANK_RULE * norm2:  # NaN compares false: a constant column stays, and poisons
                    continue
                Q.append(a / np.sqrt(r2))
                A.append(self.Z[:, j])
            y = self.Z[:, v].copy()
            r = len(Q)
            c = np.zeros(r, dtype=LD)
            for _ in range(2):
                for k, q in enumerate(Q):
                    t = q @ y
                    c[k] += t
                    y = y - t * q
            rss = y @ y
            # A = Q R, R upper triangular; beta = R^-1 c by back substitution
            beta = np.zeros(r, dtype=LD)
            for k in range(r - 1, -1, -1):
                t = c[k]
                for m in range(k + 1, r):
                    t -= (Q[k] @ A[m]) * beta[m]
                beta[k] = t / (Q[k] @ A[k])
            score = -(LD(N) * np.log(rss / LD(N)) + LD(lam) * np.log(LD(N)) * LD(L))
        return float(score), rss, float(beta @ beta), r


def cbic_exact(X, v, P, lam):
    """-> (score, rss, beta_norm2, rank); X an N x n array or an Exact."""
    ex = X if isinstance(X, Exact) else Exact(X)
    return ex.cbic(v, P, lam)


class ExactDataset:
    """What test_constraints.Restatement needs of a dataset (n, cbic_raw) over
    cbic_exact: the_score = -score, rounded to float32 by the caller."""

    def __init__(self, X):
        self.ex = Exact(X)
        self.n = self.ex.n

    def cbic_raw(self, lam, v, P):
        return F32(-self.ex.cbic(v, P, lam)[0])


# ---- the bound ---------------------------------------------------------------
def b1(N, L, beta_norm2):
    return (L + 1) * U * (N - 1) * (1.0 + beta_norm2)


def resolvable(rss, B):
    return float(rss) > 2.0 * B


def score_bound(N, score, rss, B):
    """The score bound of a resolvable set (rss > 2 B): the logarithm over
    rss +- B, the float32 rounding of the stored score, and the FP64 rounding
    of N ln(rss / N)."""
    x = B / float(rss)
    return (N * max(math.log1p(x), -math.log1p(-x)) + 2.0 ** -23 * abs(score)
            + 4 * U * N * (1.0 + abs(math.log(float(rss) / N))))


def unresolvable_floor(N, L, lam, B):
    """The smallest finite score of an unresolvable set: rss = 3 B."""
    return -(N * math.log(3.0 * B / N) + lam * math.log(N) * L)


def check_value(got, N, L, lam, ref):
    """One GPU (or restated) score against the reference tuple of cbic_exact.
    -> (kind, message or None): kind 'nan' (a constant column), 'resolvable' or
    'unresolvable'; message is None when the value keeps the contract."""
    score, rss, beta2, _ = ref
    g = float(got)
    if math.isnan(float(rss)) or math.isnan(score):
        return "nan", None if math.isnan(g) else f"NaN expected, got {g}"
    if math.isnan(g):
        return "resolvable", "NaN"
    B = C_BOUND * b1(N, L, beta2)
    if resolvable(rss, B):
        tol = score_bound(N, score, rss, B)
        if abs(g - score) <= tol:
            return "resolvable", None
        return "resolvable", f"score {g!r} vs {score!r}: off by {abs(g - score):.3e}, bound {tol:.3e}"
    floor = unresolvable_floor(N, L, lam, B)
    if g == math.inf or (math.isfinite(g) and g >= floor):
        return "unresolvable", None
    return "unresolvable", f"unresolvable set (rss {float(rss):.3e}, B {B:.3e}): {g!r} below the floor {floor!r}"


# ---- the kernels' operation order in NumPy FP64 --------------------------------
def gram_fp64(X):
    """Z'Z of the FP64-normalised columns (the device's Gram matrix up to summation order)."""
    x = np.asarray(X, dtype=np.float64)
    N = x.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = x - x.sum(axis=0) / N
        d = c - c.sum(axis=0) / N
        Z = c / np.sqrt((d * d).sum(axis=0) / (N - 1))
        return Z.T @ Z


def restate_fp64(G, N, v, P, lam, guard=True):
    """cbic_set_score (csrc/cbic_dev.h) statement for statement,
    without FMA contraction.  -> (score as float32, rss)."""
    gv = members(P, v)
    L = len(gv)
    f = np.float64
    piv = f(TAU * U) * f(L + 1) * (f(N) - f(1.0))  # pivot_threshold: every diagonal entry of G is N - 1
    Lm = np.zeros((L, L))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(L):
            gjj = f(G[gv[j], gv[j]])
            s = gjj
            for k in range(j):
                s = s - Lm[j, k] * Lm[j, k]
            if guard and s <= piv:
                s = f(np.inf)
            d = np.sqrt(s)
            inv = f(1.0) / d
            Lm[j, j] = d
            for i in range(j + 1, L):
                t = f(G[gv[i], gv[j]])
                for k in range(j):
                    t = t - Lm[i, k] * Lm[j, k]
                Lm[i, j] = t * inv
        y = np.zeros(L)
        yy = f(0.0)
        for i in range(L):
            t = f(G[gv[i], v])
            for k in range(i):
                t = t - Lm[i, k] * y[k]
            t = t / Lm[i, i]
            y[i] = t
            yy = yy + t * t
        rss = f(G[v, v]) - yy
        if guard and rss < 0:
            rss = f(0.0)
        the_score = f(N) * np.log(rss / f(N)) + f(lam) * np.log(f(N)) * f(L)
        return -F32(the_score), rss


# ---- data classes --------------------------------------------------------------
N_VARS = 12
NEAR_PAIR = [1e-3, 1e-5, 1e-7, 1e-9]
NEAR_TRIPLE = [1e-3, 1e-5, 1e-7]
CLASSES = (["benign", "benign_N50"] + [f"near_pair_{e:g}" for e in NEAR_PAIR]
           + [f"near_triple_{e:g}" for e in NEAR_TRIPLE]
           + ["duplicate", "affine", "integer_sum", "integer_sum_dup", "N8"])
# at least 90 % of the cases with v outside the dependency must be resolvable
CAPPED = {"benign", "benign_N50", "near_pair_0.001", "near_pair_1e-05", "near_triple_0.001", "near_triple_1e-05",
          "duplicate", "affine", "integer_sum", "integer_sum_dup"}
LAM = 2.0


@functools.lru_cache(maxsize=None)
def data_class(name):
    """-> dict(X, N, n, groups): groups = the column sets of the (near-)dependencies."""
    n = N_VARS
    idx = CLASSES.index(name)
    N = {"benign_N50": 50, "duplicate": 50, "integer_sum_dup": 50, "N8": 8}.get(name, 1000)
    X, _ = synth.gaussian_sem(n, N, 9700 + idx)
    noise = np.random.default_rng(9800 + idx).standard_normal(N)
    groups = []
    if name.startswith("near_pair_"):
        e = float(name.split("_")[-1])
        X[:, 2] = X[:, 1] + e * noise
        groups = [(1, 2)]
    elif name.startswith("near_triple_"):
        e = float(name.split("_")[-1])
        X[:, 0] = 0.7 * X[:, 1] - 1.3 * X[:, 3] + e * noise
        groups = [(0, 1, 3)]
    elif name == "duplicate":
        X[:, 5] = X[:, 4]
        groups = [(4, 5)]
    elif name == "affine":
        X[:, 5] = 3.0 * X[:, 4] + 5.0
        groups = [(4, 5)]
    elif name in ("integer_sum", "integer_sum_dup"):
        X = np.round(8.0 * X)
        X[:, 3] = X[:, 1] + X[:, 2]
        groups = [(1, 2, 3)]
        if name == "integer_sum_dup":
            X[:, 5] = X[:, 4]
            groups.append((4, 5))
    return dict(name=name, X=X, N=N, n=n, lam=LAM, groups=groups)


@functools.lru_cache(maxsize=None)
def class_cases(name, count=150):
    """About `count` (v, P) pairs with |P| = 1 .. 10; every second one is forced
    to contain the dependent (or near-dependent) columns other than v.
    -> list of (v, P, outside): outside = v is in no dependency group."""
    d = data_class(name)
    n = d["n"]
    rng = np.random.default_rng(9900 + CLASSES.index(name))
    dep = sorted(set(c for g in d["groups"] for c in g))
    out = []
    for i in range(count):
        L = 1 + i % 10
        v = int(rng.integers(n))
        others = [x for x in range(n) if x != v]
        forced = [c for c in dep if c != v] if (i // 10) % 2 else []
        forced = forced[:L] if len(forced) <= L else [int(c) for c in rng.choice(forced, size=L, replace=False)]
        rest = [x for x in others if x not in forced]
        pick = forced + [int(c) for c in rng.choice(rest, size=L - len(forced), replace=False)]
        out.append((v, bits(*pick), v not in dep))
    return out


@functools.lru_cache(maxsize=None)
def class_reference(name):
    """cbic_exact of every case of the class, computed once."""
    d = data_class(name)
    ex = Exact(d["X"])
    return [ex.cbic(v, P, d["lam"]) for v, P, _ in class_cases(name)]


@functools.lru_cache(maxsize=None)
def constant_case():
    """A benign dataset with one constant column (its normalised form is 0 / 0)."""
    X, _ = synth.gaussian_sem(8, 50, 9790)
    X[:, 6] = 2.5
    return dict(X=X, N=50, n=8, lam=LAM, constant=6)


# ---- the exact-dependency inputs of the list tests -----------------------------
def _dependent_input(n, N, seed):
    X, _ = synth.gaussian_sem(n, N, seed)
    X = np.round(8.0 * X)
    X[:, 3] = X[:, 1] + X[:, 2]
    X[:, 5] = X[:, 4]
    return X


INSIDE = (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def list_case(name):
    """'k4': n = 10, N = 300, k = 4, every variable (x3 = x1 + x2, x5 = x4 on
    integer data); 'k10': n = 12, N = 300, k = 10 on one variable outside the
    dependencies and one inside, so that layers 9 and 10 (the wide kernels) run."""
    if name == "k4":
        n, k = 10, 4
        X = _dependent_input(n, 300, 9759)
        variables = list(range(n))
    elif name == "k10":
        n, k = 12, 10
        X = _dependent_input(n, 300, 9756)
        variables = [7, 3]
    else:
        raise KeyError(name)
    return dict(X=X, n=n, N=300, lam=LAM, k=k, variables=variables, cands=[(1 << n) - 1] * len(variables),
                outside=[v for v in variables if v not in INSIDE], inside=[v for v in variables if v in INSIDE])


@functools.lru_cache(maxsize=None)
def exact_lists(name):
    """test_constraints.Restatement over cbic_exact for the variables outside
    the dependencies. -> {v: (sets, scores, margin)}"""
    import test_constraints as tc
    c = list_case(name)
    ds = ExactDataset(c["X"])
    out = {}
    for v in c["outside"]:
        r = tc.Restatement(ds, c["lam"], v, [])
        s, sc = r.run((1 << c["n"]) - 1, c["k"])
        out[v] = (s, sc, r.margin)
    return out


# ---- the three forms, bit for bit ----------------------------------------------
@functools.lru_cache(maxsize=None)
def forms_case(near=False):
    """One child (variable 10) with ten informative parents (weights
    +-U[0.5, 1.5], N = 1000), k = 10: every layer 1 .. 10 stores sets.  near:
    the same with x2 = x1 + 1e-5 noise (the near-collinear class)."""
    rng = np.random.default_rng(9760)
    N, n = 1000, 11
    X = rng.standard_normal((N, n))
    if near:
        X[:, 2] = X[:, 1] + 1e-5 * rng.standard_normal(N)
    w = rng.uniform(0.5, 1.5, size=10) * np.where(rng.random(10) < 0.5, 1.0, -1.0)
    X[:, 10] = X[:, :10] @ w + rng.standard_normal(N)
    return dict(X=X, n=n, N=N, lam=LAM, k=10, v=10)
