"""Long-double reference of the BGe score (ulg_bge_*; csrc/bge.h has the formula)
and the inputs test_bge.py and test_gpu_bge.py share.

Everything is built from the raw data in numpy long double (x87 extended, 64-bit
mantissa): normalise each column to zero mean and unit sample variance (N - 1),
S = Z'Z, R = S + t I, an own Cholesky of R[Q,Q] with the variable last, then

    s(v, P) = c_l - 1/2 sum_{j<l} ln s_j - A_l ln s_l

on the pivots s_j.  c_l comes from math.lgamma (its error is about 1e-11
absolute at N = 1e4, far below a float32 ulp of the score).  A set that touches
a constant column (0 / 0 in the normalisation) is NaN.

kernel_order() restates the kernel's operation order (csrc/bge_dev.h) in plain
FP64 numpy on an FP64 Gram matrix: same column order, same running product of
the pivots, same two logarithms.  The device contracts each multiply-subtract
into one fma, which rounds once where numpy rounds twice: its error is no
larger."""
import functools
import itertools
import math

import numpy as np

LD = np.longdouble


def consts(N, n, alpha_mu, alpha_w, l):
    """-> (c_l, A_l, t) as Python floats.  alpha_w None or 0: n + alpha_mu + 1."""
    aw = n + alpha_mu + 1 if not alpha_w else alpha_w
    t = alpha_mu * (aw - n - 1) / (alpha_mu + 1)
    A = (N + aw - n + l + 1) / 2
    c = (math.lgamma(A) - math.lgamma((aw - n + l + 1) / 2) - (N / 2) * math.log(math.pi)
         + 0.5 * math.log(alpha_mu / (N + alpha_mu)) + ((aw - n + 2 * l + 1) / 2) * math.log(t))
    return c, A, t


def normalise(X, dt=LD):
    Z = np.asarray(X).astype(dt)
    N = Z.shape[0]
    Z = Z - Z.mean(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return Z / np.sqrt((Z * Z).sum(0) / dt(N - 1))


def members(mask):
    return [b for b in range(64) if (int(mask) >> b) & 1]


def list_order(cands, k):
    """A variable's parent sets in the scorer's order: (|set|, set value)."""
    out = []
    for L in range(min(k, len(cands)) + 1):
        out += sorted(sum(1 << p for p in comb) for comb in itertools.combinations(cands, L))
    return out


def ulp32(x):
    return float(np.spacing(np.abs(np.float32(x))))


class Ref:
    """The reference for one data set and one prior."""

    def __init__(self, X, alpha_mu=1.0, alpha_w=None):
        X = np.asarray(X, dtype=np.float64)
        self.N, self.n = X.shape
        self.alpha_mu, self.alpha_w = alpha_mu, alpha_w
        Z = normalise(X, LD)
        self.S = Z.T @ Z
        self.t = consts(self.N, self.n, alpha_mu, alpha_w, 0)[2]
        self.R = self.S + LD(self.t) * np.eye(self.n, dtype=LD)
        Z64 = normalise(X, np.float64)
        self.G64 = Z64.T @ Z64

    def consts(self, l):
        return consts(self.N, self.n, self.alpha_mu, self.alpha_w, l)

    def pivots(self, vs, masks):
        """Batched Cholesky pivots: -> list of (positions, pivots[B, l + 1]) per set size l."""
        by_l = {}
        for pos, (v, m) in enumerate(zip(vs, masks)):
            q = members(int(m) & ~(1 << int(v))) + [int(v)]
            by_l.setdefault(len(q) - 1, []).append((pos, q))
        out = []
        for l, items in sorted(by_l.items()):
            D = l + 1
            for c0 in range(0, len(items), 50000):
                chunk = items[c0:c0 + 50000]
                Q = np.array([q for _, q in chunk], dtype=np.int64)
                A = self.R[Q[:, :, None], Q[:, None, :]]  # [B, D, D]
                Lm = np.zeros_like(A)
                piv = np.zeros((len(chunk), D), dtype=LD)
                with np.errstate(invalid="ignore", divide="ignore"):
                    for j in range(D):
                        s = A[:, j, j] - (Lm[:, j, :j] * Lm[:, j, :j]).sum(1)
                        piv[:, j] = s
                        d = np.sqrt(s)
                        for i in range(j + 1, D):
                            Lm[:, i, j] = (A[:, i, j] - (Lm[:, i, :j] * Lm[:, j, :j]).sum(1)) / d
                out.append((l, np.array([p for p, _ in chunk]), piv))
        return out

    def scores(self, vs, masks):
        """-> long double array, NaN where a pivot is not > 0 or a constant column is touched."""
        res = np.full(len(vs), np.nan, dtype=LD)
        for l, pos, piv in self.pivots(vs, masks):
            c, A, _ = self.consts(l)
            with np.errstate(invalid="ignore", divide="ignore"):
                val = LD(c) - np.log(piv[:, :l]).sum(1) / 2 - LD(A) * np.log(piv[:, l])
                ok = np.all(piv > 0, axis=1)
            res[pos] = np.where(ok, val, LD(np.nan))
        return res

    def score(self, v, mask):
        return self.scores([v], [mask])[0]

    def kernel_order(self, v, mask, G=None):
        """The kernel's operation order in plain FP64 on G (default: the FP64 numpy Gram matrix)."""
        G = self.G64 if G is None else G
        q = members(int(mask) & ~(1 << int(v))) + [int(v)]
        L = len(q) - 1
        c, A, t = self.consts(L)
        t = np.float64(t)
        Lm = np.zeros((L + 1, L + 1), dtype=np.float64)
        prod, sigma, ok = np.float64(1.0), np.float64(0.0), True
        with np.errstate(invalid="ignore", divide="ignore"):
            for j in range(L + 1):
                s = np.float64(G[q[j], q[j]]) + t
                for k in range(j):
                    s = s - Lm[j, k] * Lm[j, k]
                ok = ok and bool(s > 0)
                if j < L:
                    prod = prod * s
                    inv = np.float64(1.0) / np.sqrt(s)
                    for i in range(j + 1, L + 1):
                        x = np.float64(G[q[i], q[j]])
                        for k in range(j):
                            x = x - Lm[i, k] * Lm[j, k]
                        Lm[i, j] = x * inv
                else:
                    sigma = s
            val = np.float64(c) - np.float64(0.5) * np.log(prod) - np.float64(A) * np.log(sigma)
        return float(val) if ok else float("nan")


# ---- inputs ------------------------------------------------------------------------
def sem(n, N, seed, density=0.3):
    """A random linear Gaussian SEM over a random upper-triangular DAG."""
    rng = np.random.default_rng(seed)
    W = np.triu(rng.uniform(0.5, 1.5, (n, n)) * rng.choice([-1, 1], (n, n)) * (rng.random((n, n)) < density), 1)
    X = np.zeros((N, n))
    for j in range(n):
        X[:, j] = X @ W[:, j] + rng.standard_normal(N)
    return X


@functools.lru_cache(maxsize=None)
def case(name):
    """The shared inputs, read-only.  -> X (N x n)."""
    rng = np.random.default_rng(2024)
    if name in ("n10_N8", "n10_N50", "n10_N1000"):
        X = sem(10, int(name.split("N")[1]), 11)
    elif name == "n32":      # one variable with 31 parents
        X = sem(32, 200, 12, density=0.15)
    elif name == "n63":      # the variable and its candidates above bit 31
        X = sem(63, 150, 13, density=0.08)
    elif name == "mixed":    # three variables with 3, 7 and 12 candidates
        X = sem(14, 300, 14)
    elif name == "n20":      # layer 6: 542,640 sets, more than one pass of the grid
        X = sem(20, 500, 15, density=0.2)
    elif name == "illcond":  # exact duplicate, affine copy, 1e-9-collinear
        X = sem(8, 400, 16)
        X[:, 3] = X[:, 1]
        X[:, 5] = 3.0 - 2.5 * X[:, 2]
        X[:, 6] = X[:, 0] + X[:, 4] + 1e-9 * rng.standard_normal(400)
    elif name == "c3like":   # the issue's trial shape: N = 1e4, n = 25 with a duplicate and a 1e-9-collinear column
        X = sem(25, 10000, 17)
        X[:, 3] = X[:, 1]
        X[:, 4] = X[:, 0] + X[:, 2] + 1e-9 * rng.standard_normal(10000)
    elif name == "const":    # column 2 is constant
        X = sem(6, 120, 18)
        X[:, 2] = 4.25
    elif name == "sum":      # variable 5 is its parents' sum plus 1e-3 noise: positive scores
        X = sem(6, 300, 19, density=0.0)
        X[:, 5] = X[:, 0] + X[:, 1] + X[:, 2] + 1e-3 * rng.standard_normal(300)
    elif name == "e2e":      # n = 6 with positive scores present
        X = sem(6, 250, 20, density=0.5)
        X[:, 4] = X[:, 0] - X[:, 1] + 1e-2 * rng.standard_normal(250)
        X[:, 5] = 2.0 * X[:, 3] + 5e-2 * rng.standard_normal(250)
    elif name == "prior":    # well conditioned, for the non-default prior
        X = sem(8, 600, 21)
    else:
        raise KeyError(name)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def ref(name, alpha_mu=1.0, alpha_w=None):
    return Ref(case(name), alpha_mu, alpha_w)
