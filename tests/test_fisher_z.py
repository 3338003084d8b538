"""The oracle's Fisher-z test (ora_partial_z, oracle/ora_mmpc.c) against a
long-double restatement of the rule in that file's header.

ulg_mmpc and ulg_mmpc_min_z are compared with ora_partial_z, so a mistake made
the same way on both sides would pass every GPU test.  This file restates the
rule a third time, independently: numpy longdouble (80-bit x87, eps 1.08e-19)
with hand-written Cholesky loops -- np.linalg drops to double -- on a Gram
matrix that is itself built in long double from the raw data.

Bound (u = 2^-53, k = |S|, kappa the 2-norm condition number of the
correlation block on {X, T} + S, dof = N - k - 3, r the partial correlation):

    |z_ora - z_exact| <= 8 (k + 2)^2 kappa u sqrt(dof) / (1 - r^2) + 4 u z

The Cholesky of the (k + 2)-block in double has a backward error of at most
about (k + 2)^2 u relative to the block (Higham, Accuracy and Stability, thm
10.3, first order), the rounding of the long-double Gram entries to the doubles
the oracle reads is one u more per entry, and a relative perturbation e of the
block moves the partial correlation -- a ratio of entries of the block's
inverse -- by at most about 2 kappa e (1 - r^2 <= 1 absorbs the rest); 8 covers
those constants.  d atanh(r) = dr / (1 - r^2), the factor sqrt(dof) scales it
to z, and log, the division in front of it and the final product are 4
roundings on z itself.  Largest ratio to the bound observed over every input
below: RATIO_SEEN.
"""
import ctypes as C
import math

import numpy as np
import pytest

import synth

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "no 80-bit long double here: this file would check double against double"

U = 2.0 ** -53
KAPPA_MAX = 1e4
RATIO_SEEN = 0.023  # the largest |z_ora - z_exact| / bound of test_partial_z_within_bound (x86-64, glibc)

STAR_N, STAR_ROWS, STAR_HUB = 40, 4001, 37
STAR_CHILDREN = (3, 8, 20, 31, 32, 33, 34, 35, 38, 39, 0, 1)


def star_data(seed=9900):
    """40 columns, N = 4001: a hub at column 37 with twelve children 0.8 h + noise
    (columns on both sides of bit 31), every other column independent noise."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((STAR_ROWS, STAR_N))
    for c in STAR_CHILDREN:
        X[:, c] += 0.8 * X[:, STAR_HUB]
    return X


def ld_gram(X):
    """G = Z'Z in long double as BIC_OLS.cpp:66-97 normalises: the column minus its
    mean, divided by the sample sd (N - 1) of that centred column about its own mean."""
    x = np.asarray(X, dtype=np.float64).astype(LD)
    N = x.shape[0]
    c = x - x.sum(0) / LD(N)
    c2 = c - c.sum(0) / LD(N)
    with np.errstate(invalid="ignore", divide="ignore"):
        Z = c / np.sqrt((c2 * c2).sum(0) / LD(N - 1))
        return Z.T @ Z


def ld_partial_r(G, X, T, S):
    """The partial correlation of X and T given S, every operation in long double."""
    k = len(S)
    L = np.zeros((k, k), dtype=LD)
    for i in range(k):
        for j in range(i + 1):
            s = G[S[i], S[j]]
            for q in range(j):
                s = s - L[i, q] * L[j, q]
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    a, c, b = G[X, X], G[T, T], G[X, T]
    yx = np.zeros(k, dtype=LD)
    yt = np.zeros(k, dtype=LD)
    for i in range(k):
        sx, st = G[S[i], X], G[S[i], T]
        for q in range(i):
            sx = sx - L[i, q] * yx[q]
            st = st - L[i, q] * yt[q]
        yx[i] = sx / L[i, i]
        yt[i] = st / L[i, i]
        a = a - yx[i] * yx[i]
        c = c - yt[i] * yt[i]
        b = b - yx[i] * yt[i]
    return b / np.sqrt(a * c)


def ld_z(G, N, X, T, S):
    """(z, bound) of one test: |atanh r| sqrt(dof) in long double and the module bound."""
    k = len(S)
    dof = N - k - 3
    r = ld_partial_r(G, X, T, S)
    z = np.abs(np.arctanh(r)) * np.sqrt(LD(dof))
    idx = [X, T] + list(S)
    kappa = np.linalg.cond(np.asarray(G[np.ix_(idx, idx)], dtype=np.float64), 2)
    assert kappa <= KAPPA_MAX, (X, T, S, kappa)
    bound = 8.0 * (k + 2) ** 2 * kappa * U * math.sqrt(dof) / float(1 - r * r) + 4.0 * U * float(z)
    return z, bound


def ora_z(oracle, G64, N, X, T, S):
    """ora_partial_z on a row-major double matrix; S as given (the caller sorts)."""
    n = G64.shape[0]
    s = np.ascontiguousarray(S, dtype=np.int32)
    return oracle.lib().ora_partial_z(G64.ctypes.data_as(C.c_void_p), n, float(N), int(X), int(T),
                                      s.ctypes.data_as(C.c_void_p), len(s))


def min_z_sets(pool, must, max_cond):
    """The conditioning sets of ora_mmpc.c's min_z, in its order: the pool without must,
    subset masks ascending, must appended and the set then sorted ascending."""
    others = [v for v in pool if v != must]
    need = 1 if must >= 0 else 0
    for m in range(1 << len(others)):
        if bin(m).count("1") + need > max_cond:
            continue
        S = [others[i] for i in range(len(others)) if (m >> i) & 1]
        if must >= 0:
            S.append(must)
        yield sorted(S)


def ora_min_z(oracle, G64, N, X, T, pool, must, max_cond, stop=-math.inf):
    """min_z of ora_mmpc.c restated over ora_partial_z (the function is static there)."""
    best = math.inf
    for S in min_z_sets(pool, must, max_cond):
        z = ora_z(oracle, G64, N, X, T, S)
        if z < best:
            best = z
        if best <= stop:
            break
    return best


@pytest.fixture(scope="module")
def grams():
    """(name, N, G long double, G rounded to double) of the SEM and the star data."""
    out = []
    for name, X in (("sem", synth.gaussian_sem(14, 403, 9901)[0]), ("sem2", synth.gaussian_sem(14, 403, 9902)[0]),
                    ("star", star_data())):
        G = ld_gram(X)
        out.append((name, X.shape[0], G, np.ascontiguousarray(G, dtype=np.float64)))
    return out


def _triples(name, n, rng):
    """(X, T, S) with |S| = 0 ... 12: 20 per size on each SEM (|S| = 12 takes all 14
    variables), 10 per size on the star data around its hub and across bit 31."""
    per = 10 if name == "star" else 20
    for k in range(13):
        for _ in range(per):
            p = rng.permutation(n)
            if name == "star" and k >= 1:  # the hub, or some of its children, in S
                front = [STAR_HUB] if rng.random() < 0.5 else list(rng.permutation(STAR_CHILDREN)[:min(k, 5)])
                p = np.array(front + [v for v in p if v not in front])
                X, T, S = int(p[k]), int(p[k + 1]), [int(v) for v in p[:k]]
            else:
                X, T, S = int(p[0]), int(p[1]), [int(v) for v in p[2:2 + k]]
            yield X, T, S


def test_partial_z_within_bound(oracle_built, grams):
    """ora_partial_z against the long-double value on several hundred (X, T, S),
    |S| = 0 ... 12, S sorted as min_z sorts it."""
    rng = np.random.default_rng(77)
    worst, count = 0.0, 0
    for name, N, G, G64 in grams:
        for X, T, S in _triples(name, G.shape[0], rng):
            S = sorted(S)
            z, bound = ld_z(G, N, X, T, S)
            got = ora_z(oracle_built, G64, N, X, T, S)
            ratio = abs(float(LD(got) - z)) / bound
            assert ratio <= 1.0, (name, X, T, S, got, float(z), bound)
            worst = max(worst, ratio)
            count += 1
    print(f"ora_partial_z vs long double: {count} tests, largest ratio to the bound {worst:.3g}")
    assert count >= 600


def test_dof_not_positive_gives_zero(oracle_built, grams):
    _, _, _, G64 = grams[0]
    assert ora_z(oracle_built, G64, 5, 0, 1, [2, 3]) == 0.0  # dof = 5 - 2 - 3 = 0
    assert ora_z(oracle_built, G64, 4, 0, 1, [2, 3]) == 0.0  # dof < 0
    assert ora_z(oracle_built, G64, 6, 0, 1, [2, 3]) > 0.0  # dof = 1


def test_copy_of_target_gives_the_clamped_value(oracle_built):
    """X a copy of T: r = 1 is clamped to 1 - 1e-15, with and without a conditioning set."""
    X, _ = synth.gaussian_sem(8, 403, 9903)
    X[:, 6] = X[:, 1]
    G = ld_gram(X)
    G64 = np.ascontiguousarray(G, dtype=np.float64)
    r = 1 - 1e-15
    for S in ([], [2, 4]):
        dof = 403 - len(S) - 3
        got = ora_z(oracle_built, G64, 403, 6, 1, S)
        assert got == abs(0.5 * math.log((1 + r) / (1 - r))) * math.sqrt(dof)  # the oracle's own operations
        want = np.arctanh(LD(r)) * np.sqrt(LD(dof))
        assert abs(float(LD(got) - want)) <= 4 * U * float(want)


@pytest.mark.parametrize("max_cond", [0, 1, 3, 24])
def test_min_z_matches_long_double_minimum(oracle_built, grams, max_cond):
    """min_z restated (pool without must, masks ascending, must appended, sorted)
    against the long-double minimum over the same subsets, with and without must."""
    rng = np.random.default_rng(78 + max_cond)
    for name, N, G, G64 in grams:
        n = G.shape[0]
        for trial in range(6):
            p = [int(v) for v in rng.permutation(n)]
            if name == "star":
                p = [v for v in p if v != STAR_HUB]
                p.insert(2 + trial % 3, STAR_HUB)
            X, T, pool = p[0], p[1], p[2:2 + 1 + trial]
            for must in (-1, pool[trial // 2]):
                sets = list(min_z_sets(pool, must, max_cond))
                got = ora_min_z(oracle_built, G64, N, X, T, pool, must, max_cond)
                if not sets:
                    assert max_cond == 0 and must >= 0 and got == math.inf
                    continue
                exact = [ld_z(G, N, X, T, S) for S in sets]
                want = min(z for z, _ in exact)
                assert abs(float(LD(got) - want)) <= max(b for _, b in exact), (name, X, T, pool, must)
                # the early stop: the first value at or below the stop is the result
                vals = [ora_z(oracle_built, G64, N, X, T, S) for S in sets]
                stop = sorted(vals)[len(vals) // 2]
                first = next(i for i, v in enumerate(vals) if v <= stop)
                assert ora_min_z(oracle_built, G64, N, X, T, pool, must, max_cond, stop) == min(vals[:first + 1])
