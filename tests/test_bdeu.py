"""BDeu (`score --bdeu`, ULG_SCORE_BDEU) on the CPU: the Python restatement of
the reference's value and the exact value that the GPU tests check against,
their two bounds, the host check program and the command line's refusals.

The value.  For variable v of arity r, parent set P, q = prod r_p and
equivalent sample size ess,
    a_j = ess / q,  a_jk = ess / (q r),
    s = sum over non-empty cells   [ lgamma(a_jk + n_jk) - lgamma(a_jk) ]
      + sum over non-empty configs [ lgamma(a_j) - lgamma(a_j + n_j) ].

restated_bdeu() follows bdeu_scoring_function.cpp:21-35, 69-79, 117-166 in the
reference's own arithmetic: ess, a_j, a_jk, lgamma(a_j), lgamma(a_jk) and the
running score are float32; a cell in lexicographic contingency-table order
(as test_discrete.restated walks them) does `score -= lg_jk; score +=
float(lgamma(float(a_jk + n)))`, then a parent configuration in ascending index
order (the reference iterates a boost::unordered_map there) does `score +=
lg_j; score = float(score - lgamma(float(a_j + n_j)))`.

exact_bdeu() is the value the kernel promises: FP64 a_j and a_jk, every term
from math.lgamma, math.fsum of the terms.  It finds the counts with
numpy.unique on the 64-bit cell index and never allocates q r entries.  It
returns (exact64, T, A): T = the number of terms, A = sum (|lgamma(a + n)| +
|lgamma(a)|) over them.  With u = 2^-24:

B, restatement against exact64:  B = (2 T + 2) u A + ulp_f32(exact64).
  * 2 T u A: each of the T terms costs the running float32 score two
    additions, each rounding the partial sum, which never exceeds A.
  * u A: float(lgamma(a_jk + n)) and the float lg_j, lg_jk are rounded
    once per use; lgamma(a_j + n_j) enters as a double.
  * u A: the float32 arguments.  ess, a_j and a_jk are rounded to float and
    so is a + n; lgamma moves by |psi(x)| times the argument's error, and
    x |psi(x)| <= max(1 + x, x ln x) (psi(x) < ln x throughout, and
    x psi(x) = -1 - gamma x + ... below its zero at 1.46).  Nothing makes this
    part stay below u A for every conceivable table: restated_bdeu() therefore
    carries the running first-order error of its own arithmetic -- u |rounded
    result| for every float32 rounding, max(1 + x, x ln x) / x times the
    distance of each float32 argument from its FP64 value -- and
    test_restatement_within_bound_of_exact asserts that this budget stays
    below (2 T + 2) u A on every case the GPU tests hold to B.
  * ulp_f32(exact64): second-order terms, math.lgamma's own error (a few
    FP64 ulps of A) and fsum's single rounding, all far below one float ulp.

Ek, kernel against exact64:
    Ek = ulp_f32(exact64) / 2 + 2 (T 2^-(shift+1) + c (T + 3) 2^-52 A).
  * T 2^-(shift+1): bdeu_fix rounds each of the T terms to a multiple of
    2^-shift once; the integer sum is exact.  shift = bdeu_shift(N, ess)
    (csrc/disc_bdeu.h), restated in bdeu_shift() below.
  * c (T + 3) 2^-52 A: a term is the difference of two lgamma values.  With c
    the error of the device's FP64 lgamma in ulps, the two values are off by
    at most c 2^-52 (|lgamma(a + n)| + |lgamma(a)|): c 2^-52 A over all terms.
    a + n (one rounding, |psi| times 2^-53 (a + n), below the same quantity),
    the subtraction, the conversion of the integer sum to double and, on this
    side, math.lgamma's few ulps and fsum's one rounding are each at most
    2^-52 A more; (T + 3) covers them as Bk's does in test_discrete.py.  a_j
    and a_jk are the same IEEE divisions on both sides.  c is not documented
    for the device library; c = 64 is an assumption, stated here, and the
    tests assert that it does not matter: the part of Ek beyond ulp / 2 stays
    below 0.01 ulp_f32(exact64) on every case (so would c = 1000).
  * ulp_f32(exact64) / 2 and the factor 2: the one rounding to float, and the
    case of the FP64 sum lying within the small terms of a rounding boundary,
    as in test_discrete.py.
Nothing in B or Ek is measured.

What Ek can see (test_bound_resolves_one_record).  One record moved from the
fullest cell of a parent configuration to its emptiest other cell changes the
value by |ln(a_jk + n_to) - ln(a_jk + n_from - 1)|.  That change is 0 where
n_to = n_from - 1 (the table's counts are then the same multiset: no score can
tell), about 1 / n between two cells of n records each, and at least ln 2
wherever a cell of two or more records has an empty neighbour (a_jk <= 1).  A
float32 result near -2000 has an ulp of 1.2e-4, so no bound on a float32 value
can put *every* such change 100 Ek away: the test asserts 100 Ek wherever the
move fills an empty cell from a cell of two or more (every input has such
tables), and for the remaining tables that Ek stays below 1e-3 of the
smallest |value|, in the manner of test_kernel_bound_resolves_one_record.
Input g (62,000,000 records, values near -1e8) is float32-limited like the
large tables of that test: it is there for the scale of the fixed point."""
import functools
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG
from test_discrete import (ARITY_G, N_G, counts_table, g_counts, n6_case, parents_of, q_of, shape_input, shape_pairs,
                           synthetic, ulp_f32)

SCORE = os.path.join(PKG, "bin", "score")
CHECK = os.path.join(PKG, "bin", "bdeu_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "bdeu_check")

U24 = 2.0 ** -24
LGAMMA_ULPS = 64  # c above: assumed, and asserted not to matter
ARITY5 = [2, 3, 2, 4, 3]
SIZES5 = [2, 63, 64, 65, 257, 1000, 2500]
f32 = np.float32


# ---- the scale ------------------------------------------------------------------
def bdeu_shift(N, ess):
    """bdeu_shift() of csrc/disc_bdeu.h: U = 2 N (Lm + 1) < 2^ex, shift = min(32, 62 - ex)."""
    lm = max(-math.log(math.ldexp(ess, -63)), math.log(ess + N))
    return min(32, 62 - math.frexp(2.0 * N * (lm + 1.0))[1])


# ---- the exact value ------------------------------------------------------------
def exact_bdeu_from_counts(njk, nj, rv, q, ess):
    """(exact64, T, A) from the non-empty cell counts njk and parent-configuration counts nj."""
    a_j, a_jk = ess / float(q), ess / float(q * rv)
    lg_j, lg_jk = math.lgamma(a_j), math.lgamma(a_jk)
    terms, A = [], []
    for counts, a, lg, sign in ((njk, a_jk, lg_jk, 1.0), (nj, a_j, lg_j, -1.0)):
        vals, mult = np.unique(np.asarray(counts, dtype=np.int64), return_counts=True)
        for n, m in zip(vals.tolist(), mult.tolist()):
            x = math.lgamma(a + n)
            terms += [sign * (x - lg)] * m
            A.append((abs(x) + abs(lg)) * m)
    return math.fsum(terms), len(terms), math.fsum(A)


def _counts(codes, arity, v, mask):
    """Non-empty cell and parent-configuration counts, with the 64-bit indices they belong to."""
    N = codes.shape[0]
    cfg = np.zeros(N, dtype=np.int64)
    q = 1
    for p in parents_of(mask & ~(1 << v)):
        cfg += codes[:, p].astype(np.int64) * q
        q *= int(arity[p])
    rv = int(arity[v])
    assert q * rv < 2 ** 63
    cell = cfg + codes[:, v].astype(np.int64) * q
    return np.unique(cell, return_counts=True), np.unique(cfg, return_counts=True), rv, q


def exact_bdeu(codes, arity, v, mask, ess):
    """The value the kernel promises -> (exact64, T, A), see the module docstring.  Never allocates
    q r entries; q r < 2^63 (the scorer refuses anything larger)."""
    (_, njk), (_, nj), rv, q = _counts(codes, arity, v, mask)
    return exact_bdeu_from_counts(njk, nj, rv, q, ess)


def bound_b(exact, T, A):
    return (2 * T + 2) * U24 * A + ulp_f32(exact)


def bound_ek_extra(T, A, N, ess):
    """The part of Ek beyond ulp_f32 / 2."""
    return 2.0 * (T * 2.0 ** -(bdeu_shift(N, ess) + 1) + LGAMMA_ULPS * (T + 3) * 2.0 ** -52 * A)


def bound_ek(exact, T, A, N, ess):
    return ulp_f32(exact) / 2 + bound_ek_extra(T, A, N, ess)


# ---- the restatement --------------------------------------------------------------
def _g(x):
    """>= x |psi(x)| for x > 0."""
    return max(1.0 + x, x * math.log(x))


def restated_bdeu(codes, arity, v, mask, ess):
    """-> (float32 value as the reference computes it, first-order error budget of that arithmetic)."""
    mask &= ~(1 << v)
    ps = parents_of(mask)
    rv = int(arity[v])
    tab, q = counts_table(codes, arity, v, mask)
    ess32 = f32(ess)
    a_j, a_jk = f32(ess32 / f32(q)), f32(ess32 / f32(q * rv))
    lg_j, lg_jk = f32(math.lgamma(float(a_j))), f32(math.lgamma(float(a_jk)))
    a_j64, a_jk64 = ess / float(q), ess / float(q * rv)
    # lg's own error: its float rounding and its float32 argument
    e_lg_j = U24 * abs(float(lg_j)) + _g(a_j64) / a_j64 * abs(float(a_j) - a_j64)
    e_lg_jk = U24 * abs(float(lg_jk)) + _g(a_jk64) / a_jk64 * abs(float(a_jk) - a_jk64)
    members = sorted(ps + [v])
    base = {}
    b = 1
    for p in ps:
        base[p] = b
        b *= int(arity[p])
    base[v] = q
    score = f32(0.0)
    budget = 0.0
    for combo in itertools.product(*[range(int(arity[x])) for x in members]):
        n = int(tab[sum(k * base[x] for k, x in zip(combo, members))])
        if n == 0:
            continue  # makeContab holds no node for an empty cell
        x32 = f32(a_jk + f32(n))
        x64 = a_jk64 + n
        temp = f32(math.lgamma(float(x32)))
        score = f32(score - lg_jk)
        budget += e_lg_jk + U24 * abs(float(score))
        score = f32(score + temp)
        budget += U24 * abs(float(temp)) + _g(x64) / x64 * abs(float(x32) - x64) + U24 * abs(float(score))
    nj = tab.reshape(rv, q).sum(axis=0)
    for j in range(q):
        n = int(nj[j])
        if n == 0:
            continue
        score = f32(score + lg_j)
        budget += e_lg_j + U24 * abs(float(score))
        x32 = f32(a_j + f32(n))
        x64 = a_j64 + n
        score = f32(float(score) - math.lgamma(float(x32)))
        budget += _g(x64) / x64 * abs(float(x32) - x64) + U24 * abs(float(score))
    return score, budget


def restated_bdeu_lists(codes, arity, variables, candidates, max_parents, ess, constraints=()):
    """Per variable: [(mask, float32 value, B)] in (|set|, set value) order, R3 / R5 / R6 (the BIC
    rules of test_discrete.restated_lists on the BDeu value)."""
    n = codes.shape[1]
    out = []
    for v, cand in zip(variables, candidates):
        cs = parents_of(cand & ((1 << n) - 1) & ~(1 << v))
        alts = [(r, f) for (cv, r, f) in constraints if cv == v]
        lst = []
        for L in range(0, min(len(cs), max_parents) + 1):
            for m in sorted(sum(1 << p for p in comb) for comb in itertools.combinations(cs, L)):
                if alts and not any((r & ~m) == 0 and (m & f) == 0 for r, f in alts):
                    continue  # scores 1: never stored
                if arity[v] == 1:
                    if L == 0:
                        lst.append((m, f32(0.0), 0.0))
                    continue
                s, _ = restated_bdeu(codes, arity, v, m, ess)
                if (L == 0 and s < 1) or (L > 0 and s < 0):
                    lst.append((m, s, bound_b(*exact_bdeu(codes, arity, v, m, ess))))
        out.append(lst)
    return out


# ---- inputs shared with test_gpu_bdeu.py ----------------------------------------------
def all_pairs(n):
    vs, ps = [], []
    for v in range(n):
        others = [p for p in range(n) if p != v]
        for L in range(len(others) + 1):
            for comb in itertools.combinations(others, L):
                vs.append(v)
                ps.append(sum(1 << p for p in comb))
    return vs, ps


@functools.lru_cache(maxsize=None)
def case5(N):
    codes = synthetic(5, N, ARITY5, 1000 + N)
    codes.setflags(write=False)
    return codes


def cases5():
    """(N, ess) of the value tests."""
    return [(N, 1.0) for N in SIZES5] + [(257, 0.1), (257, 10.0)]


@functools.lru_cache(maxsize=None)
def reference5(N, ess):
    """Per (v, P) of the 5-variable case: (restated float32, budget, exact64, T, A).  Computed once."""
    codes = case5(N)
    out = []
    for v, m in zip(*all_pairs(5)):
        s, budget = restated_bdeu(codes, ARITY5, v, m, ess)
        out.append((s, budget) + exact_bdeu(codes, ARITY5, v, m, ess))
    return out


SHAPES = ["a", "b1500", "b2100", "c300", "f", "g"]


def shape_exact(name, v, m, ess=1.0):
    """exact_bdeu on shape_input(name); input g from its one-pass joint counts."""
    codes, arity = shape_input(name)
    if name == "g":  # exact_bdeu's sort of 62e6 indices takes a minute; the counts are the same
        tab, q = g_counts(v, m)
        nj = tab.reshape(-1, q).sum(axis=0)
        return exact_bdeu_from_counts(tab[tab > 0], nj[nj > 0], arity[v], q, ess)
    return exact_bdeu(codes, arity, v, m, ess)


# ---- the bounds, before any GPU sees them ---------------------------------------------
@pytest.mark.parametrize("N,ess", cases5())
def test_restatement_within_bound_of_exact(N, ess):
    worst = extra = slack = 0.0
    for (v, m), (s, budget, exact, T, A) in zip(zip(*all_pairs(5)), reference5(N, ess)):
        B = bound_b(exact, T, A)
        assert exact < 0, (v, m, exact)
        assert budget <= (2 * T + 2) * U24 * A, (v, m, budget, (2 * T + 2) * U24 * A)  # the derivation holds here
        assert abs(float(s) - exact) <= B, (v, m, float(s), exact, B)
        worst = max(worst, abs(float(s) - exact) / B)
        slack = max(slack, budget / ((2 * T + 2) * U24 * A))
        e = bound_ek_extra(T, A, N, ess) / ulp_f32(exact)
        assert e < 0.01, (v, m, e)
        extra = max(extra, e)
    print(f"N={N} ess={ess}: restatement within {worst:.3f} B, error budget {slack:.3f} of (2T+2) u A, "
          f"Ek beyond ulp/2 <= {extra:.4f} ulp_f32")


def test_restatement_within_bound_on_n6():
    codes, arity = n6_case()
    for ess in (1.0, 2.5):
        for v in range(6):
            others = [p for p in range(6) if p != v]
            for L in range(4):
                for comb in itertools.combinations(others, L):
                    m = sum(1 << p for p in comb)
                    s, budget = restated_bdeu(codes, arity, v, m, ess)
                    exact, T, A = exact_bdeu(codes, arity, v, m, ess)
                    assert budget <= (2 * T + 2) * U24 * A and abs(float(s) - exact) <= bound_b(exact, T, A)
                    assert bound_ek_extra(T, A, codes.shape[0], ess) < 0.01 * ulp_f32(exact)


def test_exact_from_counts_equals_dense_table():
    """exact_bdeu against the same sum over the dense table, and the shape of its (T, A)."""
    codes, arity = n6_case()
    for v, m in [(0, 0), (2, 0b011011), (5, 0b000110), (1, 0b111101)]:
        tab, q = counts_table(codes, arity, v, m)
        nj = tab.reshape(-1, q).sum(axis=0)
        a_j, a_jk = 0.7 / q, 0.7 / (q * arity[v])
        want = math.fsum([math.lgamma(a_jk + int(c)) - math.lgamma(a_jk) for c in tab if c] +
                         [math.lgamma(a_j) - math.lgamma(a_j + int(c)) for c in nj if c])
        got, T, A = exact_bdeu(codes, arity, v, m, 0.7)
        assert abs(got - want) <= 1e-12 * abs(want) and T == int((tab > 0).sum() + (nj > 0).sum()) and A > abs(got)


def test_shift_restatement():
    assert bdeu_shift(2, 1.0) == 32 and bdeu_shift(2500, 10.0) == 32
    assert bdeu_shift(N_G, 1.0) == 29  # 2 N (63 ln 2 + 1) = 5.5e9 < 2^33
    assert bdeu_shift(2 ** 31 - 1, 1e-6) == 24


def _one_record(name, ess):
    """-> (changes by at least 100 Ek where a cell of >= 2 records gives one to an empty cell,
    max Ek / |value| over the other tables, their smallest |value|, tables of each kind)."""
    codes, arity = shape_input(name)
    N = codes.shape[0]
    rel, smallest, filled, other = 0.0, math.inf, 0, 0
    for v, m in zip(*shape_pairs(name)):
        q, rv = q_of(arity, v, m), arity[v]
        if q * rv > 10 ** 6 or rv == 1:
            continue
        (cells, njk), _, _, _ = _counts(codes, arity, v, m)
        exact, T, A = exact_bdeu_from_counts(njk, _counts(codes, arity, v, m)[1][1], rv, q, ess)
        ek = bound_ek(exact, T, A, N, ess)
        a_jk = ess / float(q * rv)
        # the fullest cell, and the emptiest other cell of its parent configuration
        i = int(np.argmax(njk))
        n_from, cfg = int(njk[i]), int(cells[i]) % q
        mates = {int(c) // q: int(k) for c, k in zip(cells, njk) if int(c) % q == cfg}
        n_to = min(mates.get(k, 0) for k in range(rv) if k != int(cells[i]) // q)
        change = abs(math.log(a_jk + n_to) - math.log(a_jk + n_from - 1))
        if n_to == 0 and n_from >= 2:
            assert change >= math.log(2.0) * 0.999 and change > 100 * ek, (name, v, m, change, ek)
            filled += 1
        else:
            rel, smallest, other = max(rel, ek / abs(exact)), min(smallest, abs(exact)), other + 1
    return rel, smallest, filled, other


@pytest.mark.parametrize("name", ["a", "b1500", "b2100", "c300", "f"])
def test_bound_resolves_one_record(name):
    rel, smallest, filled, other = _one_record(name, 1.0)
    print(f"{name}: {filled} tables where one record fills an empty cell: change > 100 Ek; "
          f"{other} others: Ek <= {rel:.2e} |value|, smallest |value| {smallest:.1f}")
    assert filled > 0
    assert other == 0 or (rel < 1e-3 and smallest > 1)


def test_bound_on_the_five_variable_cases():
    """The same for the value tests' inputs: where some cell of two or more records has an empty
    neighbour the change is > 100 Ek; everywhere Ek < 1e-3 |value|."""
    for N, ess in cases5():
        codes = case5(N)
        for (v, m), (_, _, exact, T, A) in zip(zip(*all_pairs(5)), reference5(N, ess)):
            ek = bound_ek(exact, T, A, N, ess)
            assert ek < 1e-3 * abs(exact) and abs(exact) > 0.5, (N, ess, v, m, ek, exact)
            tab, q = counts_table(codes, ARITY5, v, m)
            t = tab.reshape(ARITY5[v], q)
            if ((t.max(axis=0) >= 2) & (t.min(axis=0) == 0)).any():
                a_jk = ess / (q * ARITY5[v])
                j = int(np.argmax((t.max(axis=0) >= 2) & (t.min(axis=0) == 0)))
                change = abs(math.log(a_jk) - math.log(a_jk + int(t[:, j].max()) - 1))
                assert change > 100 * ek, (N, ess, v, m, change, ek)


def test_input_g_is_where_the_scale_drops():
    """N = 62,000,000: the BDeu shift leaves 2^32, and the float32 result is what limits Ek."""
    assert bdeu_shift(N_G, 1.0) < 32 and ARITY_G == [3, 4]
    for v, m in zip(*shape_pairs("g")):
        exact, T, A = shape_exact("g", v, m)
        assert bound_ek_extra(T, A, N_G, 1.0) < 0.01 * ulp_f32(exact)
        # the terms at the scale in use stay far inside 64 bits
        assert A * 2.0 ** bdeu_shift(N_G, 1.0) < 2.0 ** 62


# ---- the host check programs ------------------------------------------------------------
def test_bdeu_check():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bdeu_check ok" in r.stdout, (r.stdout, r.stderr)


def test_bdeu_check_under_sanitizers():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/bdeu_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "bdeu_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- command line refusals ------------------------------------------------------------------
@pytest.mark.parametrize("opts", [["--bdeu", "-f", "cBIC"], ["--bdeu", "-e", "0"], ["--bdeu", "-e", "1e9"]])
def test_score_bdeu_refuses_before_opening_a_file(opts, tmp_path):
    out = tmp_path / "out.pss"
    r = subprocess.run([SCORE, str(tmp_path / "no_such_in.csv"), str(out), *opts], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert "--bdeu" in r.stderr and "cannot read" not in r.stderr and not out.exists()


def test_score_help_lists_bdeu():
    r = subprocess.run([SCORE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--bdeu" in r.stdout + r.stderr and "every subset" in r.stdout + r.stderr
