"""Discrete BIC (`score -f BIC`) on the CPU: the record reader, the Python
restatement of the reference's value that the GPU tests check against, and the
command line's refusals.

The restatement follows bic_scoring_function.cpp:20-76 and
log_likelihood_calculator.cpp:17-77: counts from numpy, the float32 table
ilogi[i] = float(i * log(i)), float32 additions over the cells in
lexicographic contingency-table order (variables of P u {v} ascending, the
first outermost), then float32 subtractions over the parent configurations in
ascending index order (the reference iterates a boost::unordered_map there: its
own order is unspecified), then the penalty t * float(log(N) / 2).

Tolerance.  Any order of T float additions of terms x_i is within
(T + 2) 2^-24 sum|x_i| of the exact sum; the bound counts one more rounding for
each table entry and for the penalty product.  Per set
    B = (T + 2) 2^-24 (sum_cells n ln n + sum_j n_j ln n_j + t ln(N) / 2) + ulp_float(|score|)
with T = the number of terms added or subtracted."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG

HEP = os.path.join(GOLDEN, "hepatitis.clean.csv")
DUMP = os.path.join(PKG, "bin", "records_dump")
SAN_DUMP = os.path.join(PKG, "bin", "san", "records_dump")
SCORE = os.path.join(PKG, "bin", "score")


# ---- the restatement --------------------------------------------------------
def parents_of(mask):
    return [p for p in range(64) if (mask >> p) & 1]


def counts_table(codes, arity, v, mask):
    """Dense table, cell = sum_p code_p base_p + code_v q (parents ascending, first base 1)."""
    ps = parents_of(mask & ~(1 << v))
    idx = np.zeros(codes.shape[0], dtype=np.int64)
    q = 1
    for p in ps:
        idx += codes[:, p].astype(np.int64) * q
        q *= int(arity[p])
    idx += codes[:, v].astype(np.int64) * q
    return np.bincount(idx, minlength=q * int(arity[v])).astype(np.int64), q


def restated(codes, arity, v, mask):
    """-> (float32 value as the reference sums it, FP64 value, bound B)."""
    N = codes.shape[0]
    mask &= ~(1 << v)
    ps = parents_of(mask)
    rv = int(arity[v])
    tab, q = counts_table(codes, arity, v, mask)
    # lexicographic contingency-table order over P u {v}, first variable outermost
    members = sorted(ps + [v])
    base = {}
    b = 1
    for p in ps:
        base[p] = b
        b *= int(arity[p])
    base[v] = q
    score = np.float32(0.0)
    sum_abs = 0.0
    terms = 0
    for combo in itertools.product(*[range(int(arity[x])) for x in members]):
        c = int(tab[sum(k * base[x] for k, x in zip(combo, members))])
        if c == 0:
            continue  # makeContab holds no node for an empty cell
        score = np.float32(score + np.float32(c * math.log(c)))
        sum_abs += c * math.log(c)
        terms += 1
    nj = tab.reshape(rv, q).sum(axis=0)
    exact = float(sum(int(c) * math.log(int(c)) for c in tab if c > 0))
    for j in range(q):
        c = int(nj[j])
        if c == 0:
            continue
        score = np.float32(score - np.float32(c * math.log(c)))
        sum_abs += c * math.log(c)
        exact -= c * math.log(c)
        terms += 1
    t = np.float32(rv - 1)
    for p in ps:
        t = np.float32(t * np.float32(arity[p]))
    score = np.float32(score - np.float32(t * np.float32(math.log(N) / 2)))
    t64 = float(rv - 1) * q
    exact -= t64 * math.log(N) / 2
    sum_abs += t64 * math.log(N) / 2
    terms += 1
    ulp = float(np.spacing(np.float32(abs(exact))))
    bound = (terms + 2) * 2.0 ** -24 * sum_abs + ulp
    return score, exact, bound


def restated_lists(codes, arity, variables, candidates, max_parents, constraints=()):
    """Per variable: [(mask, float32 value, B)] in (|set|, set value) order, R3 / R5 / R6."""
    n = codes.shape[1]
    out = []
    for v, cand in zip(variables, candidates):
        cs = parents_of(cand & ((1 << n) - 1) & ~(1 << v))
        alts = [(r, f) for (cv, r, f) in constraints if cv == v]
        lst = []
        for L in range(0, min(len(cs), max_parents) + 1):
            masks = sorted(sum(1 << p for p in comb) for comb in itertools.combinations(cs, L))
            for m in masks:
                if alts and not any((r & ~m) == 0 and (m & f) == 0 for r, f in alts):
                    continue  # scores 1: never stored
                if arity[v] == 1:
                    if L == 0:
                        lst.append((m, np.float32(0.0), 0.0))
                    continue
                s, _, bnd = restated(codes, arity, v, m)
                if (L == 0 and s < 1) or (L > 0 and s < 0):
                    lst.append((m, s, bnd))
        out.append(lst)
    return out


def synthetic(n, N, arities, seed):
    """Seeded records with some dependence between neighbouring columns."""
    rng = np.random.default_rng(seed)
    codes = np.zeros((N, n), dtype=np.uint8)
    for j in range(n):
        col = rng.integers(0, arities[j], size=N)
        if j:
            follow = rng.random(N) < 0.4
            col = np.where(follow, codes[:, j - 1] % arities[j], col)
        codes[:, j] = col
    for j in range(n):  # every value present where N allows it
        k = min(N, arities[j])
        codes[:k, j] = np.arange(k)
    return codes


# ---- records_dump -------------------------------------------------------------
def _dump(exe, path, *opts):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe, str(path), *opts], capture_output=True, text=True, env=env, timeout=120)


def _parse(out):
    lines = out.splitlines()
    N, n = int(lines[0].split()[1]), int(lines[1].split()[1])
    names, arity = lines[2].split()[1:], [int(x) for x in lines[3].split()[1:]]
    codes = [[int(x) for x in ln.split()] for ln in lines[4:]]
    return N, n, names, arity, codes


@pytest.fixture(scope="module")
def san_dump():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/records_dump"], check=True, stdout=subprocess.DEVNULL)
    return SAN_DUMP


def _first_appearance(rows):
    """Codes by order of first appearance per column."""
    n = len(rows[0])
    maps = [dict() for _ in range(n)]
    return [[maps[c].setdefault(r[c], len(maps[c])) for c in range(n)] for r in rows], [len(m) for m in maps]


def _reader_cases(exe, tmp_path):
    text = [ln.strip().split(",") for ln in open(HEP).read().splitlines()]
    # with -s: the header names, 80 records
    r = _dump(exe, HEP, "-s")
    assert r.returncode == 0, r.stderr
    N, n, names, arity, codes = _parse(r.stdout)
    want_codes, want_arity = _first_appearance(text[1:])
    assert (N, n, names) == (80, 20, text[0])
    assert arity == want_arity and codes == want_codes
    # without -s the first line is a record: its tokens are values
    r2 = _dump(exe, HEP)
    assert r2.returncode == 0, r2.stderr
    N2, n2, names2, arity2, codes2 = _parse(r2.stdout)
    assert N2 == 81 and n2 == 20 and names2 == [f"Variable_{i}" for i in range(20)]
    assert arity2 == [a + 1 for a in arity]
    assert codes2[0] == [0] * 20 and codes2 == _first_appearance(text)[0]
    # a tab delimiter, leading and trailing blanks, first-appearance order
    p = tmp_path / "t.tsv"
    p.write_text("  a\tb\tc  \n z\tx\ty\n\tx\tx\ty\t\nz\tq\ty \n  x\tx\tw\n")
    r3 = _dump(exe, p, "-s", "-d", "\t")
    assert r3.returncode == 0, r3.stderr
    N3, n3, names3, arity3, codes3 = _parse(r3.stdout)
    assert (N3, n3, names3, arity3) == (4, 3, ["a", "b", "c"], [2, 2, 2])
    assert codes3 == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 1]]
    # a ragged row is an error naming its line
    q = tmp_path / "ragged.csv"
    q.write_text("a,b,c\n1,2,3\n4,5,6\n7,8\n1,2,3\n")
    r4 = _dump(exe, q, "-s")
    assert r4.returncode == 1 and "line 4" in r4.stderr
    r5 = _dump(exe, q)
    assert r5.returncode == 1 and "line 4" in r5.stderr


def test_records_dump(tmp_path):
    _reader_cases(DUMP, tmp_path)


def test_records_dump_under_sanitizers(san_dump, tmp_path):
    _reader_cases(san_dump, tmp_path)


# ---- the bound, before any GPU sees it -----------------------------------------
N6_ARITY = [2, 3, 4, 2, 3, 4]


def n6_case():
    return synthetic(6, 150, N6_ARITY, 20261019), N6_ARITY


def test_restatement_within_bound_of_fp64():
    codes, arity = n6_case()
    worst = 0.0
    smallest = math.inf
    rel = 0.0
    for v in range(6):
        others = [p for p in range(6) if p != v]
        for L in range(0, 4):
            for comb in itertools.combinations(others, L):
                m = sum(1 << p for p in comb)
                s, exact, bound = restated(codes, arity, v, m)
                assert abs(float(s) - exact) <= bound, (v, m, float(s), exact, bound)
                worst = max(worst, abs(float(s) - exact) / bound)
                smallest = min(smallest, abs(exact))
                rel = max(rel, bound / abs(exact))
    print(f"restatement used at most {worst:.3f} B; B <= {rel:.2e} |score|; smallest |score| {smallest:.1f}")
    # one miscounted record moves a score by about 1: B cannot hide it
    assert rel < 1e-4 and smallest > 10


def test_counts_table_layout():
    codes = np.array([[0, 1, 2], [1, 0, 2], [1, 1, 0], [0, 1, 2]], dtype=np.uint8)
    tab, q = counts_table(codes, [2, 2, 3], 1, 0b101)
    # parents 0 (base 1) and 2 (base 2), q = 6, child base 6
    assert q == 6 and tab.sum() == 4
    assert tab[0 + 2 * 2 + 1 * 6] == 2 and tab[1 + 2 * 2 + 0 * 6] == 1 and tab[1 + 0 * 2 + 1 * 6] == 1


# ---- command line refusals -------------------------------------------------------
@pytest.mark.parametrize("opts", [["-f", "fNML"], ["-f", "BIC", "--enableDeCamposPruning"],
                                  ["--enableDeCamposPruning"]])
def test_score_refuses_before_opening_a_file(opts, tmp_path):
    out = tmp_path / "out.pss"
    r = subprocess.run([SCORE, str(tmp_path / "no_such_in.csv"), str(out), *opts], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert "cBIC" in r.stderr and "BIC" in r.stderr.replace("cBIC", "")
    assert "cannot read" not in r.stderr and not out.exists()


def test_score_bic_needs_two_records(tmp_path):
    """R2: the reference divides by log 1 at N = 1; refused before any GPU work."""
    p = tmp_path / "one.csv"
    p.write_text("a,b\n0,1\n")
    r = subprocess.run([SCORE, str(p), str(tmp_path / "o.pss"), "-s"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "at least 2 records" in r.stderr
    q = tmp_path / "ragged.csv"
    q.write_text("a,b\n0,1\n1\n")
    r = subprocess.run([SCORE, str(q), str(tmp_path / "o.pss"), "-s"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "line 3" in r.stderr
