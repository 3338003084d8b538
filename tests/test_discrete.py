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
with T = the number of terms added or subtracted.

The kernel's own bound.  B is the error of the reference's float32 summation.
The kernel promises more: the exactly summed FP64 value, rounded to float once
(csrc/disc_dev.h, item_value in csrc/disc.hip).  exact_value() below restates
that value without walking the cells (numpy.unique on the 64-bit cell index,
math.fsum), so it also serves tables far too large to enumerate, and returns
(exact64, T, A): the value, the number T of n ln n terms (non-empty cells plus
non-empty parent configurations) and A = sum |n ln n|.  With pen =
(r_v - 1) q ln(N) / 2 the kernel's float differs from exact64 by at most
    Bk = ulp_f32(exact64) / 2 + T 2^-(shift+1) + (T + 3) 2^-52 (A + pen),
term by term:
  * T 2^-(shift+1): fix_nlogn rounds each of the T terms to a multiple of
    2^-shift once; the integer sum of those is exact.
  * the FP64 part.  The kernel: each term is the device's log (two ulps,
    relative 2^-51) times n (one rounding, 2^-53): 3 2^-52 A; the int64 sum
    converted to double, (double)q, the two products of the penalty and the
    subtraction ll - pen are one rounding each: at most 2 2^-52 (A + pen)
    together.  This restatement: numpy's log (one ulp) and the product, 2^-52 A;
    the penalty's two roundings and fsum's single one, 2^-52 (A + pen).  That is
    6 2^-52 (A + pen) in all, which (T + 3) 2^-52 (A + pen) covers from T = 3 on
    (T = 2 happens only for a column with a single value, where both sides give
    exactly 0).
  * ulp_f32(exact64) / 2: the one rounding to float.  Where the FP64 sum lies
    within the two terms above of a float rounding boundary, the float may fall
    on the boundary's other side; it is then still within ulp / 2 of the
    kernel's FP64 sum, hence within ulp / 2 plus those two terms of exact64.
The tests assert ulp_f32(exact64) / 2 + 2 (T 2^-(shift+1) + (T + 3) 2^-52 (A + pen)),
the doubled small terms standing for that last case.  shift is disc_data()'s:
min(32, 62 - exponent of N ln N).  Nothing in Bk is measured.

What Bk can see.  For tables of up to 10^6 cells Bk stays below 1e-3 of the
smallest |score| of every input the GPU shape tests use, and one record moved
to another cell changes a score by about 1, so a miscounted record cannot hide
(test_kernel_bound_resolves_one_record).  Beyond that the penalty
(r_v - 1) q ln(N) / 2 grows with q while the log-likelihood stays below
N ln N, and half an ulp of the float32 result swamps the log-likelihood: those
cases check the table's shape, the 64-bit q and -- where the counts are read
back -- the counts, not the log-likelihood."""
import functools
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


def exact_from_counts(njk, nj, rv, q, N):
    """(exact64, T, A) from the non-empty cell counts njk and parent-configuration counts nj."""
    njk = np.asarray(njk, dtype=np.float64)
    nj = np.asarray(nj, dtype=np.float64)
    plus, minus = njk * np.log(njk), nj * np.log(nj)
    pen = float((rv - 1) * q) * math.log(N) / 2
    exact = math.fsum(itertools.chain(plus.tolist(), (-minus).tolist(), [-pen]))
    return exact, int(njk.size + nj.size), math.fsum(plus.tolist()) + math.fsum(minus.tolist())


def exact_value(codes, arity, v, mask):
    """The value the kernel promises, in FP64: sum n_jk ln n_jk - sum n_j ln n_j - (r_v - 1) q ln(N) / 2
    over the non-empty cells and parent configurations -> (exact64, T, A), see the module docstring.
    Never allocates q r_v entries; q r_v < 2^63 (the scorer refuses anything larger)."""
    N = codes.shape[0]
    ps = parents_of(mask & ~(1 << v))
    cfg = np.zeros(N, dtype=np.int64)
    q = 1
    for p in ps:
        cfg += codes[:, p].astype(np.int64) * q
        q *= int(arity[p])
    rv = int(arity[v])
    assert q * rv < 2 ** 63
    cell = cfg + codes[:, v].astype(np.int64) * q
    njk = np.unique(cell, return_counts=True)[1]
    nj = np.unique(cfg, return_counts=True)[1]
    return exact_from_counts(njk, nj, rv, q, N)


def exact_value_batch(codes, arity, v, parent_sets):
    """exact_value for many parent sets of v at once: parent_sets is an S x L array of parent indices,
    ascending in each row, every column involved of arity <= 2 -> (exact64[S], T[S], A[S]).  One
    bincount over set_id * cells + cell; the row sums are plain FP64 sums (at most 48 terms of size
    <= N ln N with N a few dozen: their rounding is ~1e-14, far inside Bk)."""
    ps = np.asarray(parent_sets, dtype=np.int64).reshape(len(parent_sets), -1)
    S, L = ps.shape
    ar = np.asarray(arity, dtype=np.int64)
    assert ar[v] <= 2 and (S == 0 or L == 0 or ar[ps].max() <= 2)
    N = codes.shape[0]
    c = codes.astype(np.int64)
    cfg = np.zeros((S, N), dtype=np.int64)
    for a in range(L):
        cfg += c[:, ps[:, a]].T << a
    q2 = 1 << L
    row = np.arange(S, dtype=np.int64)[:, None]
    njk = np.bincount((row * (2 * q2) + cfg + c[:, v][None, :] * q2).ravel(), minlength=S * 2 * q2)
    nj = np.bincount((row * q2 + cfg).ravel(), minlength=S * q2)

    def nlogn(x, width):
        x = x.reshape(S, width).astype(np.float64)
        return np.where(x > 0, x * np.log(np.maximum(x, 1.0)), 0.0).sum(axis=1), (x > 0).sum(axis=1)

    (plus, tp), (minus, tm) = nlogn(njk, 2 * q2), nlogn(nj, q2)
    q = ar[ps].prod(axis=1)
    pen = ((int(ar[v]) - 1) * q).astype(np.float64) * math.log(N) / 2
    return plus - minus - pen, tp + tm, plus + minus


def disc_shift(N):
    """disc_data()'s fixed-point scale (csrc/disc_dev.h)."""
    return min(32, 62 - math.frexp(N * math.log(N))[1])


def ulp_f32(x):
    """The spacing of float32 at |x| (x a double, normal range)."""
    return math.ldexp(1.0, max(math.frexp(abs(float(x)))[1], -125) - 24)


def kernel_bound(exact, T, A, rv, q, N):
    """What the GPU tests allow between the kernel's float and exact64 (module docstring)."""
    pen = float((rv - 1) * q) * math.log(N) / 2
    return ulp_f32(exact) / 2 + 2.0 * (T * 2.0 ** -(disc_shift(N) + 1) + (T + 3) * 2.0 ** -52 * (A + pen))


def q_of(arity, v, mask):
    q = 1
    for p in parents_of(mask & ~(1 << v)):
        q *= int(arity[p])
    return q


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


# ---- the kernel's own bound, and the inputs of test_gpu_discrete_shapes.py ------------
def pairs_up_to(n, variables, k):
    """Every (v, parent mask) with at most k parents out of the other n - 1 variables."""
    vs, ps = [], []
    for v in variables:
        others = [p for p in range(n) if p != v]
        for L in range(k + 1):
            for comb in itertools.combinations(others, L):
                vs.append(v)
                ps.append(sum(1 << p for p in comb))
    return vs, ps


def _mask(*ps):
    return sum(1 << p for p in ps)


def combos(items, L):
    """The L-subsets of items as an S x L array (one empty row for L = 0)."""
    return np.array(list(itertools.combinations(items, L)), dtype=np.int64).reshape(math.comb(len(items), L), L)


ARITY_A = [4, 4, 4, 4, 4, 4, 4, 3]
# (v, parents): 192, 768, 1024 (q = 256), 3072, 4096 (q = 1024), 12288 (q = 4096), 12288 (q = 3072),
# 16384 (q = 4096) and two of 49152 cells
SETS_A = [(7, _mask(0, 1, 2)), (7, _mask(0, 1, 2, 3)), (0, _mask(1, 2, 3, 4)), (7, _mask(0, 1, 2, 3, 4)),
          (0, _mask(1, 2, 3, 4, 5)), (7, _mask(0, 1, 2, 3, 4, 5)), (0, _mask(1, 2, 3, 4, 5, 7)),
          (0, _mask(1, 2, 3, 4, 5, 6)), (7, _mask(0, 1, 2, 3, 4, 5, 6)), (0, _mask(1, 2, 3, 4, 5, 6, 7))]
ARITY_A2 = [2] * 15 + [3]
# 16384, 24576, 32768 (the option's maximum), 49152 and 98304 cells
SETS_A2 = [(0, _mask(*range(1, 14))), (15, _mask(*range(0, 13))), (0, _mask(*range(1, 15))),
           (15, _mask(*range(0, 14))), (0, _mask(*range(1, 16)))]
# test_a_dense_limit_at_its_maximum also lists all 2^14 parent sets of variable 0 among the binary
# columns and holds these positions of the list (layers ascending, masks ascending) to Bk
CAND_A2 = _mask(*range(1, 15))
SAMPLE_A2 = [0, 1, 200, 5000] + list(range((1 << 14) - 15, 1 << 14))
ARITY_B = ARITY_A + [255] * 6 + [200]
# 13,005,000 cells; 2.08e8 cells; q = 255^5 * 200, 5.5e16 cells
SETS_B = [(8, _mask(9, 14)), (0, _mask(1, 8, 9, 14)), (8, _mask(9, 10, 11, 12, 13, 14))]
# the same records in tables small enough for the histogram: 1020, 3200, 1020 and 3060 cells
SMALL_B = [(8, _mask(0)), (14, _mask(1, 2)), (0, _mask(8)), (9, _mask(3, 7))]
ARITY_C = [2, 3, 4, 5, 2, 3, 4, 5, 6, 7]
ARITY_D = [3] * 6
ARITY_E = [1 if j in (7, 19) else 2 for j in range(30)]
ARITY_F = [(2, 3, 2, 4)[j % 4] for j in range(44)]
ARITY_F63 = [(2, 3, 2, 4)[j % 4] for j in range(63)]
VARS_F = [3, 10, 21, 30, 33, 38, 40, 43]
CAND_F = _mask(26, 28, 29, 30, 31, 32, 33, 35, 37, 40, 41, 43)
ARITY_G = [3, 4]
N_G = 62_000_000


def pairs_f():
    """200 seeded pairs with one to four parents among the variables 30..43."""
    rng = np.random.default_rng(44)
    vs, ps = [], []
    for _ in range(200):
        par = rng.choice(np.arange(30, 44), size=int(rng.integers(1, 5)), replace=False)
        v = int(rng.choice([x for x in range(44) if x not in par]))
        vs.append(v)
        ps.append(_mask(*[int(p) for p in par]))
    return vs, ps


@functools.lru_cache(maxsize=None)
def shape_input(name):
    """The inputs of the GPU shape tests -> (codes, arity): built once per session, never modified."""
    if name == "g":
        rng = np.random.default_rng(62)
        codes = np.empty((N_G, 2), dtype=np.uint8)
        for j, r in enumerate(ARITY_G):
            codes[:, j] = rng.integers(0, r, size=N_G, dtype=np.uint8)
            codes[:r, j] = np.arange(r)
        arity = ARITY_G
    else:
        n_N_arity_seed = {"a": (3000, ARITY_A, 81), "a2": (3000, ARITY_A2, 82), "b1500": (1500, ARITY_B, 83),
                          "b2100": (2100, ARITY_B, 84), "c300": (300, ARITY_C, 85), "c2100": (2100, ARITY_C, 86),
                          "d": (20000, ARITY_D, 87), "e": (16, ARITY_E, 88), "f": (500, ARITY_F, 89),
                          "f63": (200, ARITY_F63, 90)}
        N, arity, seed = n_N_arity_seed[name]
        codes = synthetic(len(arity), N, arity, seed)
    assert all(len(np.unique(codes[:, j])) == arity[j] for j in range(len(arity)))  # every value present
    codes.setflags(write=False)
    return codes, list(arity)


def list_order(candidates, k):
    """The parent masks of one variable's list in the order ulg_disc_score stores them."""
    return [m for L in range(min(len(candidates), k) + 1)
            for m in sorted(_mask(*comb) for comb in itertools.combinations(candidates, L))]


def shape_pairs(name):
    """The (variable, parent mask) pairs the GPU shape tests score on shape_input(name)."""
    if name == "a":  # and the lists of variables 7 and 0 with every other column a candidate
        vs, ps = pairs_up_to(8, [7, 0], 7)
        return [v for v, _ in SETS_A] + vs, [m for _, m in SETS_A] + ps
    if name == "a2":
        order = list_order(parents_of(CAND_A2), 14)
        return [v for v, _ in SETS_A2] + [0] * len(SAMPLE_A2), [m for _, m in SETS_A2] + [order[i] for i in SAMPLE_A2]
    if name in ("b1500", "b2100"):
        return [v for v, _ in SETS_B + SMALL_B], [m for _, m in SETS_B + SMALL_B]
    if name in ("c300", "c2100"):
        return pairs_up_to(10, range(10), 4)
    if name == "d":
        return pairs_up_to(6, range(6), 5)
    if name == "f":
        vs, ps = pairs_f()
        for v in VARS_F:
            cs = parents_of(CAND_F & ~(1 << v))
            for L in range(4):
                for comb in itertools.combinations(cs, L):
                    vs.append(v)
                    ps.append(_mask(*comb))
        return vs, ps
    if name == "f63":
        return [0, 62, 5], [_mask(31, 62), _mask(0, 61), _mask(62)]
    if name == "g":
        return [0, 1, 0, 1], [0, 0, 2, 1]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def g_joint(rows=None):
    codes = shape_input("g")[0][:rows]
    return np.bincount(codes[:, 0] + np.uint8(3) * codes[:, 1], minlength=12).reshape(4, 3)  # [code 1][code 0]


def g_counts(v, m, rows=None):
    """Input g's dense table of (v, m) in the kernel's layout (counts_table's) and its q, from one pass
    over the records; rows: only the first so many."""
    joint = g_joint(rows)
    if m & ~(1 << v) == 0:
        return joint.sum(axis=v).astype(np.int64), 1
    return (joint.T if v == 0 else joint).ravel().astype(np.int64), ARITY_G[1 - v]


def test_exact_value_equals_restatement():
    codes, arity = n6_case()
    vs, ps = pairs_up_to(6, range(6), 3)
    assert len(vs) == 156
    for v, m in zip(vs, ps):
        want = restated(codes, arity, v, m)[1]
        got, T, A = exact_value(codes, arity, v, m)
        assert abs(got - want) <= 1e-9 * abs(want), (v, m, got, want)
        tab, q = counts_table(codes, arity, v, m)
        assert T == int((tab > 0).sum() + (tab.reshape(-1, q).sum(axis=0) > 0).sum()) and A > 0


def test_exact_value_batch_equals_scalar():
    rng = np.random.default_rng(30)
    codes = rng.integers(0, 2, size=(16, 30)).astype(np.uint8)
    codes[:2, :] = [[0], [1]]
    arity = [2] * 30
    for L, count in ((0, 1), (1, 50), (2, 100), (3, 150), (4, 200)):  # the empty set and 500 random sets
        v = int(rng.integers(0, 30))
        others = [p for p in range(30) if p != v]
        sets = np.array([sorted(rng.choice(others, size=L, replace=False)) for _ in range(count)], dtype=np.int64)
        ex, T, A = exact_value_batch(codes, arity, v, sets.reshape(count, L))
        for i in range(count):
            e1, T1, A1 = exact_value(codes, arity, v, _mask(*[int(p) for p in sets[i]]))
            assert abs(ex[i] - e1) <= 1e-12 * abs(e1) and T[i] == T1 and abs(A[i] - A1) <= 1e-12 * max(A1, 1.0)
    # columns with a single value: they count in q as 1 and leave every count alone
    codes_e, arity_e = shape_input("e")
    sets = np.array([[3, 7, 19, 22], [0, 1, 7, 29]])
    ex, T, A = exact_value_batch(codes_e, arity_e, 5, sets)
    for i in range(2):
        e1, T1, A1 = exact_value(codes_e, arity_e, 5, _mask(*[int(p) for p in sets[i]]))
        assert abs(ex[i] - e1) <= 1e-12 * abs(e1) and T[i] == T1
    assert exact_value_batch(codes_e, arity_e, 7, sets[:, [0, 2]])[0].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("name", ["a", "a2", "b1500", "b2100", "c300", "c2100", "d", "e", "f", "f63", "g"])
def test_kernel_bound_resolves_one_record(name):
    """Bk < 1e-3 of the smallest |score| over every table of at most 10^6 cells the GPU shape tests
    hold to Bk on this input (shape_pairs; of input e's 835,230 sets, all those of three variables)."""
    codes, arity = shape_input(name)
    N = codes.shape[0]
    rel, smallest = 0.0, math.inf
    if name == "e":
        for v in (0, 13, 29):
            others = [p for p in range(30) if p != v]
            for L in range(5):
                sets = combos(others, L)
                ex, T, A = exact_value_batch(codes, arity, v, sets)
                q = np.asarray(arity)[sets].prod(axis=1)
                bk = np.array([kernel_bound(e, int(t), float(a), 2, int(qq), N) for e, t, a, qq in zip(ex, T, A, q)])
                rel, smallest = max(rel, float((bk / np.abs(ex)).max())), min(smallest, float(np.abs(ex).min()))
    else:
        for v, m in zip(*shape_pairs(name)):
            q = q_of(arity, v, m)
            if q * arity[v] > 10 ** 6:
                continue
            if name == "g":  # exact_value's sort of 62e6 indices takes a minute; the counts are the same
                tab, _ = g_counts(v, m)
                want, _ = counts_table(codes[:5000], arity, v, m)
                assert np.array_equal(g_counts(v, m, 5000)[0], want) and tab.sum() == N
                nj = tab.reshape(-1, q).sum(axis=0)
                ex, T, A = exact_from_counts(tab[tab > 0], nj[nj > 0], arity[v], q, N)
            else:
                ex, T, A = exact_value(codes, arity, v, m)
            rel = max(rel, kernel_bound(ex, T, A, arity[v], q, N) / abs(ex))
            smallest = min(smallest, abs(ex))
    print(f"{name}: Bk <= {rel:.2e} |score|, smallest |score| {smallest:.1f}")
    assert rel < 1e-3 and smallest > 1


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
