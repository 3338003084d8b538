"""`score --prune` / option "disc_prune" on the CPU: the rule (DESIGN R8), its
literal restatement, the subset-rank check program and the command line's
refusals.

The reference's prune() (scoring_function/score_calculator.cpp:137-197) sorts a
variable's (set, score) pairs with compareSecond -- higher score first, scores
within 2 * FLT_EPSILON (float arithmetic) equal and then the smaller varset
first -- and lets every set not yet erased erase all later supersets.
prune_literal() restates exactly that; prune_rule() is the form the GPU
implements: a stored set P goes iff a kept proper subset Q has
(float)(s(Q) - s(P)) >= -2 FLT_EPSILON.  The two agree wherever the comparator
is a strict weak order, i.e. where a float ulp is not below 2 FLT_EPSILON:
|score| >= 4, which every input here is asserted to satisfy.

test_gpu_disc_prune.py applies prune_rule() to the lists the GPU stored without
pruning and requires the pruned call's lists to equal the result bit for bit."""
import functools
import itertools
import os
import subprocess

import numpy as np

from conftest import PKG
from test_discrete import exact_value, n6_case, parents_of, synthetic

SCORE = os.path.join(PKG, "bin", "score")
CHECK = os.path.join(PKG, "bin", "prune_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "prune_check")

TWO_EPS = np.float32(2.0) * np.finfo(np.float32).eps
assert float(TWO_EPS) == 2.0 ** -22  # 2.3841858e-07f


# ---- the rule -----------------------------------------------------------------
def prune_rule(masks, scores):
    """One variable's stored list (any order in which a set follows its subsets; the scorer's is
    (|set|, set value)) -> the kept positions, ascending.  scores: float32."""
    masks = [int(m) for m in masks]
    sc = np.asarray(scores, dtype=np.float32)
    km = np.zeros(len(masks), dtype=np.uint64)
    ks = np.zeros(len(masks), dtype=np.float32)
    k = 0
    kept = []
    for pos, (m, s) in enumerate(zip(masks, sc)):
        sub = ((km[:k] & np.uint64(~m & (2 ** 64 - 1))) == 0) & (km[:k] != np.uint64(m))  # kept proper subsets
        if k and np.any((ks[:k][sub] - s) >= -TWO_EPS):  # float32 - float32
            continue
        km[k], ks[k] = m, s
        k += 1
        kept.append(pos)
    return kept


def prune_literal(masks, scores):
    """prune() as written: sort with compareSecond, then scan -> the kept positions, ascending."""
    sc = np.asarray(scores, dtype=np.float32)

    def first(a, b):  # compareSecond(lhs, rhs)
        val = np.float32(sc[a] - sc[b])
        if abs(val) > TWO_EPS:
            return val > 0
        return int(masks[a]) < int(masks[b])

    def cmp(a, b):
        return -1 if first(a, b) else (1 if first(b, a) else 0)

    order = sorted(range(len(masks)), key=functools.cmp_to_key(cmp))
    gone = [False] * len(order)
    for i, a in enumerate(order):
        if gone[i]:
            continue
        pi = int(masks[a])
        for j in range(i + 1, len(order)):
            if not gone[j] and (pi & ~int(masks[order[j]])) == 0:  # VARSET_IS_SUBSET_OF(pi, pj)
                gone[j] = True
    return sorted(order[i] for i in range(len(order)) if not gone[i])


def apply_rule(offs, sets, scores):
    """prune_rule on fetched lists -> (offsets, sets, scores) of the kept sets, same dtypes."""
    keep, new_offs = [], [0]
    for i in range(len(offs) - 1):
        lo, hi = int(offs[i]), int(offs[i + 1])
        keep += [lo + p for p in prune_rule(sets[lo:hi], scores[lo:hi])]
        new_offs.append(len(keep))
    keep = np.asarray(keep, dtype=np.int64)
    return np.asarray(new_offs, dtype=offs.dtype), sets[keep], scores[keep]


# ---- inputs ---------------------------------------------------------------------
XOR8_ARITY = [2, 2, 3, 2, 3, 2, 2, 4]


@functools.lru_cache(maxsize=None)
def xor8(N, seed):
    """The parity input: column 5 follows the parity of columns 0, 1, 3 and column 6 that of
    2, 4, 1, 7, so no single parent or pair explains them and three or four parents do."""
    rng = np.random.default_rng(seed)
    c = [rng.integers(0, a, N) for a in XOR8_ARITY]
    c[5] = np.where(rng.random(N) >= 0.1, (c[0] + c[1] + c[3]) % 2, c[5])
    c[6] = np.where(rng.random(N) >= 0.15, (c[2] + c[4] + c[1] + c[7]) % 2, c[6])
    codes = np.stack(c, axis=1).astype(np.uint8)
    for j, a in enumerate(XOR8_ARITY):
        codes[:a, j] = np.arange(a)
    codes.setflags(write=False)
    return codes, list(XOR8_ARITY)


def stored_lists(codes, arity, k):
    """Per variable, full candidates: the (mask, float32 value) the scorer stores (R3), in its order."""
    n = codes.shape[1]
    out = []
    for v in range(n):
        others = [p for p in range(n) if p != v]
        lst = []
        for L in range(k + 1):
            for m in sorted(sum(1 << p for p in comb) for comb in itertools.combinations(others, L)):
                s = np.float32(exact_value(codes, arity, v, m)[0])
                if (L == 0 and s < 1) or (L > 0 and s < 0):
                    lst.append((m, s))
        out.append(lst)
    return out


def _both(lists):
    kept = []
    for lst in lists:
        masks, scores = [m for m, _ in lst], [s for _, s in lst]
        assert all(abs(float(s)) >= 4 for s in scores)  # the comparator's strict-weak-order domain
        rule, literal = prune_rule(masks, scores), prune_literal(masks, scores)
        assert rule == literal
        kept.append([masks[p] for p in rule])
    return kept


def test_rule_equals_literal_on_n6():
    codes, arity = n6_case()
    lists = stored_lists(codes, arity, 3)
    kept = _both(lists)
    assert sum(len(x) for x in lists) == 156
    assert [len(x) for x in kept] == [2, 3, 3, 4, 3, 3] and sum(len(x) for x in kept) == 18


def test_rule_equals_literal_on_the_parity_input():
    codes, arity = xor8(1500, 11)
    lists = stored_lists(codes, arity, 4)
    kept = _both(lists)
    assert sum(len(x) for x in lists) == 792 and sum(len(x) for x in kept) == 17
    sizes = [len(parents_of(m)) for x in kept for m in x]
    assert {s: sizes.count(s) for s in set(sizes)} == {0: 8, 3: 4, 4: 5}
    # B travels two layers through pruned sets: something large is kept, nothing of size 1 or 2
    assert max(sizes) >= 3 and not any(s in (1, 2) for s in sizes)


def test_rule_equals_literal_on_synthetic8():
    codes = synthetic(8, 2000, [2, 3, 2, 4, 3, 2, 3, 2], 7)
    lists = stored_lists(codes, [2, 3, 2, 4, 3, 2, 3, 2], 4)
    kept = _both(lists)
    assert sum(len(x) for x in lists) == 792 and sum(len(x) for x in kept) == 53


def test_rule_sees_through_sets_that_are_not_stored():
    """Only stored sets dominate, but domination passes through the holes: {} prunes {a, b} with
    neither {a} nor {b} in the list."""
    masks, scores = [0, 0b011, 0b100], np.array([-100.0, -100.5, -99.0], dtype=np.float32)
    assert prune_rule(masks, scores) == prune_literal(masks, scores) == [0, 2]
    # within 2 FLT_EPSILON counts as equal: the subset wins
    near = np.array([-100.0, np.nextafter(np.float32(-100.0), np.float32(0)), -100.0], dtype=np.float32)
    assert near[1] > near[0] and prune_rule([0, 0b01, 0b10], near) == prune_literal([0, 0b01, 0b10], near) == [0, 1]


# ---- the subset ranks of the kernel -------------------------------------------
def test_prune_check():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "prune_check ok" in r.stdout, (r.stdout, r.stderr)


def test_prune_check_under_sanitizers():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/prune_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "prune_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- command line ---------------------------------------------------------------
def test_score_refuses_prune_for_cbic_before_opening_a_file(tmp_path):
    out = tmp_path / "out.pss"
    r = subprocess.run([SCORE, str(tmp_path / "no_such_in.csv"), str(out), "-f", "cBIC", "--prune"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert "--prune" in r.stderr and "dominance" in r.stderr and "continuous" in r.stderr
    assert "cannot read" not in r.stderr and not out.exists()


def test_score_help_lists_prune():
    r = subprocess.run([SCORE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--prune" in r.stdout + r.stderr
