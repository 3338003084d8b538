"""BGe on the CPU (ulg_bge_*, `score --bge`): the long-double reference of
bge_ref.py against the score's own identities, the kernel's operation order in
plain FP64 against that reference on every input test_gpu_bge.py uses, the
constants of csrc/bge.h (bin/bge_check), the prune rule on BGe values and the
command line's refusals.

The bound of test_kernel_order_is_within_a_thousandth_of_a_float_ulp is what
test_gpu_bge.py's tolerance rests on: a GPU value is the FP64 result of that
order rounded to float once, so it lies within 1/2 + 1e-3 float32 ulps of the
reference, i.e. within 1 ulp of float32(reference)."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import bge_ref
from bge_ref import LD, case, consts, list_order, ref, ulp32
from conftest import PKG
from test_disc_prune import prune_literal, prune_rule

SCORE = os.path.join(PKG, "bin", "score")
CHECK = os.path.join(PKG, "bin", "bge_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "bge_check")

# (input, alpha_mu, alpha_w, largest set): the data sets and priors of test_gpu_bge.py
GPU_INPUTS = [("n10_N8", 1.0, None, 9), ("n10_N50", 1.0, None, 9), ("n10_N1000", 1.0, None, 9), ("n32", 1.0, None, 31),
              ("n63", 1.0, None, 6), ("mixed", 1.0, None, 12), ("n20", 1.0, None, 6), ("illcond", 1.0, None, 7),
              ("c3like", 1.0, None, 7), ("const", 1.0, None, 5), ("sum", 1.0, None, 5), ("e2e", 1.0, None, 5),
              ("prior", 0.1, 13.0, 7)]


def sample_sets(n, kmax, per_size=12, seed=5):
    """Up to per_size sets of every size 0 .. kmax for up to six variables, the first and last in colex order among them."""
    rng = np.random.default_rng(seed)
    vs, ms = [], []
    for v in sorted(set([0, 1, n // 2, n - 2, n - 1]) & set(range(n))):
        others = [p for p in range(n) if p != v]
        for L in range(min(kmax, n - 1) + 1):
            picks = {tuple(others[:L]), tuple(others[len(others) - L:])}
            while len(picks) < min(per_size, math.comb(len(others), L)):
                picks.add(tuple(sorted(rng.choice(others, L, replace=False).tolist())))
            for P in sorted(picks):
                vs.append(v)
                ms.append(sum(1 << p for p in P))
    return vs, ms


# ---- the reference against the score's identities -----------------------------------
@pytest.mark.parametrize("name,am,aw", [("prior", 1.0, None), ("prior", 0.1, 13.0), ("e2e", 1.0, None), ("n10_N8", 1.0, None)])
def test_reference_is_score_equivalent(name, am, aw):
    """s(y | x) + s(x) = s(x | y) + s(y) for every pair, and covered edges in general:
    s(y | Z + x) + s(x | Z) = s(x | Z + y) + s(y | Z), to 1e-12 relative."""
    r = ref(name, am, aw)
    n = r.n
    for x, y in itertools.combinations(range(min(n, 6)), 2):
        rest = [z for z in range(n) if z not in (x, y)]
        for Z in (0, *(1 << z for z in rest[:3]), sum(1 << z for z in rest)):
            a = r.score(y, Z | 1 << x) + r.score(x, Z)
            b = r.score(x, Z | 1 << y) + r.score(y, Z)
            assert abs(a - b) <= 1e-12 * max(abs(a), 1), (x, y, Z, float(a), float(b))


def test_reference_is_order_invariant():
    """Every order of a complete DAG over the same variables has the same total."""
    for name, m in (("prior", 4), ("sum", 4)):
        r = ref(name)
        totals = []
        for o in itertools.permutations(range(m)):
            totals.append(sum(r.score(o[i], sum(1 << p for p in o[:i])) for i in range(m)))
        assert len(totals) == 24
        assert max(totals) - min(totals) <= 1e-12 * abs(totals[0])


def test_pivot_form_equals_the_determinant_form():
    """c_l - 1/2 ln det R[P,P] - A_l ln sigma = c_l - A_l ln det R[Q,Q] + (A_l - 1/2) ln det R[P,P], the
    determinants from numpy's FP64 slogdet of the two blocks.  'prior' is well conditioned (kappa < 1e3),
    so slogdet is good to about 1e-13 relative in each ln det; A_l is about N / 2."""
    for am, aw in ((1.0, None), (0.1, 13.0)):
        r = ref("prior", am, aw)
        R = r.R.astype(np.float64)
        vs, ms = sample_sets(r.n, 7, per_size=6)
        got = r.scores(vs, ms)
        for v, m, g in zip(vs, ms, got):
            P = bge_ref.members(m)
            Q = P + [v]
            c, A, _ = r.consts(len(P))
            sq, ldq = np.linalg.slogdet(R[np.ix_(Q, Q)])
            sp, ldp = np.linalg.slogdet(R[np.ix_(P, P)]) if P else (1.0, 0.0)
            assert sq == 1.0 and sp == 1.0
            want = c - A * ldq + (A - 0.5) * ldp
            assert abs(float(g) - want) <= 1e-10 * max(abs(want), 1.0), (v, m, float(g), want)


def test_no_sign_rule_is_needed_for_nothing():
    """The departure from the reference's store rule has inputs behind it: duplicated and near-deterministic
    columns give positive scores, the empty sets included nowhere (a normalised column alone is never that good)."""
    for name in ("illcond", "sum", "e2e", "c3like"):
        r = ref(name)
        vs, ms = sample_sets(r.n, 4)
        s = r.scores(vs, ms)
        assert np.all(np.isfinite(s.astype(np.float64)))
        assert np.any(s > 0), name
    r = ref("sum")
    assert r.score(5, 0b000111) > 0 > r.score(5, 0b000011) and r.score(5, 0) < 0


def test_constant_column_is_nan_iff_touched():
    r = ref("const")
    vs, ms = [], []
    for v in range(6):
        for m in list_order([p for p in range(6) if p != v], 5):
            vs.append(v)
            ms.append(m)
    s = r.scores(vs, ms)
    for v, m, x in zip(vs, ms, s):
        assert bool(np.isnan(x)) == (v == 2 or bool(m >> 2 & 1)), (v, m)


# ---- the kernel's order in FP64 -------------------------------------------------------
@pytest.mark.parametrize("name,am,aw,kmax", GPU_INPUTS, ids=[g[0] for g in GPU_INPUTS])
def test_kernel_order_is_within_a_thousandth_of_a_float_ulp(name, am, aw, kmax):
    r = ref(name, am, aw)
    vs, ms = sample_sets(r.n, kmax, per_size=8 if kmax > 9 else 12)
    want = r.scores(vs, ms)
    worst = 0.0
    for v, m, w in zip(vs, ms, want):
        got = r.kernel_order(v, m)
        if np.isnan(w):
            assert math.isnan(got), (v, m)
            continue
        worst = max(worst, abs(float(w - LD(got))) / ulp32(w))
    print(f"{name}: {len(vs)} sets, FP64 kernel order at most {worst:.3g} float32 ulps from the long-double reference")
    assert worst <= 1e-3


# ---- the constants ------------------------------------------------------------------------
def test_bge_check():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bge_check ok" in r.stdout, (r.stdout, r.stderr)


def test_bge_check_under_sanitizers():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/bge_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "bge_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("N,n,am,aw", [(8, 10, 1.0, 0.0), (1000, 10, 1.0, 0.0), (10000, 25, 1.0, 0.0), (600, 8, 0.1, 13.0),
                                       (150, 63, 1e-3, 0.0), (200, 32, 1e3, 32 + 1e6)])
def test_constants_table(N, n, am, aw):
    """c_l, A_l and t as the library computes them against bge_ref.consts.  Both sum the same five terms
    in FP64; the bound is 16 ulps of the largest of them."""
    r = subprocess.run([CHECK, str(N), str(n), repr(am), repr(aw)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    t = float(lines[0].split()[1])
    assert abs(t - consts(N, n, am, aw, 0)[2]) <= 4 * 2.0 ** -52 * t
    awe = aw or n + am + 1
    for l in range(32):
        tok = lines[1 + l].split()
        assert int(tok[0]) == l
        c, A, _ = consts(N, n, am, aw, l)
        big = max(abs(math.lgamma(A)), abs(math.lgamma((awe - n + l + 1) / 2)), N / 2 * math.log(math.pi),
                  abs((awe - n + 2 * l + 1) / 2 * math.log(t)), 1.0)
        assert abs(float(tok[1]) - c) <= 16 * 2.0 ** -52 * big, (l, tok[1], c)
        assert float(tok[2]) == A


def test_bge_check_refuses_a_prior_out_of_range():
    for bad in (("100", "10", "0", "0"), ("100", "10", "1", "11"), ("100", "10", "1", "5"), ("100", "10", "nan", "0")):
        r = subprocess.run([CHECK, *bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, bad


# ---- the prune rule on BGe values -------------------------------------------------------
@pytest.mark.parametrize("name", ["prior", "e2e", "sum"])
def test_prune_rule_equals_literal_on_bge_values(name):
    """test_disc_prune's rule and the literal prune() agree on BGe lists (every finite value stored), in the
    comparator's strict-weak-order domain |score| >= 4."""
    r = ref(name)
    kept_total = stored = 0
    for v in range(r.n):
        masks = list_order([p for p in range(r.n) if p != v], 3)
        scores = r.scores([v] * len(masks), masks).astype(np.float32)
        assert np.all(np.isfinite(scores)) and np.all(np.abs(scores) >= 4)
        rule = prune_rule(masks, scores)
        assert rule == prune_literal(masks, scores)
        assert 0 in rule  # the empty set has no subset
        kept_total += len(rule)
        stored += len(masks)
    assert 0 < kept_total < stored


# ---- command line ---------------------------------------------------------------------------
@pytest.mark.parametrize("extra,words", [
    (["--bdeu"], ["--bge", "--bdeu"]),
    (["--fnml"], ["--bge", "--fnml"]),
    (["-f", "cBIC"], ["--bge", "-f cBIC"]),
    (["--enableDeCamposPruning"], ["--enableDeCamposPruning", "--bge"]),
    (["--alpha-mu", "0"], ["--alpha-mu"]),
    (["--alpha-mu", "1e4"], ["--alpha-mu"]),
    (["--alpha-mu", "nan"], ["--alpha-mu"]),
    (["--alpha-w", "-3"], ["--alpha-w"]),
    (["--alpha-w", "inf"], ["--alpha-w"]),
])
def test_score_refuses_before_opening_a_file(tmp_path, extra, words):
    out = tmp_path / "out.pss"
    r = subprocess.run([SCORE, str(tmp_path / "no_such_in.csv"), str(out), "--bge", *extra],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert all(w in r.stderr for w in words), r.stderr
    assert "cannot read" not in r.stderr and "cannot load" not in r.stderr and not out.exists()


def test_score_keeps_refusing_f_bge(tmp_path):
    for name in ("BGe", "bge"):
        r = subprocess.run([SCORE, str(tmp_path / "no_such_in.csv"), str(tmp_path / "o.pss"), "-f", name],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "not on this path" in r.stderr


def test_score_bge_reads_numbers_and_prune_is_accepted(tmp_path):
    """--bge takes the numeric reader (a missing file is its error, exit 1), with --prune and --lambda too."""
    for extra in ([], ["--prune"], ["--lambda", "7"], ["--alpha-mu", "0.1", "--alpha-w", "12"]):
        r = subprocess.run([SCORE, str(tmp_path / "no_such_in.csv"), str(tmp_path / "o.pss"), "--bge", *extra],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "cannot read" in r.stderr, (extra, r.stderr)


def test_score_help_lists_bge():
    r = subprocess.run([SCORE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert all(w in r.stdout + r.stderr for w in ("--bge", "--alpha-mu", "--alpha-w"))


def test_header_declares_the_bge_calls():
    import ulg
    syms = ulg.header_symbols()
    assert all(s in syms for s in ("ulg_bge_set_prior", "ulg_bge_score", "ulg_bge_score_sets"))
    assert all(hasattr(ulg.lib(), s) for s in ("ulg_bge_set_prior", "ulg_bge_score", "ulg_bge_score_sets"))
    assert all(hasattr(ulg.Context, m) for m in ("set_bge_prior", "score_bge", "score_sets_bge"))
