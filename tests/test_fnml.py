"""fNML (`score --fnml`, ULG_SCORE_FNML) on the CPU: a Python restatement of the
contract, itself held to brute force, the bound Fk that the GPU tests hold the
kernel to, the host check program and the command line's refusals.

The value.  For variable v of arity r and parent set P,
    s = sum_cells n_jk ln n_jk - sum_j n_j ln n_j - sum_{j : n_j > 0} ln C(r, n_j),
    C(2, n) = sum_h binom(n, h) (h/n)^h ((n-h)/n)^(n-h)           (0^0 = 1),
    C(k, n) = C(k-1, n) + n / (k-2) C(k-2, n),   C(1, n) = C(r, 0) = 1.
The contract (csrc/disc_fnml.h): C(2, n) is that sum for n <= 1000 and
Szpankowski's exp(ln(n pi / 2) / 2 + sqrt(8 / (9 n pi)) + (1/12 - 4 / (9 pi)) / n)
above; the recurrence runs on rho_k = C(k, n) / C(k-1, n) = 1 + n / ((k-2) rho_{k-1})
with ln C(k, n) = ln C(k-1, n) + ln rho_k.

The restatement.  c2_fraction / regret_fraction are exact rationals
(fractions.Fraction) and equal the brute-force multinomial sum over all count
vectors.  log_regret(r, n) is the contract in numpy.longdouble (64-bit
mantissa): C(2, n) from the rational for n <= 1000, Szpankowski's form in long
double above, then the ratio recurrence; it is checked against the rationals.
exact_fnml() is math.fsum of the terms from the exact counts -> (exact64, T, A,
nj): T = the number of n ln n terms, A = sum |n ln n|, nj = the non-empty
parent-configuration counts.

Fk, kernel against exact64.  With u = 2^-53, s = fnml_shift(N, rmax) and
Tj = len(nj),
    Fk = ulp_f32(exact64) / 2 + 2 ((T + Tj) 2^-(s+1) + (T + 3) 2^-52 (A + R) + sum_j E(r, n_j)),
R = sum_j ln C(r, n_j), term by term:
  * (T + Tj) 2^-(s+1), the fix rule: each of the T n ln n terms and the Tj
    regrets is rounded once to a multiple of 2^-s (half a unit each, at most
    3 N terms); the integer sum is exact.
  * (T + 3) 2^-52 (A + R): the FP64 error of n ln n on both sides (the
    device's log, two ulps, times n; Python's log and product), the conversion
    of the integer sum, fsum's one rounding and the rounding of each long
    double regret to FP64, as Bk's in test_discrete.py.
  * E(r, n), the FP64 error of a table entry.  d2 = the relative error of the
    device's rho_2 = C(2, n): 2 u for n <= 1000 (the host table is within one
    FP64 ulp of the exact sum: fnml_check and test_host_table_against_rationals)
    and, above, Szpankowski's exponent x = ln C(2, n) evaluated in FP64 -- n pi / 2
    (two roundings and pi's), a log of L = 2 ulps, the halving, two additions
    of small terms: at most ((2 L + 2) x + 2) u absolutely -- then an exp of L
    ulps: d2 = ((2 L + 2) x + 2 L + 2) u.  A ratio rho_k = 1 + y, y =
    n / ((k-2) rho_{k-1}) < rho_k, passes d_{k-1} on and adds two roundings for
    y and one for the sum: d_k <= d_{k-1} + 3 u.  ln rho_k is off by d_k plus
    the log's own 2 L u ln rho_k, and each of the r - 2 additions rounds the
    partial sum, at most u ln C:
        E(r, n) = (r - 1) d2 + u (1.5 (r - 2)(r - 1) + (2 L + r - 2) ln C(r, n)).
    That is up to 253 ratio steps plus the host's C(2, n).  L is the device
    library's accuracy as test_discrete.py assumes it for log; the tests assert
    that E does not matter next to the fix rule's half units.
  * ulp_f32(exact64) / 2 and the factor 2: the one rounding to float, and an
    FP64 sum within the small terms of a rounding boundary, as in test_discrete.py.
A table entry read back (ulg_disc_regret) is within
    Et(r, n) = E(r, n) + 2^-(s+1) + 2 u max(ln C, 1)
of log_regret: its one fix rounding, and the rounding of the reference to FP64.
Nothing in Fk or Et is measured."""
import functools
import itertools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import PKG
from test_bdeu import _counts
from test_discrete import pairs_up_to, synthetic, ulp_f32

SCORE = os.path.join(PKG, "bin", "score")
CHECK = os.path.join(PKG, "bin", "fnml_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "fnml_check")

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the restatement needs a long double of 64 mantissa bits"
U = 2.0 ** -53
LIB_ULPS = 2      # L above
EXACT_MAX = 1000  # kFnmlExact
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)

ARITY6 = [2, 2, 3, 3, 4, 255]
N6 = 2500


# ---- exact rationals --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _self_power(h):
    return h ** h  # 0 ** 0 == 1


@functools.lru_cache(maxsize=None)
def c2_fraction(n):
    num, binom = 0, 1
    for h in range(n + 1):
        num += binom * _self_power(h) * _self_power(n - h)
        binom = binom * (n - h) // (h + 1)
    return Fraction(num, n ** n)


def regret_fraction(r, n):
    """C(r, n) exactly, by the recurrence on the values."""
    if r <= 1 or n == 0:
        return Fraction(1)
    a, b = Fraction(1), c2_fraction(n)
    for k in range(3, r + 1):
        a, b = b, b + Fraction(n, k - 2) * a
    return b


def brute_force(r, n):
    """The multinomial sum over all count vectors (h_1 .. h_r) of n."""
    total = Fraction(0)
    for cuts in itertools.combinations(range(n + r - 1), r - 1):
        hs = [b - a - 1 for a, b in zip((-1,) + cuts, cuts + (n + r - 1,))]
        w = Fraction(math.factorial(n))
        for h in hs:
            w = w * Fraction(h, n) ** h / math.factorial(h)
        total += w
    return total


def _ld(fr):
    """A rational as a long double (two FP64 pieces: 106 bits before the one rounding)."""
    hi = float(fr)
    return LD(hi) + LD(float(fr - Fraction(hi)))


# ---- the contract in long double ----------------------------------------------------
def c2_contract(n):
    if n <= EXACT_MAX:
        return _ld(c2_fraction(n))
    x = LD(n)
    return np.exp(np.log(x * PI_LD / 2) / 2 + np.sqrt(8 / (9 * x * PI_LD)) + (LD(1) / 12 - 4 / (9 * PI_LD)) / x)


@functools.lru_cache(maxsize=None)
def log_regret(r, n):
    """ln C(r, n) as the contract states it, long double."""
    if r <= 1 or n == 0:
        return LD(0)
    rho = c2_contract(n)
    lc = np.log(rho)
    for k in range(3, r + 1):
        rho = 1 + LD(n) / (LD(k - 2) * rho)
        lc = lc + np.log(rho)
    return lc


def fnml_shift(N, rmax):
    """fnml_shift() of csrc/disc_fnml.h: U = N (2 ln N + ln rmax + 2) < 2^ex, shift = min(32, 62 - ex)."""
    return min(32, 62 - math.frexp(N * (2.0 * math.log(N) + math.log(max(rmax, 2)) + 2.0))[1])


# ---- the bounds -------------------------------------------------------------------
def table_err(r, n):
    """E(r, n) of the module docstring."""
    if r <= 1 or n == 0:
        return 0.0
    x = float(log_regret(2, n))
    d2 = 2 * U if n <= EXACT_MAX else ((2 * LIB_ULPS + 2) * x + 2 * LIB_ULPS + 2) * U
    return (r - 1) * d2 + U * (1.5 * (r - 2) * (r - 1) + (2 * LIB_ULPS + r - 2) * float(log_regret(r, n)))


def bound_entry(r, n, N, rmax):
    """Et(r, n)."""
    return table_err(r, n) + 2.0 ** -(fnml_shift(N, rmax) + 1) + 2 * U * max(float(log_regret(r, n)), 1.0)


def exact_fnml_from_counts(njk, nj, rv):
    njk, nj = [int(c) for c in njk], [int(c) for c in nj]
    plus = [c * math.log(c) for c in njk]
    minus = [c * math.log(c) for c in nj]
    regs = [float(log_regret(rv, c)) for c in nj]
    exact = math.fsum(itertools.chain(plus, (-x for x in minus), (-x for x in regs)))
    return exact, len(njk) + len(nj), math.fsum(plus) + math.fsum(minus), nj


def exact_fnml(codes, arity, v, mask):
    """The value the kernel promises -> (exact64, T, A, nj); never allocates q r entries."""
    (_, njk), (_, nj), rv, _ = _counts(codes, arity, v, mask)
    return exact_fnml_from_counts(njk, nj, rv)


def bound_fk_parts(exact, T, A, nj, rv, N, rmax):
    """-> (the fix rule's part, the FP64 part of the n ln n terms and the sums, the table's part), undoubled."""
    R = math.fsum(float(log_regret(rv, c)) for c in nj)
    return ((T + len(nj)) * 2.0 ** -(fnml_shift(N, rmax) + 1), (T + 3) * 2.0 ** -52 * (A + R),
            math.fsum(table_err(rv, c) for c in nj))


def bound_fk(exact, T, A, nj, rv, N, rmax):
    return ulp_f32(exact) / 2 + 2.0 * sum(bound_fk_parts(exact, T, A, nj, rv, N, rmax))


# ---- the input shared with test_gpu_fnml.py -------------------------------------------
@functools.lru_cache(maxsize=None)
def fnml6_case():
    """n = 6, N = 2500: the empty set has n_j = 2500, a binary parent about 1250 and a ternary one
    about 833, so the parent configurations lie on both sides of the 1000 / 1001 threshold; column 5
    has 255 values, where float values of C overflow."""
    codes = synthetic(6, N6, ARITY6, 20261020)
    codes.setflags(write=False)
    return codes, list(ARITY6)


def pairs6():
    return pairs_up_to(6, range(6), 3)


@functools.lru_cache(maxsize=None)
def reference6():
    """Per (v, P) of pairs6(): (exact64, T, A, nj).  Computed once."""
    codes, arity = fnml6_case()
    return [exact_fnml(codes, arity, v, m) for v, m in zip(*pairs6())]


# ---- the restatement, held to brute force ------------------------------------------------
def test_c2_first_values():
    assert [c2_fraction(n) for n in range(4)] == [1, 2, Fraction(5, 2), Fraction(26, 9)]


@pytest.mark.parametrize("r,n", [(2, 5), (3, 4), (4, 6), (5, 5)])
def test_recurrence_equals_brute_force(r, n):
    want = brute_force(r, n)
    assert regret_fraction(r, n) == want
    assert abs(float(log_regret(r, n)) - math.log(want)) <= 4 * U * math.log(want)


def test_regret_edges_and_growth():
    assert regret_fraction(1, 7) == 1 and regret_fraction(9, 0) == 1 and regret_fraction(7, 1) == 7
    assert log_regret(1, 500) == 0 and log_regret(255, 0) == 0
    for n in (1, 2, 10, 999, 1000, 1001, 2500):
        row = [float(log_regret(r, n)) for r in (2, 3, 4, 255)]
        assert row == sorted(row) and row[0] > 0 and row[-1] <= n * math.log(255) * (1 + 1e-6)  # C(r, n) <= r^n


@pytest.mark.parametrize("r,n", [(3, 4), (4, 6), (17, 100), (60, 1000), (255, 1000), (255, 37)])
def test_long_double_ratio_form_against_rationals(r, n):
    want = np.log(_ld(regret_fraction(r, n)))
    got = log_regret(r, n)
    assert abs(float(got - want)) <= 2.0 ** -60 * r * float(want)  # r steps of long double roundings
    assert table_err(r, n) < 2.0 ** -33  # the FP64 error of an entry is below the half unit of the fix rule


def test_float_values_overflow_where_log_space_does_not():
    """The reference's float C(r, n) is infinite from 3.4e38 on: ln C(60, 1000) = 117.5."""
    lc = float(log_regret(60, 1000))
    assert abs(lc - 117.5) < 0.05 and lc > math.log(float(np.finfo(np.float32).max))
    assert float(log_regret(255, N6)) > 88.73
    assert abs(float(log_regret(255, 100000)) - 889.8) < 0.05


def test_szpankowski_against_the_exact_sum():
    """The step at the threshold: the approximation at n = 1001 is 5.46e-7 above the exact sum."""
    n = EXACT_MAX + 1
    rel = float(c2_contract(n) / _ld(c2_fraction(n)) - 1)
    assert 5.4e-7 < rel < 5.5e-7
    assert float(log_regret(2, n)) > float(log_regret(2, n - 1))


def test_host_table_against_rationals():
    """fnml_c2_table() (csrc/disc_fnml.h), printed by `fnml_check c2`: within one FP64 ulp of the
    correctly rounded rational, at every n <= 100 and a spread of larger ones."""
    r = subprocess.run([CHECK, "c2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    table = [float.fromhex(x) for x in r.stdout.split()]
    assert len(table) == EXACT_MAX + 1
    worst = 0.0
    for n in list(range(101)) + list(range(137, 1000, 37)) + [200, 500, 998, 999, 1000]:
        want = float(c2_fraction(n))
        assert abs(table[n] - want) <= math.ulp(want), (n, table[n], want)
        worst = max(worst, abs(table[n] - want) / math.ulp(want))
    assert table[:3] == [1.0, 2.0, 2.5]
    print(f"host C(2, n): at most {worst:.0f} ulp from the rounded rational")


def test_shift_restatement():
    assert fnml_shift(2, 2) == 32 and fnml_shift(N6, 255) == 32
    assert fnml_shift(2 ** 31 - 1, 255) == 25  # the floor fnml_check finds


def test_bound_on_the_gpu_test_input():
    """Fk < 1e-3 |value| on every pair the GPU test holds to it; the table's part of Fk is far below
    the fix rule's; parent configurations on both sides of the threshold occur."""
    codes, arity = fnml6_case()
    assert all(len(np.unique(codes[:, j])) == arity[j] for j in range(6))
    below = above = 0
    rel = share = 0.0
    smallest = math.inf
    for (v, m), (exact, T, A, nj) in zip(zip(*pairs6()), reference6()):
        fk = bound_fk(exact, T, A, nj, arity[v], N6, 255)
        fix, fp, tab = bound_fk_parts(exact, T, A, nj, arity[v], N6, 255)
        assert exact < 0 and fk < 1e-3 * abs(exact), (v, m, exact, fk)
        assert tab < 0.05 * fix, (v, m, tab, fix)
        assert sum(nj) == N6 and T <= 2 * N6
        rel, smallest, share = max(rel, fk / abs(exact)), min(smallest, abs(exact)), max(share, tab / fix)
        below += sum(1 for c in nj if c <= EXACT_MAX)
        above += sum(1 for c in nj if c > EXACT_MAX)
    assert below > 0 and above > 0
    print(f"Fk <= {rel:.2e} |value|, smallest |value| {smallest:.1f}, table part <= {share:.3f} of the fix part; "
          f"{below} configurations with n_j <= 1000, {above} above")


def test_value_by_hand():
    """Two binary columns, four records: the value from the definition."""
    codes = np.array([[0, 0], [0, 0], [1, 1], [1, 0]], dtype=np.uint8)
    exact, T, A, nj = exact_fnml(codes, [2, 2], 0, 0b10)
    # parent 1 = 0: child counts (2, 1), n_j = 3; parent 1 = 1: child counts (0, 1), n_j = 1
    want = 2 * math.log(2) - 3 * math.log(3) - math.log(26 / 9) - math.log(2)
    assert abs(exact - want) < 1e-14 and T == 5 and sorted(nj) == [1, 3]


# ---- the host check program ------------------------------------------------------------
def test_fnml_check():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fnml_check ok" in r.stdout, (r.stdout, r.stderr)


def test_fnml_check_under_sanitizers():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/fnml_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "fnml_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- command line refusals ------------------------------------------------------------------
@pytest.mark.parametrize("opts,word", [(["-f", "fNML"], "fNML"), (["--fnml", "--bdeu"], "--fnml"),
                                       (["--fnml", "-f", "cBIC"], "--fnml"),
                                       (["--fnml", "--enableDeCamposPruning"], "--fnml")])
def test_score_fnml_refuses_before_opening_a_file(opts, word, tmp_path):
    out = tmp_path / "out.pss"
    r = subprocess.run([SCORE, str(tmp_path / "no_such_in.csv"), str(out), *opts], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert word in r.stderr and "cannot read" not in r.stderr and not out.exists()


def test_score_help_lists_fnml():
    r = subprocess.run([SCORE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--fnml" in r.stdout + r.stderr
