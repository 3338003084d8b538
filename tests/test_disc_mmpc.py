"""Discrete MMPC (`mmpc --discrete`, ulg_disc_mmpc) on the CPU: the Python
restatement of its rules that the GPU tests check against, the condition the
committed inputs must meet for that comparison to be fair, ulg_chi2_log_sf
against closed forms, and the command line's refusals.

The rules are those at the top of csrc/disc_mmpc.hip.  The
restatement counts with numpy.bincount, takes n ln n in FP64 and has its own
-ln p: for even dof the finite Poisson sum, for odd dof erfc plus the finite
half-integer sum, both summed in log space (math.lgamma), with erfc's
asymptotic series where erfc itself underflows.

Margins.  A decision of MMPC compares an association with the threshold
-ln alpha, or the best candidate with the runner-up.  The restatement records
the smallest |a - b| / max(1, |a|, |b|) over all of them; an input is usable
only if that margin is far above what FP64 rounding can move (>= 1e-6 here: the
GPU's G^2 differs from the restatement's by ~1e-12 relative).

One kind of argmax is left out of the margin: an exact tie between two
candidates whose deciding tests have the same dof and the same sorted counts in
all four tables (hepatitis has such pairs of binary columns at N = 80).  G^2 is
a function of those counts alone -- the restatement adds its terms with
math.fsum, the kernel as integers, both independent of the cells' order -- so
both sides see an exact tie and the lowest index decides it: rounding has no
part in that decision.  A tie of any other kind counts as margin 0."""
import functools
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import ulg
from conftest import PKG
from test_discrete import HEP, synthetic

MMPC = os.path.join(PKG, "bin", "mmpc")
CHI2 = os.path.join(PKG, "bin", "chi2_check")
SAN_CHI2 = os.path.join(PKG, "bin", "san", "chi2_check")
MAX_CELLS = 32768
MAX_POOL = 24


# ---- -ln p: the closed forms ---------------------------------------------------
def _log_erfc(y):
    if y < 25.0:
        return math.log(math.erfc(y))
    # erfc(y) ~ exp(-y^2) / (y sqrt(pi)) (1 - 1/(2y^2) + 3/(2y^2)^2 - ...)
    z = y * y
    s = term = 1.0
    for k in range(1, 200):
        nxt = -term * (2 * k - 1) / (2 * z)
        if abs(nxt) >= abs(term):
            break
        term = nxt
        s += term
        if abs(term) < 1e-18:
            break
    return -z - math.log(y * math.sqrt(math.pi)) + math.log(s)


def log_sf_closed(x, dof):
    """ln Q(dof / 2, x / 2) for integer dof >= 1."""
    if x <= 0:
        return 0.0
    z = x / 2.0
    lz = math.log(z)
    if dof % 2 == 0:
        logs = [k * lz - z - math.lgamma(k + 1.0) for k in range(dof // 2)]
    else:
        logs = [_log_erfc(math.sqrt(z))]
        logs += [(k - 0.5) * lz - z - math.lgamma(k + 0.5) for k in range(1, (dof - 1) // 2 + 1)]
    m = max(logs)
    return m + math.log(math.fsum(math.exp(v - m) for v in logs))


def log_sf_poisson_sum(x, dof):
    """The even-dof closed form once more, in 50-digit decimal arithmetic.  In log_sf_closed each
    term's exponent k ln z - z - lgamma(k + 1) is rounded at ~1e-16 of its size, up to ~1e-11
    absolute for thousands of terms: harmless next to MMPC's margins, but more than the
    1e-12 the grid test below allows where ln Q is itself ~0 (dof 32768, x far below dof)."""
    import decimal
    with decimal.localcontext() as cx:
        cx.prec = 50
        z = decimal.Decimal(x) / 2
        t = s = decimal.Decimal(1)
        for k in range(1, dof // 2):
            t = t * z / k
            s += t
        return float(s.ln() - z)


# ---- the test statistic --------------------------------------------------------
def bits(mask):
    return [p for p in range(64) if (mask >> p) & 1]


def shape_of(arity, x, t, mask):
    q = 1
    for s in bits(mask):
        q *= int(arity[s])
    rx, rt = int(arity[x]), int(arity[t])
    return q * rx * rt, (rx - 1) * (rt - 1) * q, q


def g2_restated(codes, arity, x, t, mask):
    """-> (G^2 in FP64, dof, cells, number of n ln n terms, sum |n ln n|)."""
    cells, dof, q = shape_of(arity, x, t, mask)
    rx, rt = int(arity[x]), int(arity[t])
    idx = np.zeros(codes.shape[0], dtype=np.int64)
    base = 1
    for s in bits(mask):  # ascending, the first with base 1
        idx += codes[:, s].astype(np.int64) * base
        base *= int(arity[s])
    idx += (codes[:, x].astype(np.int64) + rx * codes[:, t].astype(np.int64)) * q
    tab = np.bincount(idx, minlength=cells).astype(np.int64).reshape(rt, rx, q)

    def nlogn(a):
        # fsum: the exactly rounded sum, so tables that are relabellings of each other give equal bits
        a = a[a > 1].astype(np.float64)
        return math.fsum(a * np.log(a)), int(a.size)

    (sxtz, c1), (sz, c2) = nlogn(tab), nlogn(tab.sum(axis=(0, 1)))
    (sxz, c3), (stz, c4) = nlogn(tab.sum(axis=0)), nlogn(tab.sum(axis=1))
    g2 = 2.0 * (sxtz + sz - sxz - stz)
    return max(g2, 0.0), dof, cells, c1 + c2 + c3 + c4, sxtz + sz + sxz + stz


def table_signature(codes, arity, x, t, mask):
    """What G^2 and dof are a function of: dof and the sorted counts of the four tables."""
    cells, dof, q = shape_of(arity, x, t, mask)
    rx = int(arity[x])
    idx = np.zeros(codes.shape[0], dtype=np.int64)
    base = 1
    for s in bits(mask):
        idx += codes[:, s].astype(np.int64) * base
        base *= int(arity[s])
    idx += (codes[:, x].astype(np.int64) + rx * codes[:, t].astype(np.int64)) * q
    tab = np.bincount(idx, minlength=cells).reshape(int(arity[t]), rx, q)
    parts = (tab, tab.sum(axis=(0, 1)), tab.sum(axis=0), tab.sum(axis=1))
    return (dof,) + tuple(tuple(sorted(int(c) for c in np.ravel(p) if c > 1)) for p in parts)


# ---- MMPC ------------------------------------------------------------------------
class Restatement:
    """The rules on one data set; run() is one call of ulg_disc_mmpc."""

    def __init__(self, codes, arity):
        self.codes, self.arity = codes, [int(a) for a in arity]
        self.N, self.n = codes.shape
        self._assoc = {}

    def assoc(self, x, t, mask):
        key = (x, t, mask)
        if key not in self._assoc:
            g2, dof, _, _, _ = g2_restated(self.codes, self.arity, x, t, mask)
            self._assoc[key] = 0.0 if dof == 0 else -log_sf_closed(g2, dof)
        return self._assoc[key]

    def run(self, alpha=0.05, max_cond=-1, h=5):
        """-> {"rows", "tests", "skipped", "margin"}."""
        n = self.n
        if max_cond < 0 or max_cond > MAX_POOL:
            max_cond = MAX_POOL
        crit = -math.log(alpha)
        st = {"tests": 0, "skipped": 0, "margin": math.inf}

        def rel(a, b):
            return abs(a - b) / max(1.0, abs(a), abs(b))

        def query(T, X, pool, must):
            """(min association over the performed subsets (inf if none), the first test that gave it),
            sizes ascending up to the first size with no performable subset."""
            others = [v for v in pool if v != must]
            need = 0 if must is None else 1
            best, arg = math.inf, None
            for s in range(0, len(others) + 1):
                if s + need > max_cond:
                    break
                done = 0
                for comb in itertools.combinations(others, s):
                    mask = sum(1 << v for v in comb) | (0 if must is None else 1 << must)
                    cells, _, _ = shape_of(self.arity, X, T, mask)
                    if cells <= MAX_CELLS and self.N >= h * cells:
                        a = self.assoc(X, T, mask)
                        st["margin"] = min(st["margin"], rel(a, crit))
                        if a < best:
                            best, arg = a, (X, T, mask)
                        done += 1
                    else:
                        st["skipped"] += 1
                st["tests"] += done
                if not done:
                    break
            return best, arg

        def same_table(u, v):
            return u is not None and v is not None and \
                table_signature(self.codes, self.arity, *u) == table_signature(self.codes, self.arity, *v)

        pc = []
        for T in range(n):
            alive = {X for X in range(n) if X != T}
            assoc, arg = {}, {}
            for X in sorted(alive):
                a, arg[X] = query(T, X, [], None)
                assoc[X] = 0.0 if math.isinf(a) else a
            cpc = []
            while True:
                alive = {X for X in alive if assoc[X] > crit}
                if not alive:
                    break
                order = sorted(alive, key=lambda X: (-assoc[X], X))
                F = order[0]
                if len(order) > 1 and not (assoc[F] == assoc[order[1]] and same_table(arg[F], arg[order[1]])):
                    st["margin"] = min(st["margin"], rel(assoc[F], assoc[order[1]]))
                assert len(cpc) < MAX_POOL
                alive.discard(F)
                cpc.append(F)
                for X in sorted(alive):
                    a, g = query(T, X, cpc, F)
                    if a < assoc[X]:
                        assoc[X], arg[X] = a, g
            keep = [True] * len(cpc)
            for i, X in enumerate(cpc):
                rest = [v for j, v in enumerate(cpc) if j != i and keep[j]]
                if query(T, X, rest, None)[0] <= crit:
                    keep[i] = False
            pc.append({v for v, k in zip(cpc, keep) if k})
        rows = [sum(1 << X for X in range(n) if X in pc[T] and T in pc[X]) for T in range(n)]
        return {"rows": rows, "tests": st["tests"], "skipped": st["skipped"], "margin": st["margin"]}


# ---- the committed inputs --------------------------------------------------------
ARITY6 = [2, 3, 2, 4, 3, 2]
ARITY8C = [2, 3, 2, 4, 3, 2, 1, 3]   # column 6 is constant
ARITY8D = [2, 3, 2, 2, 3, 2, 2, 3]


def dense(N, seed):
    """Column j follows j-1 with probability 0.35, (j-2)+(j-1) mod r_j with 0.35, j-4 with 0.25."""
    rng = np.random.default_rng(seed)
    n = len(ARITY8D)
    codes = np.zeros((N, n), dtype=np.uint8)
    for j in range(n):
        r = ARITY8D[j]
        col = rng.integers(0, r, size=N)
        u = rng.random(N)
        if j >= 1:
            col = np.where(u < 0.35, codes[:, j - 1] % r, col)
        if j >= 2:
            col = np.where((u >= 0.35) & (u < 0.70), (codes[:, j - 2].astype(np.int64) + codes[:, j - 1]) % r, col)
        if j >= 4:
            col = np.where((u >= 0.70) & (u < 0.95), codes[:, j - 4] % r, col)
        codes[:, j] = col
    for j in range(n):
        codes[:ARITY8D[j], j] = np.arange(ARITY8D[j])
    return codes


ARITY36 = [(2, 3, 2, 4, 3, 2)[j % 6] for j in range(36)]


def wide36(N, seed):
    """syn6's chain (each column follows its left neighbour with probability 0.4) in the columns 31 to
    35 of 36; the columns 0 to 30 are independent.  Every decision that matters sits on bits >= 31."""
    rng = np.random.default_rng(seed)
    codes = np.zeros((N, 36), dtype=np.uint8)
    for j in range(36):
        col = rng.integers(0, ARITY36[j], size=N)
        if j >= 31:
            col = np.where(rng.random(N) < 0.4, codes[:, j - 1] % ARITY36[j], col)
        codes[:, j] = col
    for j in range(36):
        codes[:ARITY36[j], j] = np.arange(ARITY36[j])
    return codes


def hepatitis():
    rows = [ln.strip().split(",") for ln in open(HEP).read().splitlines()][1:]
    maps = [dict() for _ in rows[0]]
    codes = np.array([[maps[c].setdefault(r[c], len(maps[c])) for c in range(len(maps))] for r in rows],
                     dtype=np.uint8)
    return codes, [len(m) for m in maps]


INPUTS = ([f"syn6-N{N}-s{s}" for N, seeds in ((64, (1, 2, 3)), (300, (1, 2, 3, 4, 5)), (2500, (1, 2, 3, 4, 5)))
           for s in seeds] + ["const8-N2500-s1"] +
          [f"dense8-N{N}-s{s}" for N in (2500, 300) for s in (1, 2, 3, 4)] + ["hepatitis", "wide36-N1000-s1"])
ALPHAS = (0.05, 0.01)
MAX_CONDS = (-1, 0, 1, 3)
MIN_PER_CELL = (5, 1)


@functools.lru_cache(maxsize=None)
def input_case(name):
    """-> (codes, arity, Restatement): built once per session, never modified."""
    if name == "hepatitis":
        codes, arity = hepatitis()
    else:
        kind, N, s = name.split("-")
        N, s = int(N[1:]), int(s[1:])
        if kind == "syn6":
            codes, arity = synthetic(6, N, ARITY6, s), ARITY6
        elif kind == "const8":
            codes, arity = synthetic(8, N, ARITY8C, s), ARITY8C
        elif kind == "wide36":
            codes, arity = wide36(N, s), ARITY36
        else:
            codes, arity = dense(N, s), ARITY8D
    codes.setflags(write=False)
    return codes, list(arity), Restatement(codes, arity)


@functools.lru_cache(maxsize=None)
def restated_run(name, alpha, max_cond, h):
    return input_case(name)[2].run(alpha, max_cond, h)


def edges_of(rows):
    return sum(bin(r).count("1") for r in rows) // 2


@pytest.mark.parametrize("name", INPUTS)
def test_inputs_decide_with_a_margin(name):
    """The condition on the inputs: no decision of the restatement is closer than 1e-6."""
    worst = math.inf
    for alpha in ALPHAS:
        for mc in MAX_CONDS:
            for h in MIN_PER_CELL:
                r = restated_run(name, alpha, mc, h)
                worst = min(worst, r["margin"])
                rows = r["rows"]
                assert all(((rows[j] >> i) & 1) == ((rows[i] >> j) & 1) for i in range(len(rows))
                           for j in range(len(rows))) and all(not (rows[i] >> i) & 1 for i in range(len(rows)))
    print(f"{name}: smallest margin {worst:.3g}")
    assert worst >= 1e-6


def test_restatement_on_known_shapes():
    r = restated_run("hepatitis", 0.05, -1, 5)
    print(f"hepatitis alpha 0.05: {edges_of(r['rows'])} edges, {r['tests']} tests, {r['skipped']} skipped, "
          f"margin {r['margin']:.3g}")
    assert edges_of(r["rows"]) == 15
    assert edges_of(restated_run("hepatitis", 0.01, -1, 5)["rows"]) == 9
    # the constant column and the column that follows only it have no neighbours
    for alpha in ALPHAS:
        rows = restated_run("const8-N2500-s1", alpha, -1, 5)["rows"]
        assert rows[6] == 0 and rows[7] == 0 and any(rows)
    # at N = 64 the reliability rule leaves tests out, at N = 2500 the dense inputs condition on up to 3
    assert all(restated_run(f"syn6-N64-s{s}", 0.05, -1, 5)["skipped"] > 0 for s in (1, 2, 3))
    assert restated_run("dense8-N2500-s1", 0.05, -1, 5)["tests"] > restated_run("dense8-N2500-s1", 0.05, 1, 5)["tests"]
    # independent columns, dependent columns
    rng = np.random.default_rng(5)
    a = rng.integers(0, 3, size=4000)
    b = rng.integers(0, 2, size=4000)
    c = np.where(rng.random(4000) < 0.8, a % 2, rng.integers(0, 2, size=4000))
    codes = np.stack([a, b, c], axis=1).astype(np.uint8)
    rows = Restatement(codes, [3, 2, 2]).run(0.01, -1, 5)["rows"]
    assert rows == [0b100, 0, 0b001]


def test_g2_restated_by_hand():
    # a 2 x 2 table [[3, 1], [1, 3]]: G^2 = 2 sum n ln(n N / (row col))
    codes = np.array([[0, 0]] * 3 + [[0, 1]] + [[1, 0]] + [[1, 1]] * 3, dtype=np.uint8)
    g2, dof, cells, _, _ = g2_restated(codes, [2, 2], 0, 1, 0)
    want = 2 * (6 * math.log(3 * 8 / 16) + 2 * math.log(1 * 8 / 16))
    assert dof == 1 and cells == 4 and abs(g2 - want) < 1e-12
    # conditioning on a copy of x makes x and t independent within every stratum
    codes3 = np.concatenate([codes, codes[:, :1]], axis=1)
    g2c, dofc, cellsc, _, _ = g2_restated(codes3, [2, 2, 2], 0, 1, 0b100)
    assert dofc == 2 and cellsc == 8 and g2c < 1e-12


# ---- ulg_chi2_log_sf --------------------------------------------------------------
DOFS = [1, 2, 3, 4, 9, 50, 324, 2001, 32768]
XS = sorted({m * 10.0 ** e for e in range(-6, 7) for m in (1.0, 2.5, 6.0)} | {1e7} |
            {d * f for d in DOFS for f in (0.5, 0.9, 1.0, 1.1, 2.0)})


@pytest.mark.parametrize("dof", DOFS)
def test_chi2_log_sf_against_closed_forms(dof):
    worst = 0.0
    for x in XS:
        want = log_sf_closed(x, dof) if dof % 2 else log_sf_poisson_sum(x, dof)
        got = ulg.chi2_log_sf(x, dof)
        assert math.isfinite(got) and got <= 0.0
        err = abs(got - want)
        worst = max(worst, max(err - 1e-12, 0.0) / max(abs(want), 1e-300))
        assert err <= 1e-9 * abs(want) + 1e-12, (dof, x, got, want)
    print(f"dof {dof}: worst relative difference beyond 1e-12 absolute: {worst:.3g}")


def test_closed_forms_agree():
    """The log-space sum MMPC's restatement uses against the decimal one, where both apply."""
    for dof in (2, 4, 50, 324):
        for x in XS:
            a, b = log_sf_closed(x, dof), log_sf_poisson_sum(x, dof)
            assert abs(a - b) <= 1e-12 * abs(b) + 1e-13, (dof, x, a, b)


def test_chi2_log_sf_edges():
    for x in XS:
        assert ulg.chi2_log_sf(x, 2) == -x / 2  # the closed form, to the last bit
    assert ulg.chi2_log_sf(0.0, 5) == 0.0 and ulg.chi2_log_sf(-3.0, 5) == 0.0
    # monotone in x, finite where the probability underflows
    v = [ulg.chi2_log_sf(x, 7) for x in XS]
    assert all(a >= b for a, b in zip(v, v[1:])) and v[-1] < -4e6


def _grid(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, ",".join(str(d) for d in DOFS), ",".join(repr(x) for x in XS)], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(DOFS) * len(XS)
    return out


def test_chi2_check_is_the_library_routine():
    for d, x, v in _grid(CHI2):
        assert float(v) == ulg.chi2_log_sf(float(x), float(d)), (d, x)
    r = subprocess.run([CHI2, "1,b", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


@pytest.fixture(scope="module")
def san_chi2():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/chi2_check"], check=True, stdout=subprocess.DEVNULL)
    return SAN_CHI2


def test_chi2_check_under_sanitizers(san_chi2):
    """The stand-alone program under ASan + UBSan: a report aborts it; the values are the plain build's
    to 1e-13 relative (the two builds differ in optimisation level)."""
    for (d, x, v), (d2, x2, v2) in zip(_grid(san_chi2), _grid(CHI2)):
        assert (d, x) == (d2, x2)
        assert abs(float(v) - float(v2)) <= 1e-13 * abs(float(v2)), (d, x, v, v2)


# ---- command line refusals (no GPU) -------------------------------------------------
def test_mmpc_refusals(tmp_path):
    out = tmp_path / "sk.csv"
    missing = str(tmp_path / "no_such_in.csv")
    for opts in (["-s"], ["-d", ";"], ["--min-per-cell", "3"]):
        r = subprocess.run([MMPC, *opts, missing, str(out)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--discrete" in r.stderr, (opts, r.stderr)
    r = subprocess.run([MMPC, "--discrete", "--min-per-cell", "0", missing, str(out)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "min-per-cell" in r.stderr
    assert not out.exists()
    r = subprocess.run([MMPC, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--discrete", "--hasHeader", "--delimiter", "--min-per-cell", "--alpha", "--max-cond", "--diagonal"):
        assert opt in r.stdout
    # a file that cannot be read is reported before any GPU is asked for
    r = subprocess.run([MMPC, "--discrete", "-s", missing, str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "no usable HIP device" not in r.stderr and not out.exists()
