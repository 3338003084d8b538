"""Discrete MMPC on the GPU (ulg_disc_g2, ulg_disc_mmpc, `mmpc --discrete`)
against the Python restatement in test_disc_mmpc.py.

Values.  The kernel adds every n ln n term as an integer multiple of 2^-shift
(shift = 32 for every N used here: N ln N < 2^30; test_gpu_discrete_shapes.py
has the one input with shift = 31).  One such term is within
2^-(shift+1) of the device's FP64 n ln n, which is within two ulps of the
device log (relative 2^-51) plus the product's rounding of the exact value; the
restatement's FP64 terms carry one ulp of numpy's log and the product's
rounding, and its four sums are exactly rounded (math.fsum) and then combined
with three more roundings.  With T terms of total size A = sum |n ln n|,
    |G2_gpu - G2_ref| <= B = 2 [T 2^-(shift+1) + (T + 4) 2^-52 A].
B is ~1e-9 at N = 2500; one record moved between two cells changes G^2 by
about ln of a count, ~1, so B cannot hide a miscounted record.  dof and cells
are integers and must be equal.

Skeletons.  Every input meets the margin condition test_disc_mmpc.py asserts
(>= 1e-6 relative in every decision, ~1e6 B), so the rows and the counts of
performed and skipped tests must equal the restatement's exactly."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ulg
from conftest import PKG
from test_disc_mmpc import (ALPHAS, ARITY6, INPUTS, MAX_CONDS, MIN_PER_CELL, g2_restated, input_case, restated_run)
from test_discrete import HEP, synthetic

pytestmark = pytest.mark.gpu

MMPC = os.path.join(PKG, "bin", "mmpc")
SCORE = os.path.join(PKG, "bin", "score")
ASTAR = os.path.join(PKG, "bin", "astar")
STATUS = {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _shift(N):
    ex = math.frexp(N * math.log(N))[1]
    return min(32, 62 - ex)


def _all_tests(n, max_s):
    xs, ts, ms = [], [], []
    for x, t in itertools.permutations(range(n), 2):
        others = [v for v in range(n) if v not in (x, t)]
        for s in range(0, min(max_s, len(others)) + 1):
            for comb in itertools.combinations(others, s):
                xs.append(x)
                ts.append(t)
                ms.append(sum(1 << v for v in comb))
    return xs, ts, ms


def _check_values(ctx, codes, arity, xs, ts, ms):
    N = codes.shape[0]
    g2, dof, cells = ctx.g2_discrete(xs, ts, ms)
    assert g2.dtype == np.float64 and dof.dtype == np.int64 and cells.dtype == np.int64
    worst, seen = 0.0, set()
    for i, (x, t, m) in enumerate(zip(xs, ts, ms)):
        want, wdof, wcells, terms, total = g2_restated(codes, arity, x, t, m)
        bound = 2.0 * (terms * 2.0 ** -(_shift(N) + 1) + (terms + 4) * 2.0 ** -52 * total)
        assert (int(dof[i]), int(cells[i])) == (wdof, wcells), (x, t, m)
        assert g2[i] >= 0.0 and abs(g2[i] - want) <= bound, (N, x, t, m, float(g2[i]), want, bound)
        worst = max(worst, abs(g2[i] - want) / bound) if bound else worst
        seen.add(wcells)
    print(f"N={N}: {len(xs)} tests, tables of {min(seen)}..{max(seen)} cells, at most {worst:.3f} B")
    return g2


# ---- values --------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 64, 300, 2500])
def test_g2_within_bound(ctx, N):
    """Every (X, T | S), both orders, |S| <= 4, n = 6: tables of 4 to 288 cells; N = 2 and 64 are below
    the block size, 300 and 2500 end in a partial wave."""
    codes = synthetic(6, N, ARITY6, 700 + N)
    ctx.load_discrete(codes, ARITY6)
    xs, ts, ms = _all_tests(6, 4)
    g2 = _check_values(ctx, codes, ARITY6, xs, ts, ms)
    # G^2 is symmetric in X and T: the two orders are different tables with the same counts
    first = {(x, t, m): g2[i] for i, (x, t, m) in enumerate(zip(xs, ts, ms))}
    assert all(first[(t, x, m)] == v for (x, t, m), v in first.items())


def test_g2_constant_column(ctx):
    codes, arity, _ = input_case("const8-N2500-s1")
    ctx.load_discrete(codes, arity)
    xs, ts, ms = _all_tests(8, 2)
    g2 = _check_values(ctx, codes, arity, xs, ts, ms)
    _, dof, _ = ctx.g2_discrete(xs, ts, ms)
    for i, (x, t) in enumerate(zip(xs, ts)):
        if 6 in (x, t):
            assert dof[i] == 0 and g2[i] == 0.0


def test_g2_largest_table_and_beyond(ctx):
    """13 binary conditioning columns: 2^15 = 32768 cells, the whole 128 KB histogram; one more
    column of arity 2 or 3 is past it."""
    rng = np.random.default_rng(15)
    N, n = 300, 17
    codes = rng.integers(0, 2, size=(N, n)).astype(np.uint8)
    codes[:, 1] = np.where(rng.random(N) < 0.6, codes[:, 0], codes[:, 1])
    codes[:, 16] = rng.integers(0, 3, size=N)
    arity = [2] * 16 + [3]
    ctx.load_discrete(codes, arity)
    full = sum(1 << v for v in range(2, 15))
    xs, ts, ms = [0, 1, 0, 0, 0], [1, 0, 1, 1, 1], [full, full, full | 1 << 15, full | 1 << 16, 0b100]
    g2, dof, cells = ctx.g2_discrete(xs, ts, ms)
    assert cells.tolist() == [32768, 32768, 65536, 98304, 8] and dof.tolist() == [8192, 8192, 16384, 24576, 2]
    assert math.isnan(g2[2]) and math.isnan(g2[3])
    for i in (0, 1, 4):
        want, _, _, terms, total = g2_restated(codes, arity, xs[i], ts[i], ms[i])
        bound = 2.0 * (terms * 2.0 ** -33 + (terms + 4) * 2.0 ** -52 * total)
        assert abs(g2[i] - want) <= bound, (i, float(g2[i]), want, bound)
    assert g2[0] == g2[1] and g2[0] > 0


def test_g2_does_not_depend_on_order_or_call(ctx):
    codes, arity, _ = input_case("dense8-N2500-s1")
    ctx.load_discrete(codes, arity)
    xs, ts, ms = _all_tests(8, 3)
    a = ctx.g2_discrete(xs, ts, ms)[0]
    b = ctx.g2_discrete(xs[::-1], ts[::-1], ms[::-1])[0][::-1]
    c = ctx.g2_discrete(xs, ts, ms)[0]
    one = ctx.g2_discrete(xs[1234:1235], ts[1234:1235], ms[1234:1235])[0]
    assert a.tobytes() == b.tobytes() == c.tobytes() and one[0] == a[1234]
    assert len(ctx.g2_discrete([], [], [])[0]) == 0


def test_g2_high_arity(ctx):
    """Arities 255 x 128: a marginal table of 32,640 cells (codes up to 254 and 127, the r_t loop of
    128, 255 x 128 products summed by one thread for n_z); an arity-1 conditioning column is skipped
    by the kernel and leaves the table as it is; one binary column more is 65,280 cells: not performed."""
    arity = [255, 128, 2, 3, 1]
    codes = synthetic(5, 4000, arity, 255)
    assert codes[:, 0].max() == 254 and codes[:, 1].max() == 127
    ctx.load_discrete(codes, arity)
    xs, ts, ms = [0, 0, 1, 0, 0, 2, 1], [1, 1, 0, 1, 2, 0, 2], [0, 1 << 4, 0, 1 << 2, 1 << 3, 1 << 3, 1 << 4 | 1 << 3]
    g2, dof, cells = ctx.g2_discrete(xs, ts, ms)
    assert cells.tolist() == [32640, 32640, 32640, 65280, 1530, 1530, 768]
    assert dof.tolist() == [254 * 127, 254 * 127, 254 * 127, 254 * 127 * 2, 254 * 3, 254 * 3, 127 * 3]
    assert math.isnan(g2[3])
    keep = [0, 1, 2, 4, 5, 6]
    _check_values(ctx, codes, arity, [xs[i] for i in keep], [ts[i] for i in keep], [ms[i] for i in keep])
    assert g2[0] == g2[1] == g2[2] and g2[4] == g2[5] and g2[0] > 0


def test_g2_more_tests_than_workgroups(ctx):
    """2352 tests on 2048 workgroups, every one against the restatement: a workgroup's second test
    reuses its histogram."""
    codes, arity, _ = input_case("dense8-N2500-s1")
    ctx.load_discrete(codes, arity)
    xs, ts, ms = _all_tests(8, 3)
    assert len(xs) == 2352 > 2048
    _check_values(ctx, codes, arity, xs, ts, ms)


def test_g2_variables_from_bit_30_up(ctx):
    """x, t and the conditioning set among the variables 30..39 of 40: masks with bits on both sides of 32."""
    arity = [2 + (j * 7 % 5 == 0) for j in range(40)]
    codes = synthetic(40, 300, arity, 40)
    ctx.load_discrete(codes, arity)
    xs, ts, ms = [], [], []
    for x, t in itertools.permutations(range(30, 40), 2):
        others = [v for v in range(30, 40) if v not in (x, t)]
        for s in range(3):
            for comb in itertools.combinations(others, s):
                xs.append(x)
                ts.append(t)
                ms.append(sum(1 << v for v in comb))
    assert len(xs) == 90 * 37 and max(ms) >> 39 and set(arity[30:]) == {2, 3}
    _check_values(ctx, codes, arity, xs, ts, ms)


# ---- skeletons -----------------------------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
def test_skeleton_equals_restatement(ctx, name):
    codes, arity, _ = input_case(name)
    ctx.load_discrete(codes, arity)
    for alpha in ALPHAS:
        for mc in MAX_CONDS:
            for h in MIN_PER_CELL:
                want = restated_run(name, alpha, mc, h)
                rows = ctx.mmpc_discrete(alpha, mc, h)
                assert rows == want["rows"], (name, alpha, mc, h)
                assert ctx.info("disc_mmpc_tests") == want["tests"], (name, alpha, mc, h)
                assert ctx.info("disc_mmpc_skipped") == want["skipped"], (name, alpha, mc, h)
    assert ctx.mmpc_discrete() == restated_run(name, 0.05, -1, 5)["rows"]  # the defaults
    assert ctx.mmpc_discrete(0.05, 99, 5) == restated_run(name, 0.05, -1, 5)["rows"]  # > 24 means 24


# ---- errors --------------------------------------------------------------------------
def test_errors_leave_the_lists(ctx):
    codes, arity, _ = input_case("syn6-N300-s1")
    full = [(1 << 6) - 1] * 6
    # continuous data loaded
    ctx.load(np.random.default_rng(3).normal(size=(50, 4)), 2.0)
    with pytest.raises(ulg.ULGError) as e:
        ctx.mmpc_discrete()
    assert _status(e) == STATUS["STATE"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.g2_discrete([0], [1], [0])
    assert _status(e) == STATUS["STATE"]
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(6)), full, 2)
    before = ctx.fetch(st)

    def same_lists():
        return all(a.tobytes() == b.tobytes() for a, b in zip(ctx.fetch(st), before))

    for alpha in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ulg.ULGError) as e:
            ctx.mmpc_discrete(alpha)
        assert _status(e) == STATUS["ARG"] and same_lists()
    with pytest.raises(ulg.ULGError) as e:
        ctx.mmpc_discrete(0.05, -1, 0)
    assert _status(e) == STATUS["ARG"] and same_lists()
    for xs, ts, ms in (([2], [2], [0]), ([0], [1], [0b10]), ([0], [1], [0b01]), ([6], [1], [0]), ([0], [-1], [0]),
                       ([0], [1], [1 << 6])):
        with pytest.raises(ulg.ULGError) as e:
            ctx.g2_discrete(xs, ts, ms)
        assert _status(e) == STATUS["ARG"] and same_lists(), (xs, ts, ms)
    # the Fisher-z MMPC still refuses discrete data
    with pytest.raises(ulg.ULGError) as e:
        ctx.mmpc()
    assert _status(e) == STATUS["STATE"] and same_lists()
    # and the calls that succeed leave the lists too
    ctx.g2_discrete([0], [1], [0b100])
    ctx.mmpc_discrete()
    assert same_lists()


# ---- end to end ------------------------------------------------------------------------
def test_command_lines_end_to_end(tmp_path):
    sk, pss, net = tmp_path / "sk.csv", tmp_path / "hep.pss", tmp_path / "net"
    r = subprocess.run([MMPC, "--discrete", "-s", HEP, str(sk)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = restated_run("hepatitis", 0.05, -1, 5)
    n = len(want["rows"])
    text = "".join(",".join("1" if (want["rows"][i] >> j) & 1 else "0" for j in range(n)) + "\n" for i in range(n))
    assert sk.read_text() == text
    assert f"edges=15, G^2 tests {want['tests']} (skipped {want['skipped']})" in r.stdout
    r = subprocess.run([SCORE, HEP, str(pss), "-s", "-k", str(sk)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([ASTAR, str(pss), "-k", str(sk), "-n", str(net)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(str(net) + ".csv")
    # every stored parent set lies inside its variable's 2-hop candidate set
    cands = ulg.candidates_from_edges(want["rows"], n)
    names = open(HEP).readline().strip().split(",")
    index = {nm: i for i, nm in enumerate(names)}
    v, stored = -1, 0
    for ln in pss.read_text().splitlines():
        if ln.startswith("VAR "):
            v = index[ln[4:].strip()]
        elif v >= 0 and ln.strip() and not ln.startswith("META"):
            mask = sum(1 << index[x] for x in ln.split()[1:])
            assert mask & ~(cands[v] & ~(1 << v)) == 0, (v, ln)
            stored += 1
    assert v == n - 1 and stored >= n
    # --diagonal and the options of the reader
    r = subprocess.run([MMPC, "--discrete", "--hasHeader", "--delimiter", ",", "--alpha", "0.01", "--max-cond", "1",
                        "--min-per-cell", "1", "--diagonal", HEP, str(sk)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    w2 = restated_run("hepatitis", 0.01, 1, 1)["rows"]
    got = [[int(x) for x in ln.split(",")] for ln in sk.read_text().splitlines()]
    assert got == [[1 if i == j or (w2[i] >> j) & 1 else 0 for j in range(n)] for i in range(n)]
