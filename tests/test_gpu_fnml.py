"""fNML on the GPU (ULG_SCORE_FNML, ulg_disc_regret, `score --fnml`) against
test_fnml.py: the regret table within Et of the long-double contract, the
values within Fk of the exact value (both bounds are derived in that module's
docstring), bit-identical across the dense and sparse counting paths, repeated
calls and launch shapes.  Sets, counts and list structure are exact."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ulg
from conftest import PKG
from test_disc_prune import apply_rule
from test_discrete import HEP, list_order
from test_fnml import (EXACT_MAX, N6, bound_entry, bound_fk, exact_fnml, fnml6_case, log_regret, pairs6,
                       reference6)

pytestmark = pytest.mark.gpu

SCORE = os.path.join(PKG, "bin", "score")
ASTAR = os.path.join(PKG, "bin", "astar")
FNML = ulg.Context.SCORE_FNML
STATUS = {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}
ROWS = [2, 3, 4, 255]  # the distinct arities of the six columns


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the table ------------------------------------------------------------------------
def test_regret_table(ctx):
    codes, arity = fnml6_case()
    ctx.load_discrete(codes, arity)
    assert ctx.info("fnml_table_bytes") == 0
    rows = {r: ctx.regret(r, 0, N6 + 1) for r in ROWS}
    size = ctx.info("fnml_table_bytes")
    assert size == len(ROWS) * (N6 + 1) * 8
    worst = 0.0
    for r in ROWS:
        for n in (0, 1, 2, 3, 999, 1000, 1001, 1002, N6):
            got, want, et = float(rows[r][n]), float(log_regret(r, n)), bound_entry(r, n, N6, 255)
            print(f"ln C({r}, {n}) gpu={got:.12f} contract={want:.12f} Et={et:.3g}")
            assert abs(got - want) <= et, (r, n, got, want, et)
            worst = max(worst, abs(got - want) / et)
            assert ctx.regret(r, n, 1)[0] == rows[r][n]
    print(f"at most {worst:.3f} Et from the contract")
    for n, c in enumerate((1.0, 2.0, 2.5, 26.0 / 9.0)):
        assert abs(float(rows[2][n]) - math.log(c)) <= bound_entry(2, n, N6, 255)
    for r in ROWS:
        assert np.all(np.isfinite(rows[r])) and rows[r][0] == 0.0
        assert np.all(np.diff(rows[r]) > 0), f"row {r} does not rise with n"
    for lo, hi in zip(ROWS, ROWS[1:]):
        assert np.all(rows[hi][1:] > rows[lo][1:]), f"rows {lo}, {hi}: not rising with the arity"
    assert rows[255][N6] > 88.73  # the reference's float C is infinite here
    # the step at the threshold is Szpankowski's 5.5e-7 on top of the row's own growth
    # (against the mean of the neighbouring increments, which are exact - exact and approximation - approximation)
    d = np.diff(rows[2][EXACT_MAX - 1:EXACT_MAX + 3])
    step = d[1] - (d[0] + d[2]) / 2
    assert 5.3e-7 < step < 5.6e-7, step
    # nothing is rebuilt: neither by a second read nor by a scoring call
    live = ctx.info("device_bytes_live")
    assert ctx.regret(255, N6, 1)[0] == rows[255][N6]
    assert ctx.info("fnml_table_bytes") == size and ctx.info("device_bytes_live") == live
    ctx.score_sets_discrete([0], [0b10], kind=FNML)
    assert ctx.info("fnml_table_bytes") == size
    for bad in ((5, 0, 1), (2, -1, 1), (2, N6, 2), (2, N6 + 1, 1), (0, 0, 1), (256, 0, 1)):
        with pytest.raises(ulg.ULGError) as e:
            ctx.regret(*bad)
        assert _status(e) == STATUS["ARG"], bad
    assert len(ctx.regret(2, N6, 0)) == 0
    ctx.load_discrete(codes, arity)
    assert ctx.info("fnml_table_bytes") == 0


# ---- values ---------------------------------------------------------------------------
def test_values_within_fk_and_paths_identical(ctx):
    """All 156 (v, P) with at most three parents; N = 2500: the hash table leaves LDS for the HBM slab."""
    codes, arity = fnml6_case()
    vs, ps = pairs6()
    ref = reference6()
    assert len(vs) == 156
    assert any(c > EXACT_MAX for _, _, _, nj in ref for c in nj) and any(c <= EXACT_MAX for _, _, _, nj in ref for c in nj)
    ctx.load_discrete(codes, arity)
    dense = ctx.score_sets_discrete(vs, ps, kind=FNML)
    again = ctx.score_sets_discrete(vs, ps, kind=FNML)
    worst = 0.0
    for v, m, got, (exact, T, A, nj) in zip(vs, ps, dense, ref):
        fk = bound_fk(exact, T, A, nj, arity[v], N6, 255)
        print(f"v={v} P={m:#x} gpu={float(got):.6f} exact={exact:.9f} Fk={fk:.3g}")
        assert abs(float(got) - exact) <= fk, (v, m, float(got), exact, fk)
        worst = max(worst, abs(float(got) - exact) / fk)
    print(f"at most {worst:.3f} Fk from exact")
    assert dense.tobytes() == again.tobytes(), "two dense calls differ"
    rev = ctx.score_sets_discrete(vs[::-1], ps[::-1], kind=FNML)
    assert rev[::-1].tobytes() == dense.tobytes(), "reversed order differs"
    three = ctx.score_sets_discrete(vs * 3, ps * 3, kind=FNML)
    assert three.tobytes() == np.tile(dense, 3).tobytes(), "three repeats in one call differ"
    ctx.set_option("disc_dense_cells", 8)
    sparse = ctx.score_sets_discrete(vs, ps, kind=FNML)
    assert sparse.tobytes() == dense.tobytes(), "dense and sparse paths differ"
    assert ctx.score_sets_discrete(vs * 3, ps * 3, kind=FNML).tobytes() == three.tobytes()
    assert ctx.score_sets_discrete(vs[::-1], ps[::-1], kind=FNML).tobytes() == rev.tobytes()
    # the other kinds are not disturbed by the table or the option
    bic = ctx.score_sets_discrete(vs[:20], ps[:20])
    assert not np.array_equal(bic, dense[:20])


def test_more_items_than_one_pass_of_the_grid(ctx):
    """2496 items over at most 2048 workgroups, on both paths."""
    codes, arity = fnml6_case()
    vs, ps = pairs6()
    ctx.load_discrete(codes, arity)
    one = ctx.score_sets_discrete(vs, ps, kind=FNML)
    many = ctx.score_sets_discrete(vs * 16, ps * 16, kind=FNML)
    assert len(many) == 2496 and many.tobytes() == np.tile(one, 16).tobytes()
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete(vs * 16, ps * 16, kind=FNML).tobytes() == many.tobytes()


def test_arity_one_column(ctx):
    """A constant column scores +0.0 whatever its parents, has no row, and changes no other value."""
    codes, arity = fnml6_case()
    c7 = np.concatenate([codes, np.zeros((N6, 1), dtype=np.uint8)], axis=1)
    ctx.load_discrete(c7, arity + [1])
    got = ctx.score_sets_discrete([6, 6, 6, 0, 0], [0, 0b1, 0b100011, 0b10, 0b1000010], kind=FNML)
    assert got[:3].tobytes() == np.zeros(3, dtype=np.float32).tobytes()
    assert got[3].tobytes() == got[4].tobytes()
    assert ctx.info("fnml_table_bytes") == len(ROWS) * (N6 + 1) * 8
    assert ctx.regret(1, 0, 3).tolist() == [0.0, 0.0, 0.0]
    st, _ = ctx.score_discrete([6, 0], [0b1111111, 0b1111111], 2, kind=FNML)
    offs, sets, scores = ctx.fetch(st)
    assert offs[1] == 1 and int(sets[0]) == 0 and scores[0].tobytes() == np.float32(0.0).tobytes()


# ---- lists ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five():
    codes, arity = fnml6_case()
    return np.ascontiguousarray(codes[:, :5]), arity[:5], [0b11111] * 5


def _rule_lists(ctx, n, k, constraints=()):
    """The store rule on ulg_disc_score_sets' values -> (offsets, sets, scores) in the scorer's order."""
    offs, sets, scores = [0], [], []
    for v in range(n):
        order = list_order([p for p in range(n) if p != v], k)
        vals = ctx.score_sets_discrete([v] * len(order), order, kind=FNML)
        alts = [(r, f) for cv, r, f in constraints if cv == v]
        for m, s in zip(order, vals):
            if alts and not any((r & ~m) == 0 and (m & f) == 0 for r, f in alts):
                assert s == 1.0
                continue
            if (m == 0 and s < 1) or (m != 0 and s < 0):
                sets.append(m)
                scores.append(s)
        offs.append(len(sets))
    return np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32)


@pytest.mark.parametrize("dense_cells", [16384, 8])
def test_lists_prune_and_search(ctx, five, dense_cells):
    codes, arity, full = five
    ctx.load_discrete(codes, arity)
    ctx.set_option("disc_dense_cells", dense_cells)
    want = _rule_lists(ctx, 5, 3)
    st, sc = ctx.score_discrete(list(range(5)), full, 3, kind=FNML, prune=False)
    plain = ctx.fetch(st)
    assert sc == 5 * (1 + 4 + 6 + 4) and st == len(want[1]) and 0 < st
    assert [int(x) for x in plain[0]] == [int(x) for x in want[0]] and _same(plain[1:], want[1:])
    assert ctx.info("disc_dense_sets") + ctx.info("disc_sparse_sets") == sc
    assert (ctx.info("disc_sparse_sets") > 0) == (dense_cells == 8)
    assert ctx.info("disc_pruned") == 0 and ctx.info("highest_completed_layer") == 3
    # the exact values behind the stored ones
    for v in range(5):
        for m, s in zip(plain[1][plain[0][v]:plain[0][v + 1]], plain[2][plain[0][v]:plain[0][v + 1]]):
            exact, T, A, nj = exact_fnml(codes, arity, v, int(m))
            assert abs(float(s) - exact) <= bound_fk(exact, T, A, nj, arity[v], N6, max(arity))
    st1, sc1 = ctx.score_discrete(list(range(5)), full, 3, kind=FNML, prune=True)
    pruned = ctx.fetch(st1)
    assert sc1 == sc and ctx.info("disc_pruned") == st - st1 and 0 < st1 <= st
    assert _same(pruned, apply_rule(*plain))
    # the search reads the lists; the DAG's cost is the sum of its families' costs
    offs, sets, scores = pruned
    ctx.search_from_scores()
    res = ctx.astar(mode=0)
    costs = ctx.quantize(scores)
    lookup = [{int(m): float(c) for m, c in zip(sets[offs[v]:offs[v + 1]], costs[offs[v]:offs[v + 1]])} for v in range(5)]
    total = math.fsum(lookup[v][int(res["vpar"][v])] for v in range(5))
    assert abs(total - float(res["cost"])) <= 1e-5 * abs(total)


def test_lists_with_constraints(ctx, five):
    codes, arity, full = five
    cons = [(0, 0b00010, 0b00100), (0, 0b01000, 0),  # variable 0: (1 and not 2) or 3
            (3, 0, 0b10001),                         # variable 3: neither 0 nor 4
            (4, 0b00001, 0)]                         # variable 4: needs parent 0
    ctx.load_discrete(codes, arity)
    st0, _ = ctx.score_discrete(list(range(5)), full, 3, kind=FNML, prune=False)
    ctx.set_constraints(cons)
    want = _rule_lists(ctx, 5, 3, constraints=cons)
    st, _ = ctx.score_discrete(list(range(5)), full, 3, kind=FNML)
    got = ctx.fetch(st)
    assert st < st0 and st == len(want[1])
    assert [int(x) for x in got[0]] == [int(x) for x in want[0]] and _same(got[1:], want[1:])
    assert 0 not in [int(x) for x in got[1][got[0][4]:got[0][5]]]
    assert ctx.score_sets_discrete([4, 4, 3], [0, 0b00010, 0b00001], kind=FNML).tolist() == [1.0, 1.0, 1.0]  # R6


# ---- errors ---------------------------------------------------------------------------
def test_errors_leave_the_lists(ctx, five):
    codes, arity, full = five
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete([0], [1], 1, kind=FNML)
    assert _status(e) == STATUS["STATE"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets_discrete([0], [0], kind=FNML)
    assert _status(e) == STATUS["STATE"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.regret(2, 0, 1)
    assert _status(e) == STATUS["STATE"]
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(5)), full, 2, kind=FNML)
    before = ctx.fetch(st)
    for kind in (0, 2, 4, 6):
        with pytest.raises(ulg.ULGError) as e:
            ctx.score_discrete(list(range(5)), full, 3, kind=kind)
        assert _status(e) == STATUS["ARG"] and _same(ctx.fetch(st), before)
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete([0, 7], full[:2], 3, kind=FNML)
    assert _status(e) == STATUS["ARG"] and _same(ctx.fetch(st), before)
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets_discrete([0], [1 << 9], kind=FNML)
    assert _status(e) == STATUS["ARG"] and _same(ctx.fetch(st), before)
    # fNML after a continuous load
    ctx.load(np.random.default_rng(3).normal(size=(50, 4)), 2.0)
    assert ctx.info("fnml_table_bytes") == 0
    for call in (lambda: ctx.score_discrete([0], [0b1110], 1, kind=FNML),
                 lambda: ctx.score_sets_discrete([0], [0b10], kind=FNML), lambda: ctx.regret(2, 0, 1)):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS["STATE"]
    # 9 parents of arity 255: 255^10 cells
    big = (np.arange(300)[:, None] * np.arange(1, 11)[None, :] % 255).astype(np.uint8)
    ctx.load_discrete(big, [255] * 10)
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete(list(range(10)), [(1 << 10) - 1] * 10, 9, kind=FNML)
    assert _status(e) == STATUS["UNSUPPORTED"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets_discrete([0], [0b1111111110], kind=FNML)
    assert _status(e) == STATUS["UNSUPPORTED"]


# ---- command line -----------------------------------------------------------------------
def _hepatitis():
    rows = [ln.strip().split(",") for ln in open(HEP).read().splitlines()]
    names, rows = rows[0], rows[1:]
    maps = [dict() for _ in names]
    codes = np.array([[maps[c].setdefault(r[c], len(maps[c])) for c in range(len(names))] for r in rows],
                     dtype=np.uint8)
    return names, codes, [len(m) for m in maps]


def test_score_command_line_fnml(ctx, tmp_path):
    pss = tmp_path / "hep.pss"
    r = subprocess.run([SCORE, HEP, str(pss), "-s", "--fnml", "-p", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"function": "fnml"' in r.stderr
    names, codes, arity = _hepatitis()
    index = {nm: i for i, nm in enumerate(names)}
    meta, blocks = {}, []
    for ln in open(pss).read().splitlines():
        if ln.startswith("META ") and not blocks:
            k, _, val = ln[5:].partition("=")
            meta[k.strip()] = val.strip()
        elif ln.startswith("VAR "):
            blocks.append((ln[4:].strip(), []))
        elif blocks and ln.strip() and not ln.startswith("META"):
            tok = ln.split()
            blocks[-1][1].append((tok[0], sum(1 << index[x] for x in tok[1:])))
    assert meta["score_type"] == "fnml" and meta["parent_limit"] == "2" and meta["num_records"] == "80"
    assert [b[0] for b in blocks] == names
    # the same call through Python: every line's set, and its value through the "%f" text
    ctx.load_discrete(codes, arity)
    st, sc = ctx.score_discrete(list(range(20)), [(1 << 20) - 1] * 20, 2, kind=FNML)
    offs, sets, scores = ctx.fetch(st)
    assert sc == 20 * (1 + 19 + 171) and st == sum(len(b[1]) for b in blocks)
    for v, (_, lines) in enumerate(blocks):
        assert [m for _, m in lines] == [int(x) for x in sets[offs[v]:offs[v + 1]]], v
        assert [t for t, _ in lines] == ["%f" % float(s) for s in scores[offs[v]:offs[v + 1]]], v
    # a sample of the values against exact
    for k in range(0, st, 53):
        v = int(np.searchsorted(offs, k, side="right") - 1)
        exact, T, A, nj = exact_fnml(codes, arity, v, int(sets[k]))
        assert abs(float(scores[k]) - exact) <= bound_fk(exact, T, A, nj, arity[v], 80, max(arity)), (v, int(sets[k]))
    net = tmp_path / "net"
    r = subprocess.run([ASTAR, str(pss), "-n", str(net)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
