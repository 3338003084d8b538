"""Discrete BIC on the GPU (ulg_disc_*, `score -f BIC`) against the Python
restatement of the reference in test_discrete.py, within its derived bound B
(see that module's docstring); counts, path identity and list structure are
exact.

B is the error of the reference's float32 summation, which is looser than what
the kernel promises (the exactly summed FP64 value, rounded once).
test_gpu_discrete_shapes.py holds the kernel to that FP64 bound, Bk, and covers
the shapes these small inputs never reach."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ulg
from conftest import PKG
from test_discrete import (HEP, counts_table, n6_case, restated, restated_lists, synthetic)

pytestmark = pytest.mark.gpu

SCORE = os.path.join(PKG, "bin", "score")
ASTAR = os.path.join(PKG, "bin", "astar")
ARITY5 = [2, 3, 2, 4, 3]
SIZES = [2, 63, 64, 65, 257, 1000]


def ulg_status(name):
    return {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}[name]


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


def _all_pairs(n):
    vs, ps = [], []
    for v in range(n):
        others = [p for p in range(n) if p != v]
        for L in range(len(others) + 1):
            for comb in itertools.combinations(others, L):
                vs.append(v)
                ps.append(sum(1 << p for p in comb))
    return vs, ps


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _case5(N):
    return synthetic(5, N, ARITY5, 1000 + N)


# ---- counts -----------------------------------------------------------------
@pytest.mark.parametrize("dense_cells", [16384, 8])
@pytest.mark.parametrize("N", SIZES + [2500])
def test_counts_equal_numpy(ctx, N, dense_cells):
    """N = 2500: the hash table (4N slots) no longer fits LDS and lives in the HBM slab."""
    codes = _case5(N)
    ctx.load_discrete(codes, ARITY5)
    ctx.set_option("disc_dense_cells", dense_cells)
    for v, m in zip(*_all_pairs(5)):
        want, q = counts_table(codes, ARITY5, v, m)
        got = ctx.discrete_counts(v, m)
        assert got.dtype == np.int32 and np.array_equal(got, want), (N, v, m)
    with pytest.raises(ulg.ULGError) as e:
        ctx.discrete_counts(0, 0b11110, cap=2 * 3 * 2 * 4 * 3 - 1)
    assert _status(e) == ulg_status("ARG")


# ---- values -----------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES + [2500])
def test_values_within_bound_and_paths_identical(ctx, N):
    codes = _case5(N)
    vs, ps = _all_pairs(5)
    ctx.load_discrete(codes, ARITY5)
    dense = ctx.score_sets_discrete(vs, ps)
    again = ctx.score_sets_discrete(vs, ps)
    ctx.set_option("disc_dense_cells", 8)
    sparse = ctx.score_sets_discrete(vs, ps)
    sparse2 = ctx.score_sets_discrete(vs, ps)
    assert dense.tobytes() == again.tobytes(), "two dense calls differ"
    assert sparse.tobytes() == sparse2.tobytes(), "two sparse calls differ"
    assert dense.tobytes() == sparse.tobytes(), "dense and sparse paths differ"
    for v, m, got in zip(vs, ps, dense):
        want, _, bound = restated(codes, ARITY5, v, m)
        print(f"N={N} v={v} P={m:#x} gpu={float(got):.6f} ref={float(want):.6f} B={bound:.3g}")
        assert abs(float(got) - float(want)) <= bound, (N, v, m, float(got), float(want), bound)


def test_values_two_records_and_a_constant_column(ctx):
    """N = 2 with the arities its two records really have; variable 4 is constant (R5)."""
    codes = np.array([[0, 0, 1, 0, 0], [1, 1, 0, 1, 0]], dtype=np.uint8)
    arity = [2, 2, 2, 2, 1]
    ctx.load_discrete(codes, arity)
    vs, ps = _all_pairs(5)
    got = ctx.score_sets_discrete(vs, ps)
    for v, m, g in zip(vs, ps, got):
        if arity[v] == 1:
            assert g == 0.0  # R5
            continue
        want, _, bound = restated(codes, arity, v, m)
        assert abs(float(g) - float(want)) <= bound, (v, m, float(g), float(want), bound)


# ---- lists ------------------------------------------------------------------
def _check_lists(ctx, got, want):
    offs, sets, scores = got
    assert len(offs) == len(want) + 1
    for i, lst in enumerate(want):
        s = sets[offs[i]:offs[i + 1]]
        sc = scores[offs[i]:offs[i + 1]]
        assert [int(x) for x in s] == [m for m, _, _ in lst], f"list {i}: sets differ"
        for (m, w, bound), g in zip(lst, sc):
            assert abs(float(g) - float(w)) <= bound, (i, m, float(g), float(w), bound)
    assert offs[-1] == sum(len(lst) for lst in want)


@pytest.fixture(scope="module")
def n6():
    codes, arity = n6_case()
    full = [(1 << 6) - 1] * 6
    return codes, arity, full, restated_lists(codes, arity, range(6), full, 3)


@pytest.mark.parametrize("dense_cells", [16384, 8])
def test_lists_all_candidates(ctx, n6, dense_cells):
    codes, arity, full, want = n6
    ctx.load_discrete(codes, arity)
    ctx.set_option("disc_dense_cells", dense_cells)
    st, sc = ctx.score_discrete(list(range(6)), full, 3)
    assert sc == 6 * (1 + 5 + 10 + 10) and st == sum(len(x) for x in want)
    _check_lists(ctx, ctx.fetch(st), want)
    assert ctx.info("disc_dense_sets") + ctx.info("disc_sparse_sets") == sc
    assert (ctx.info("disc_sparse_sets") > 0) == (dense_cells == 8)


def test_time_limit_checked_per_layer(ctx, n6):
    """A budget the call cannot exhaust: every layer completes and the lists are the same."""
    codes, arity, full, want = n6
    ctx.load_discrete(codes, arity)
    ctx.set_option("time_limit_ms", 600000)
    st, sc = ctx.score_discrete(list(range(6)), full, 3)
    assert ctx.info("out_of_time") == 0 and ctx.info("highest_completed_layer") == 3
    assert sc == 6 * 26
    _check_lists(ctx, ctx.fetch(st), want)


def test_lists_restricted_candidates_and_variable_subset(ctx, n6):
    codes, arity, full, _ = n6
    cand = list(full)
    cand[1] = 0b101001
    cand[4] = 0b000110
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(6)), cand, 3)
    _check_lists(ctx, ctx.fetch(st), restated_lists(codes, arity, range(6), cand, 3))
    st, _ = ctx.score_discrete([4, 1], [cand[4], cand[1]], 2)
    _check_lists(ctx, ctx.fetch(st), restated_lists(codes, arity, [4, 1], [cand[4], cand[1]], 2))


def test_constant_column(ctx, n6):
    codes, arity, full, _ = n6
    codes = codes.copy()
    codes[:, 2] = 0
    arity = list(arity)
    arity[2] = 1
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(6)), full, 3)
    offs, sets, scores = ctx.fetch(st)
    assert offs[3] - offs[2] == 1 and sets[offs[2]] == 0 and scores[offs[2]].tobytes() == np.float32(0.0).tobytes()
    _check_lists(ctx, (offs, sets, scores), restated_lists(codes, arity, range(6), full, 3))


# ---- constraints ------------------------------------------------------------
def test_constraints_remove_violating_sets(ctx, n6):
    codes, arity, full, want = n6
    cons = [(0, 0b000010, 0b000100), (0, 0b001000, 0),  # variable 0: (1 and not 2) or 3
            (3, 0, 0b010001),                           # variable 3: neither 0 nor 4
            (5, 0b000001, 0), (5, 0b000100, 0b000001)]  # variable 5: every alternative requires a parent
    ctx.load_discrete(codes, arity)
    st0, _ = ctx.score_discrete(list(range(6)), full, 3)
    plain = ctx.fetch(st0)
    ctx.set_constraints(cons)
    st, _ = ctx.score_discrete(list(range(6)), full, 3)
    offs, sets, scores = ctx.fetch(st)
    wantc = restated_lists(codes, arity, range(6), full, 3, constraints=cons)
    _check_lists(ctx, (offs, sets, scores), wantc)
    assert 0 not in [int(x) for x in sets[offs[5]:offs[6]]]  # 1 < 1 fails: the empty set is absent
    # exactly the unconstrained lists minus the violating sets, values bit for bit
    po, ps_, pv = plain
    for v in range(6):
        keep = {m for m, _, _ in wantc[v]}
        sel = [k for k in range(po[v], po[v + 1]) if int(ps_[k]) in keep]
        assert [int(ps_[k]) for k in sel] == [int(x) for x in sets[offs[v]:offs[v + 1]]]
        assert pv[sel].tobytes() == scores[offs[v]:offs[v + 1]].tobytes()
    # calculateScore returns 1 for a violating set
    assert ctx.score_sets_discrete([5, 5], [0, 0b000010]).tolist() == [1.0, 1.0]
    ctx.clear_constraints()
    st2, _ = ctx.score_discrete(list(range(6)), full, 3)
    again = ctx.fetch(st2)
    assert st2 == st0 and all(a.tobytes() == b.tobytes() for a, b in zip(again, plain))
    # a load of either kind clears them
    ctx.set_constraints(cons)
    ctx.load_discrete(codes, arity)
    assert ctx.info("constraints") == 0


# ---- errors -----------------------------------------------------------------
def test_errors_leave_the_lists(ctx, n6):
    codes, arity, full, _ = n6
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete([0], [1], 1)
    assert _status(e) == ulg_status("STATE")
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets_discrete([0], [0])
    assert _status(e) == ulg_status("STATE")
    ctx.load_discrete(codes, arity)
    with pytest.raises(ulg.ULGError) as e:
        ctx.score(list(range(6)), full, 3)
    assert _status(e) == ulg_status("STATE")
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets([0], [2])
    assert _status(e) == ulg_status("STATE")
    st, _ = ctx.score_discrete(list(range(6)), full, 2)
    before = ctx.fetch(st)

    def same_lists():
        return all(a.tobytes() == b.tobytes() for a, b in zip(ctx.fetch(st), before))

    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete(list(range(6)), full, 3, kind=2)
    assert _status(e) == ulg_status("ARG") and same_lists()
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets_discrete([0], [2], kind=2)
    assert _status(e) == ulg_status("ARG") and same_lists()
    for bad in (0, 256):
        ar = list(arity)
        ar[3] = bad
        with pytest.raises(ulg.ULGError) as e:
            ctx.load_discrete(codes, ar)
        assert _status(e) == ulg_status("ARG") and same_lists()
    # the refused loads above changed nothing: the records are still there
    st_b, _ = ctx.score_discrete(list(range(6)), full, 2)
    assert st_b == st and same_lists()
    # 9 parents of arity 255: 255^10 cells
    big = (np.arange(300)[:, None] * np.arange(1, 11)[None, :] % 255).astype(np.uint8)
    c2 = ulg.Context(0)
    try:
        c2.load_discrete(big, [255] * 10)
        with pytest.raises(ulg.ULGError) as e:
            c2.score_discrete(list(range(10)), [(1 << 10) - 1] * 10, 9)
        assert _status(e) == ulg_status("UNSUPPORTED")
        with pytest.raises(ulg.ULGError) as e:
            c2.score_sets_discrete([0], [0b1111111110])
        assert _status(e) == ulg_status("UNSUPPORTED")
        with pytest.raises(ulg.ULGError) as e:
            c2.discrete_counts(0, 0b1111111110, cap=10)
        assert _status(e) == ulg_status("UNSUPPORTED")
    finally:
        c2.close()
    # a code >= its arity is caught on the device; the lists stay, the data does not
    badc = codes.copy()
    badc[77, 1] = arity[1]
    with pytest.raises(ulg.ULGError) as e:
        ctx.load_discrete(badc, arity)
    assert _status(e) == ulg_status("ARG") and same_lists()
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete(list(range(6)), full, 2)
    assert _status(e) == ulg_status("STATE") and same_lists()


def test_continuous_load_replaces_discrete(ctx, n6):
    codes, arity, full, _ = n6
    ctx.load_discrete(codes, arity)
    ctx.load(np.random.default_rng(3).normal(size=(50, 4)), 2.0)
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete([0], [0b1110], 1)
    assert _status(e) == ulg_status("STATE")
    assert ctx.score([0], [0b1110], 2)[1] == 1 + 3 + 3


# ---- pipeline ---------------------------------------------------------------
def test_search_on_discrete_lists(ctx, n6, oracle_built):
    o = oracle_built
    codes, arity, full, _ = n6
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(6)), full, 3)
    offs, sets, scores = ctx.fetch(st)
    ctx.search_from_scores()
    res = ctx.astar(mode=0)
    costs = np.array([o.quantize(float(s)) for s in scores], dtype=np.float32)
    ref = o.Search(6, offs, sets, costs).astar()
    assert ref["rc"] == 0
    assert [int(x) for x in res["vpar"]] == [int(x) for x in ref["vpar"]]
    assert list(res["order"]) == list(ref["order"])
    assert np.float32(res["cost"]).tobytes() == np.float32(ref["cost"]).tobytes()
    assert res["expanded"] == ref["expanded"]


# ---- command line -----------------------------------------------------------
def _read_pss_text(path):
    meta, blocks, cur = {}, [], None
    for ln in open(path).read().splitlines():
        if ln.startswith("META ") and cur is None:
            k, _, v = ln[5:].partition("=")
            meta[k.strip()] = v.strip()
        elif ln.startswith("VAR "):
            cur = {"name": ln[4:].strip(), "lines": []}
            blocks.append(cur)
        elif cur is not None and ln.strip() and not ln.startswith("META"):
            tok = ln.split()
            cur["lines"].append((float(tok[0]), tok[1:]))
    return meta, blocks


def _hepatitis():
    rows = [ln.strip().split(",") for ln in open(HEP).read().splitlines()]
    names, rows = rows[0], rows[1:]
    maps = [dict() for _ in names]
    codes = np.array([[maps[c].setdefault(r[c], len(maps[c])) for c in range(len(names))] for r in rows],
                     dtype=np.uint8)
    return names, codes, [len(m) for m in maps]


def test_score_command_line_default_is_bic(tmp_path, oracle_built):
    o = oracle_built
    pss = tmp_path / "hep.pss"
    r = subprocess.run([SCORE, HEP, str(pss), "-s"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"function": "bic"' in r.stderr
    meta, blocks = _read_pss_text(pss)
    assert meta["score_type"] == "bic" and meta["parent_limit"] == "3" and meta["num_records"] == "80"
    assert int(math.log(160 / math.log(80))) == 3
    names, codes, arity = _hepatitis()
    assert [b["name"] for b in blocks] == names
    index = {nm: i for i, nm in enumerate(names)}
    per_var = sum(math.comb(19, L) for L in range(4))
    assert per_var == 1160
    for v, b in enumerate(blocks):
        assert len(b["lines"]) == per_var, (v, len(b["lines"]))
        others = [p for p in range(20) if p != v]
        order = [sum(1 << p for p in comb) for L in range(4)
                 for comb in sorted(itertools.combinations(others, L), key=lambda c: sum(1 << p for p in c))]
        for (val, pnames), m in zip(b["lines"], order):
            assert sum(1 << index[x] for x in pnames) == m
            want, _, bound = restated(codes, arity, v, m)
            assert abs(val - float(want)) <= bound + 5e-7, (v, m, val, float(want), bound)
    # the search side runs on the discrete .pss as on any other
    net, ref_net = tmp_path / "net", tmp_path / "ref_net"
    r = subprocess.run([ASTAR, str(pss), "-n", str(net)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    subprocess.run([o.REF_ASTAR, str(pss), "-n", str(ref_net)], check=True, stdout=subprocess.DEVNULL, timeout=300)
    assert net.read_text() == ref_net.read_text()
    assert open(str(net) + ".csv").read() == open(str(ref_net) + ".csv").read()


def test_score_command_line_options(tmp_path):
    pss = tmp_path / "p2.pss"
    r = subprocess.run([SCORE, HEP, str(pss), "-s", "-f", "BIC", "-p", "2", "--lambda", "7"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    meta, blocks = _read_pss_text(pss)
    assert meta["parent_limit"] == "2" and all(len(b["lines"]) == 1 + 19 + 171 for b in blocks)
    # without -s the first line is a record: N = 81
    r = subprocess.run([SCORE, HEP, str(pss)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert _read_pss_text(pss)[0]["num_records"] == "81"
    cons = tmp_path / "cons.txt"
    cons.write_text("nosuchname ( !age )\n")
    out = tmp_path / "c.pss"
    r = subprocess.run([SCORE, HEP, str(out), "-s", "-c", str(cons)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "nosuchname" in r.stderr and not out.exists()
    assert "ulg_metrics" not in r.stderr
