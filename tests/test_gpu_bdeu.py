"""BDeu on the GPU (ULG_SCORE_BDEU, ulg_disc_set_ess, `score --bdeu`) against
test_bdeu.py: within B of the restatement of the reference's float arithmetic,
within Ek of the exact FP64 value (both bounds are derived in that module's
docstring), and bit-identical across the dense and sparse counting paths,
repeated calls and launch shapes.  Sets, counts and list structure are exact."""
import math
import os
import re
import subprocess
import time

import numpy as np
import pytest

import ulg
from conftest import PKG
from test_bdeu import (ARITY5, SIZES5, all_pairs, bdeu_shift, bound_b, bound_ek, case5, cases5, exact_bdeu,
                       reference5, restated_bdeu, restated_bdeu_lists, shape_exact)
from test_disc_prune import apply_rule
from test_discrete import HEP, N_G, SETS_A, n6_case, q_of, shape_input, shape_pairs

pytestmark = pytest.mark.gpu

SCORE = os.path.join(PKG, "bin", "score")
ASTAR = os.path.join(PKG, "bin", "astar")
BDEU = ulg.Context.SCORE_BDEU
STATUS = {"ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- values -------------------------------------------------------------------------
@pytest.mark.parametrize("N,ess", cases5())
def test_values_within_bounds_and_paths_identical(ctx, N, ess):
    """All 80 (v, P) of the 5-variable case; N = 2500: the hash table leaves LDS for the HBM slab."""
    codes = case5(N)
    vs, ps = all_pairs(5)
    assert len(vs) == 80 and N in SIZES5
    ctx.load_discrete(codes, ARITY5)
    dense = ctx.score_sets_discrete(vs, ps, kind=BDEU, ess=ess)
    again = ctx.score_sets_discrete(vs, ps, kind=BDEU)
    ctx.set_option("disc_dense_cells", 8)
    sparse = ctx.score_sets_discrete(vs, ps, kind=BDEU)
    sparse2 = ctx.score_sets_discrete(vs, ps, kind=BDEU)
    assert dense.tobytes() == again.tobytes(), "two dense calls differ"
    assert sparse.tobytes() == sparse2.tobytes(), "two sparse calls differ"
    assert dense.tobytes() == sparse.tobytes(), "dense and sparse paths differ"
    wb = wk = 0.0
    for v, m, got, (want, _, exact, T, A) in zip(vs, ps, dense, reference5(N, ess)):
        B, ek = bound_b(exact, T, A), bound_ek(exact, T, A, N, ess)
        print(f"N={N} ess={ess} v={v} P={m:#x} gpu={float(got):.6f} ref={float(want):.6f} exact={exact:.9f} "
              f"B={B:.3g} Ek={ek:.3g}")
        assert abs(float(got) - float(want)) <= B, (N, ess, v, m, float(got), float(want), B)
        assert abs(float(got) - exact) <= ek, (N, ess, v, m, float(got), exact, ek)
        wb, wk = max(wb, abs(float(got) - float(want)) / B), max(wk, abs(float(got) - exact) / ek)
    print(f"N={N} ess={ess}: at most {wb:.3f} B from the restatement, {wk:.3f} Ek from exact")


def test_values_two_records_and_a_constant_column(ctx):
    """N = 2 with the arities its two records really have; variable 4 is constant (R5: +0.0)."""
    codes = np.array([[0, 0, 1, 0, 0], [1, 1, 0, 1, 0]], dtype=np.uint8)
    arity = [2, 2, 2, 2, 1]
    ctx.load_discrete(codes, arity)
    vs, ps = all_pairs(5)
    got = ctx.score_sets_discrete(vs, ps, kind=BDEU, ess=1.0)
    for v, m, g in zip(vs, ps, got):
        if arity[v] == 1:
            assert g.tobytes() == np.float32(0.0).tobytes()  # +0.0: the sign bit too
            continue
        want, _ = restated_bdeu(codes, arity, v, m, 1.0)
        exact, T, A = exact_bdeu(codes, arity, v, m, 1.0)
        assert abs(float(g) - float(want)) <= bound_b(exact, T, A), (v, m, float(g), float(want))
        assert abs(float(g) - exact) <= bound_ek(exact, T, A, 2, 1.0), (v, m, float(g), exact)


# ---- lists --------------------------------------------------------------------------
def _check_lists(got, want):
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
    return codes, arity, full, restated_bdeu_lists(codes, arity, range(6), full, 3, 1.0)


def test_lists_all_candidates_on_both_paths(ctx, n6):
    codes, arity, full, want = n6
    ctx.load_discrete(codes, arity)
    got = {}
    for dense_cells in (16384, 8):
        ctx.set_option("disc_dense_cells", dense_cells)
        st, sc = ctx.score_discrete(list(range(6)), full, 3, kind=BDEU, ess=1.0)
        assert sc == 6 * (1 + 5 + 10 + 10) and st == sum(len(x) for x in want)
        got[dense_cells] = ctx.fetch(st)
        _check_lists(got[dense_cells], want)
        assert ctx.info("disc_dense_sets") + ctx.info("disc_sparse_sets") == sc
        assert (ctx.info("disc_sparse_sets") > 0) == (dense_cells == 8)
        assert ctx.info("out_of_time") == 0 and ctx.info("highest_completed_layer") == 3
    assert _same(got[16384], got[8])
    # the same pairs through ulg_disc_score_sets: bit for bit
    offs, sets, scores = got[8]
    vs = [v for v in range(6) for _ in range(offs[v], offs[v + 1])]
    assert ctx.score_sets_discrete(vs, sets, kind=BDEU).tobytes() == scores.tobytes()


def test_lists_restricted_candidates_and_variable_subset(ctx, n6):
    codes, arity, full, _ = n6
    cand = list(full)
    cand[1] = 0b101001
    cand[4] = 0b000110
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(6)), cand, 3, kind=BDEU, ess=1.0)
    _check_lists(ctx.fetch(st), restated_bdeu_lists(codes, arity, range(6), cand, 3, 1.0))
    st, _ = ctx.score_discrete([4, 1], [cand[4], cand[1]], 2, kind=BDEU)
    _check_lists(ctx.fetch(st), restated_bdeu_lists(codes, arity, [4, 1], [cand[4], cand[1]], 2, 1.0))


def test_lists_with_constraints(ctx, n6):
    codes, arity, full, want = n6
    cons = [(0, 0b000010, 0b000100), (0, 0b001000, 0),  # variable 0: (1 and not 2) or 3
            (3, 0, 0b010001),                           # variable 3: neither 0 nor 4
            (5, 0b000001, 0), (5, 0b000100, 0b000001)]  # variable 5: every alternative requires a parent
    ctx.load_discrete(codes, arity)
    st0, _ = ctx.score_discrete(list(range(6)), full, 3, kind=BDEU, ess=1.0)
    plain = ctx.fetch(st0)
    ctx.set_constraints(cons)
    st, _ = ctx.score_discrete(list(range(6)), full, 3, kind=BDEU)
    offs, sets, scores = ctx.fetch(st)
    wantc = restated_bdeu_lists(codes, arity, range(6), full, 3, 1.0, constraints=cons)
    _check_lists((offs, sets, scores), wantc)
    assert st < st0 and 0 not in [int(x) for x in sets[offs[5]:offs[6]]]
    po, ps_, pv = plain
    for v in range(6):  # the unconstrained lists minus the violating sets, values bit for bit
        keep = {m for m, _, _ in wantc[v]}
        sel = [k for k in range(po[v], po[v + 1]) if int(ps_[k]) in keep]
        assert [int(ps_[k]) for k in sel] == [int(x) for x in sets[offs[v]:offs[v + 1]]]
        assert pv[sel].tobytes() == scores[offs[v]:offs[v + 1]].tobytes()
    assert ctx.score_sets_discrete([5, 5], [0, 0b000010], kind=BDEU).tolist() == [1.0, 1.0]  # R6


def test_ess_is_sticky_and_survives_a_load(ctx, n6):
    codes, arity, full, _ = n6
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(6)), full, 3, kind=BDEU, ess=1.0)
    one = ctx.fetch(st)
    ctx.set_ess(4.0)
    ctx.load_discrete(codes, arity)
    st4, _ = ctx.score_discrete(list(range(6)), full, 3, kind=BDEU)  # ess = 4 survived the load
    four = ctx.fetch(st4)
    assert four[2].tobytes() != one[2].tobytes()
    _check_lists(four, restated_bdeu_lists(codes, arity, range(6), full, 3, 4.0))
    # BIC does not read it
    bic = ctx.score_sets_discrete([0, 3], [0b10, 0b110])
    ctx.set_ess(1.0)
    assert ctx.score_sets_discrete([0, 3], [0b10, 0b110]).tobytes() == bic.tobytes()
    ctx.load_discrete(codes, arity)
    st1, _ = ctx.score_discrete(list(range(6)), full, 3, kind=BDEU)
    assert st1 == st and _same(ctx.fetch(st1), one)


@pytest.mark.parametrize("dense_cells", [16384, 8])
def test_prune_with_bdeu(ctx, n6, dense_cells):
    """Option disc_prune on the BDeu lists: the kept sets are test_disc_prune.prune_rule applied to the
    fetched unpruned lists, bit for bit, and disc_pruned counts the rest."""
    codes, arity, full, _ = n6
    ctx.load_discrete(codes, arity)
    ctx.set_option("disc_dense_cells", dense_cells)
    st0, sc0 = ctx.score_discrete(list(range(6)), full, 3, kind=BDEU, prune=False, ess=1.0)
    plain = ctx.fetch(st0)
    assert ctx.info("disc_pruned") == 0
    st1, sc1 = ctx.score_discrete(list(range(6)), full, 3, kind=BDEU, prune=True)
    pruned = ctx.fetch(st1)
    assert sc1 == sc0 and ctx.info("disc_pruned") == st0 - st1 and 0 < st1 < st0
    assert _same(pruned, apply_rule(*plain))


# ---- shapes ---------------------------------------------------------------------------
def _within(name, vs, ps, got, what=""):
    N = shape_input(name)[0].shape[0]
    worst = 0.0
    for v, m, g in zip(vs, ps, got):
        e, T, A = shape_exact(name, int(v), int(m))
        ek = bound_ek(e, T, A, N, 1.0)
        assert abs(float(g) - e) <= ek, (name, what, int(v), hex(int(m)), float(g), e, ek)
        worst = max(worst, abs(float(g) - e) / ek)
    print(f"{name} {what}: {len(vs)} values, at most {worst:.3f} Ek")


@pytest.mark.parametrize("name", ["b1500", "b2100"])
def test_b_sparse_tables_at_natural_size(ctx, name):
    """Arities 255 and 200, tables of 1.3e7, 2.1e8 and 5.5e16 cells: a_jk = ess / (q r) goes below 2^-53,
    where a_jk + n rounds to n.  The hash table in LDS (N = 1500) and in the HBM slab (N = 2100); the
    small tables of the same records on both paths."""
    codes, arity = shape_input(name)
    vs, ps = shape_pairs(name)
    assert 1.0 / (q_of(arity, vs[2], ps[2]) * arity[vs[2]]) < 2.0 ** -53
    ctx.load_discrete(codes, arity)
    got = ctx.score_sets_discrete(vs, ps, kind=BDEU, ess=1.0)
    _within(name, vs, ps, got)
    assert ctx.score_sets_discrete(vs[::-1], ps[::-1], kind=BDEU)[::-1].tobytes() == got.tobytes()
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete(vs, ps, kind=BDEU).tobytes() == got.tobytes(), "dense and sparse paths differ"


def test_c_more_items_than_the_grid(ctx):
    """2560 tables split between the histogram and the hash table by disc_dense_cells = 64, then 7680
    items over 2048 workgroups, then every other split."""
    codes, arity = shape_input("c300")
    vs, ps = shape_pairs("c300")
    perm = np.random.default_rng(7).permutation(len(vs))
    pv, pp = [vs[i] for i in perm], [ps[i] for i in perm]
    ctx.load_discrete(codes, arity)
    ctx.set_option("disc_dense_cells", 64)
    got = ctx.score_sets_discrete(pv, pp, kind=BDEU, ess=1.0)
    _within("c300", pv, pp, got, "2560 shuffled items")
    three = ctx.score_sets_discrete(pv * 3, pp * 3, kind=BDEU)
    assert len(three) == 7680 and three.tobytes() == np.tile(got, 3).tobytes()
    for limit in (16384, 512, 8):
        ctx.set_option("disc_dense_cells", limit)
        assert ctx.score_sets_discrete(pv * 3, pp * 3, kind=BDEU).tobytes() == three.tobytes(), limit
    # the layers of score_discrete give the same values
    st, sc = ctx.score_discrete(list(range(10)), [1023] * 10, 4, kind=BDEU)
    offs, sets, scores = ctx.fetch(st)
    value = {(v, m): g for v, m, g in zip(pv, pp, got)}
    assert sc == 2560 and st == sum(1 for g in got if g < 0)  # no empty-set value reaches 1 here
    for v in range(10):
        for m, s in zip(sets[offs[v]:offs[v + 1]], scores[offs[v]:offs[v + 1]]):
            assert s.tobytes() == value[(v, int(m))].tobytes()


def test_f_variables_and_parents_from_bit_32_up(ctx):
    codes, arity = shape_input("f")
    vs, ps = shape_pairs("f")
    assert max(vs) == 43 and any(m >> 32 for m in ps)
    ctx.load_discrete(codes, arity)
    got = ctx.score_sets_discrete(vs, ps, kind=BDEU, ess=1.0)
    _within("f", vs, ps, got)
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete(vs, ps, kind=BDEU).tobytes() == got.tobytes()


def test_a_dense_limit(ctx):
    """Tables of 192 to 16384 cells in the LDS histogram, 49152 cells on the hash path at default
    options, in LDS as well with disc_dense_cells = 32768, and everything hashed with 8."""
    codes, arity = shape_input("a")
    vs, ps = shape_pairs("a")
    assert [q_of(arity, v, m) * arity[v] for v, m in SETS_A][7:] == [16384, 49152, 49152]
    ctx.load_discrete(codes, arity)
    default = ctx.score_sets_discrete(vs, ps, kind=BDEU, ess=1.0)
    _within("a", vs, ps, default, "default options")
    for limit in (32768, 8):
        ctx.set_option("disc_dense_cells", limit)
        assert ctx.score_sets_discrete(vs, ps, kind=BDEU).tobytes() == default.tobytes(), limit


def test_g_where_the_scale_drops(ctx):
    """N = 62,000,000 (the one slow test, a few seconds): bdeu_shift leaves 2^32."""
    t0 = time.perf_counter()
    codes, arity = shape_input("g")
    assert bdeu_shift(N_G, 1.0) < 32
    ctx.load_discrete(codes, arity)
    vs, ps = shape_pairs("g")
    got = ctx.score_sets_discrete(vs, ps, kind=BDEU, ess=1.0)
    for v, m, g in zip(vs, ps, got):
        e, T, A = shape_exact("g", v, m)
        ek = bound_ek(e, T, A, N_G, 1.0)
        print(f"g: v={v} P={m:#x} gpu={float(g):.1f} exact={e:.3f} Ek={ek:.3g}")
        assert abs(float(g) - e) <= ek, (v, m, float(g), e, ek)
    assert ctx.score_sets_discrete(vs, ps, kind=BDEU).tobytes() == got.tobytes()
    print(f"g: {time.perf_counter() - t0:.1f} s")


# ---- errors ---------------------------------------------------------------------------
def test_errors_leave_the_lists_and_the_ess(ctx, n6):
    codes, arity, full, _ = n6
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete([0], [1], 1, kind=BDEU)
    assert _status(e) == STATUS["STATE"]
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(6)), full, 2, kind=BDEU, ess=2.0)
    before = ctx.fetch(st)
    probe = ctx.score_sets_discrete([0, 2], [0b110, 0b1], kind=BDEU)

    def same():
        return _same(ctx.fetch(st), before)

    for kind in (2, 0, 4):
        with pytest.raises(ulg.ULGError) as e:
            ctx.score_discrete(list(range(6)), full, 3, kind=kind)
        assert _status(e) == STATUS["ARG"] and same()
        with pytest.raises(ulg.ULGError) as e:
            ctx.score_sets_discrete([0], [2], kind=kind)
        assert _status(e) == STATUS["ARG"] and same()
    for bad in (0.0, float("nan"), 1e7, -1.0, float("inf"), 1e-7):
        with pytest.raises(ulg.ULGError) as e:
            ctx.set_ess(bad)
        assert _status(e) == STATUS["ARG"] and same()
        with pytest.raises(ulg.ULGError) as e:
            ctx.score_discrete(list(range(6)), full, 2, kind=BDEU, ess=bad)
        assert _status(e) == STATUS["ARG"] and same()
        # the previous ess, 2.0, is still the one in use
        assert ctx.score_sets_discrete([0, 2], [0b110, 0b1], kind=BDEU).tobytes() == probe.tobytes()
    for ok in (1e-6, 1e6):
        ctx.set_ess(ok)
    # BDeu after a continuous load
    ctx.load(np.random.default_rng(3).normal(size=(50, 4)), 2.0)
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete([0], [0b1110], 1, kind=BDEU)
    assert _status(e) == STATUS["STATE"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets_discrete([0], [0b10], kind=BDEU)
    assert _status(e) == STATUS["STATE"]
    # 9 parents of arity 255: 255^10 cells
    big = (np.arange(300)[:, None] * np.arange(1, 11)[None, :] % 255).astype(np.uint8)
    ctx.load_discrete(big, [255] * 10)
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_discrete(list(range(10)), [(1 << 10) - 1] * 10, 9, kind=BDEU)
    assert _status(e) == STATUS["UNSUPPORTED"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets_discrete([0], [0b1111111110], kind=BDEU)
    assert _status(e) == STATUS["UNSUPPORTED"]


# ---- pipeline and command line ----------------------------------------------------------
def _hepatitis():
    rows = [ln.strip().split(",") for ln in open(HEP).read().splitlines()]
    names, rows = rows[0], rows[1:]
    maps = [dict() for _ in names]
    codes = np.array([[maps[c].setdefault(r[c], len(maps[c])) for c in range(len(names))] for r in rows],
                     dtype=np.uint8)
    return names, codes, [len(m) for m in maps]


def test_score_command_line_bdeu(ctx, tmp_path, oracle_built):
    o = oracle_built
    pss = tmp_path / "hep.pss"
    r = subprocess.run([SCORE, HEP, str(pss), "-s", "--bdeu", "-e", "1", "-p", "3"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"function": "bdeu"' in r.stderr and '"ess": 1' in r.stderr
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
    assert meta["score_type"] == "bdeu" and meta["ess"] == "1" and meta["parent_limit"] == "3"
    assert meta["num_records"] == "80" and [b[0] for b in blocks] == names
    # the same call through Python: every line's set, and its value through the "%f" text
    ctx.load_discrete(codes, arity)
    st, sc = ctx.score_discrete(list(range(20)), [(1 << 20) - 1] * 20, 3, kind=BDEU, ess=1.0)
    offs, sets, scores = ctx.fetch(st)
    assert sc == 20 * 1160 and st == sum(len(b[1]) for b in blocks)
    for v, (_, lines) in enumerate(blocks):
        assert [m for _, m in lines] == [int(x) for x in sets[offs[v]:offs[v + 1]]], v
        assert [t for t, _ in lines] == ["%f" % float(s) for s in scores[offs[v]:offs[v + 1]]], v
    # a sample of the values against exact
    for k in range(0, st, 97):
        v = int(np.searchsorted(offs, k, side="right") - 1)
        exact, T, A = exact_bdeu(codes, arity, v, int(sets[k]), 1.0)
        assert abs(float(scores[k]) - exact) <= bound_ek(exact, T, A, 80, 1.0), (v, int(sets[k]))
    # astar accepts the file; the search on the same lists equals the oracle's, and its DAG re-scores to its cost
    net = tmp_path / "net"
    r = subprocess.run([ASTAR, str(pss), "-n", str(net)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ctx.search_from_scores()
    res = ctx.astar(mode=0)
    costs = np.array([o.quantize(float(s)) for s in scores], dtype=np.float32)
    ref = o.Search(20, offs, sets, costs).astar()
    assert ref["rc"] == 0
    assert [int(x) for x in res["vpar"]] == [int(x) for x in ref["vpar"]]
    assert np.float32(res["cost"]).tobytes() == np.float32(ref["cost"]).tobytes()
    lookup = [{int(m): float(c) for m, c in zip(sets[offs[v]:offs[v + 1]], costs[offs[v]:offs[v + 1]])} for v in range(20)]
    total = math.fsum(lookup[v][int(res["vpar"][v])] for v in range(20))
    assert abs(total - float(res["cost"])) <= 1e-5 * abs(total)


def test_score_command_line_bdeu_without_p_has_no_bic_limit(tmp_path):
    """The BIC limit at N = 80 is 3; --bdeu -p 4 is taken as given, and --prune reports its sizes."""
    pss = tmp_path / "p4.pss"
    r = subprocess.run([SCORE, HEP, str(pss), "-s", "--bdeu", "-e", "0.5", "-p", "4", "--prune"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    head = open(pss).read(2000).replace(" ", "")
    assert "parent_limit=4" in head and "ess=0.5" in head and "score_type=bdeu" in head
    assert "Size before pruning" in r.stdout and '"pruned"' in r.stderr and '"ess": 0.5' in r.stderr
