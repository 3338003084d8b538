"""The prune pass of the discrete scorer on the GPU (option "disc_prune",
`score --prune`; DESIGN R8).

The yardstick of every list check: the same call is scored twice on one
context, with prune=False and with prune=True.  The scorer's values do not
depend on scheduling, so the pruned lists must equal -- bit for bit in sets,
order, scores and offsets -- test_disc_prune.prune_rule applied in float32 to
the unpruned lists that were fetched.  No tolerance anywhere."""
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ulg
from conftest import PKG
from test_disc_prune import apply_rule, xor8
from test_discrete import HEP, n6_case, parents_of, shape_input
from test_gpu_discrete import _hepatitis, _status, ulg_status

pytestmark = pytest.mark.gpu

SCORE = os.path.join(PKG, "bin", "score")
ASTAR = os.path.join(PKG, "bin", "astar")
XOR_BITS = [0, 9, 17, 31, 32, 47, 61, 62]


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _lists(got):
    offs, sets, scores = got
    return [([int(m) for m in sets[offs[i]:offs[i + 1]]], scores[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]


def yardstick(ctx, variables, cands, k, rule_on=None):
    """Scores the call unpruned and pruned -> (unpruned lists, pruned lists), the yardstick asserted
    (rule_on: only for these list positions)."""
    st0, sc0 = ctx.score_discrete(variables, cands, k, prune=False)
    plain = ctx.fetch(st0)
    assert ctx.info("disc_pruned") == 0
    st1, sc1 = ctx.score_discrete(variables, cands, k, prune=True)
    pruned = ctx.fetch(st1)
    assert sc1 == sc0 and ctx.info("disc_pruned") == st0 - st1
    assert plain[0][-1] == st0 and pruned[0][-1] == st1
    if rule_on is None:
        assert _same(pruned, apply_rule(*plain))
    else:
        po, ps, pv = plain
        qo, qs, qv = pruned
        for i in rule_on:
            o, s, v = apply_rule(po[i:i + 2] - po[i], ps[po[i]:po[i + 1]], pv[po[i]:po[i + 1]])
            assert qo[i + 1] - qo[i] == o[1], i
            assert _same((qs[qo[i]:qo[i + 1]], qv[qo[i]:qo[i + 1]]), (s, v)), i
    return plain, pruned


@pytest.fixture(scope="module")
def xor_lists():
    """Test 4's call, shared: xor8(1500, 11), full candidates, k = 4 -> (unpruned, pruned)."""
    codes, arity = xor8(1500, 11)
    c = ulg.Context(0)
    try:
        c.load_discrete(codes, arity)
        plain, pruned = yardstick(c, list(range(8)), [(1 << 8) - 1] * 8, 4)
    finally:
        c.close()
    for a in plain + pruned:
        a.setflags(write=False)
    return plain, pruned


# ---- 1-8: lists -----------------------------------------------------------------
@pytest.mark.parametrize("dense_cells", [16384, 8])
def test_n6_all_candidates(ctx, dense_cells):
    codes, arity = n6_case()
    ctx.load_discrete(codes, arity)
    ctx.set_option("disc_dense_cells", dense_cells)
    plain, pruned = yardstick(ctx, list(range(6)), [(1 << 6) - 1] * 6, 3)
    assert len(pruned[1]) < len(plain[1]) == 156
    assert all(abs(float(s)) >= 4 for s in plain[2])  # where the rule is the reference's sort-and-scan
    with pytest.raises(ulg.ULGError) as e:
        ctx.set_option("disc_prune", 2)
    assert _status(e) == ulg_status("ARG")
    with pytest.raises(ulg.ULGError) as e:
        ctx.set_option("disc_prune", -1)
    assert _status(e) == ulg_status("ARG")
    # the refused values left the option on
    st, _ = ctx.score_discrete(list(range(6)), [(1 << 6) - 1] * 6, 3)
    assert st == len(pruned[1])


def test_n6_restricted_candidates_and_variable_subset(ctx):
    """Compact positions differ from variable indices, and vars from range(n)."""
    codes, arity = n6_case()
    cand = [(1 << 6) - 1] * 6
    cand[1] = 0b101001
    cand[4] = 0b000110
    ctx.load_discrete(codes, arity)
    plain, pruned = yardstick(ctx, list(range(6)), cand, 3)
    assert len(pruned[1]) < len(plain[1])
    plain, pruned = yardstick(ctx, [4, 1], [cand[4], cand[1]], 2)
    assert len(pruned[1]) < len(plain[1])


def test_domination_passes_through_holes(ctx):
    """Variable 5 must hold both of {0, 1} or neither: {0} and {1} and their supersets without the
    other are never stored, and {} still prunes {0, 1}."""
    codes, arity = n6_case()
    ctx.load_discrete(codes, arity)
    ctx.set_constraints([(5, 0b000011, 0), (5, 0, 0b000011)])
    plain, pruned = yardstick(ctx, list(range(6)), [(1 << 6) - 1] * 6, 3)
    before, after = _lists(plain)[5][0], _lists(pruned)[5][0]
    assert not any(bin(m & 0b11).count("1") == 1 for m in before)  # the holes
    assert 0b000011 in before and 0b000011 not in after
    assert after == [0, 1 << 3, 1 << 4]


def test_parity_input(xor_lists):
    plain, pruned = xor_lists
    assert len(plain[1]) == 792 and len(pruned[1]) < 792
    sizes = [len(parents_of(int(m))) for m in pruned[1]]
    assert max(sizes) >= 3
    assert all(abs(float(s)) >= 4 for s in plain[2])


def test_wide_masks(ctx, xor_lists):
    """The parity input's columns at bits up to 62 of a 63-column input whose other columns are
    constant: compact positions 0..7 stand for variables up to 62."""
    codes8, arity8 = xor8(1500, 11)
    codes = np.zeros((1500, 63), dtype=np.uint8)
    arity = [1] * 63
    for j, b in enumerate(XOR_BITS):
        codes[:, b] = codes8[:, j]
        arity[b] = arity8[j]
    cand = sum(1 << b for b in XOR_BITS)
    ctx.load_discrete(codes, arity)
    plain, pruned = yardstick(ctx, list(range(63)), [cand] * 63, 4)
    small = _lists(xor_lists[1])
    wide = _lists(pruned)
    for v in range(63):
        masks, scores = wide[v]
        if v not in XOR_BITS:
            assert masks == [0] and scores.tobytes() == np.float32(0.0).tobytes(), v
            continue
        smasks, sscores = small[XOR_BITS.index(v)]
        assert masks == [sum(1 << XOR_BITS[p] for p in parents_of(m)) for m in smasks], v
        assert scores.tobytes() == sscores.tobytes(), v


def test_more_items_than_one_pass_of_the_grid(ctx):
    """Input e: layers of 109,620 and 712,530 slots against 2048 x 256 threads per launch."""
    codes, arity = shape_input("e")
    ctx.load_discrete(codes, arity)
    plain, pruned = yardstick(ctx, list(range(30)), [(1 << 30) - 1] * 30, 4, rule_on=[0, 13, 29])
    assert len(plain[1]) == 28 * 27841 + 2
    po, ps, pv = plain
    qo, qs, qv = pruned
    for v in range(30):
        a, b = ps[po[v]:po[v + 1]], qs[qo[v]:qo[v + 1]]
        order = np.argsort(a, kind="stable")
        at = np.searchsorted(a[order], b)
        assert (at < len(a)).all(), v
        idx = order[at]
        assert np.array_equal(a[idx], b), v
        assert (np.diff(idx) > 0).all(), v  # a subsequence: the order is the unpruned list's
        assert pv[po[v]:po[v + 1]][idx].tobytes() == qv[qo[v]:qo[v + 1]].tobytes(), v


def _upto(got, layer):
    """The fetched lists without the sets of more than `layer` parents."""
    offs, sets, scores = got
    keep = np.array([len(parents_of(int(m))) <= layer for m in sets], dtype=bool)
    new = [int(keep[:o].sum()) for o in offs]
    return np.asarray(new, dtype=offs.dtype), sets[keep], scores[keep]


@pytest.mark.parametrize("N,limit_ms", [(1500, 600000), (2_000_000, 1)])
def test_time_limit_prunes_the_completed_layers(ctx, N, limit_ms):
    """The prune pass runs over the layers the call completed: with a budget it cannot exhaust, all of
    them; with one it may (1 ms against layers of 2,000,000 records each), the lists are the rule on
    the unpruned lists of the same layers (the values do not depend on when they were computed) and
    nothing above highest_completed_layer appears.  Either outcome of the second case is checked."""
    codes, arity = xor8.__wrapped__(N, 11)
    ctx.load_discrete(codes, arity)
    st0, _ = ctx.score_discrete(list(range(8)), [(1 << 8) - 1] * 8, 4, prune=False)
    plain = ctx.fetch(st0)
    ctx.set_option("time_limit_ms", limit_ms)
    st, sc = ctx.score_discrete(list(range(8)), [(1 << 8) - 1] * 8, 4, prune=True)
    got = ctx.fetch(st)
    done = ctx.info("highest_completed_layer")
    print(f"N {N}, limit {limit_ms} ms: out_of_time {ctx.info('out_of_time')}, highest completed layer {done}")
    if limit_ms == 600000:
        assert ctx.info("out_of_time") == 0
    assert (done == 4) == (ctx.info("out_of_time") == 0) and 0 <= done <= 4
    layers = _upto(plain, done)
    assert sc == 8 * sum(len(list(itertools.combinations(range(7), L))) for L in range(done + 1))
    assert _same(got, apply_rule(*layers))
    assert all(len(parents_of(int(m))) <= done for m in got[1])
    assert ctx.info("disc_pruned") == len(layers[1]) - st


def test_option_is_sticky_and_leaves_other_calls_alone(ctx):
    X = np.random.default_rng(12).normal(size=(200, 5))
    X[:, 3] += X[:, 0] - X[:, 1]
    ctx.load(X, 2.0)
    st, sc = ctx.score(list(range(5)), [31] * 5, 3)
    cbic = ctx.fetch(st)
    ctx.set_option("disc_prune", 1)
    assert ctx.score(list(range(5)), [31] * 5, 3) == (st, sc) and _same(ctx.fetch(st), cbic)

    codes, arity = n6_case()
    full = [(1 << 6) - 1] * 6
    pairs_v = [v for v in range(6) for m in range(64) if not (m >> v) & 1]
    pairs_m = [m for v in range(6) for m in range(64) if not (m >> v) & 1]
    ctx.load_discrete(codes, arity)
    ctx.set_option("disc_prune", 0)
    st0, _ = ctx.score_discrete(list(range(6)), full, 3)
    first = ctx.fetch(st0)
    values = ctx.score_sets_discrete(pairs_v, pairs_m)
    counts = [ctx.discrete_counts(2, 0b101001), ctx.discrete_counts(5, 0)]
    st1, _ = ctx.score_discrete(list(range(6)), full, 3, prune=True)
    assert st1 < st0
    # sticky: the next call without the argument prunes too
    st2, _ = ctx.score_discrete(list(range(6)), full, 3)
    assert st2 == st1 and ctx.info("disc_pruned") == st0 - st1
    assert ctx.score_sets_discrete(pairs_v, pairs_m).tobytes() == values.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(counts, [ctx.discrete_counts(2, 0b101001),
                                                              ctx.discrete_counts(5, 0)]))
    st3, _ = ctx.score_discrete(list(range(6)), full, 3, prune=False)
    assert st3 == st0 and ctx.info("disc_pruned") == 0 and _same(ctx.fetch(st3), first)


# ---- 9: search ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n6", "xor8"])
def test_search_agrees_on_pruned_and_unpruned_lists(ctx, oracle_built, name):
    o = oracle_built
    (codes, arity), k = (n6_case(), 3) if name == "n6" else (xor8(1500, 11), 4)
    n = codes.shape[1]
    full = [(1 << n) - 1] * n
    ctx.load_discrete(codes, arity)
    res, best, lists = {}, {}, {}
    for prune in (False, True):
        st, _ = ctx.score_discrete(list(range(n)), full, k, prune=prune)
        lists[prune] = ctx.fetch(st)
        ctx.search_from_scores()
        if name == "n6":
            vs = [v for v in range(6) for U in range(64) if not (U >> v) & 1]
            Us = [U for v in range(6) for U in range(64) if not (U >> v) & 1]
            assert len(vs) == 6 * 2 ** 5
            best[prune] = ctx.bestscore(vs, Us)[0]
        res[prune] = ctx.astar(mode=0)
    a, b = res[False], res[True]
    assert list(a["order"]) == list(b["order"]) and a["expanded"] == b["expanded"]
    assert np.float32(a["cost"]).tobytes() == np.float32(b["cost"]).tobytes()
    if name == "n6":
        assert best[False].tobytes() == best[True].tobytes()
    offs, sets, scores = lists[False]
    score_of = {(v, int(m)): s for v in range(n) for m, s in zip(sets[offs[v]:offs[v + 1]], scores[offs[v]:offs[v + 1]])}
    for v in range(n):
        sa, sb = score_of[(v, int(a["vpar"][v]))], score_of[(v, int(b["vpar"][v]))]
        assert sa.tobytes() == sb.tobytes(), v
    # the reference search on the pruned lists
    offs, sets, scores = lists[True]
    costs = np.array([o.quantize(float(s)) for s in scores], dtype=np.float32)
    ref = o.Search(n, offs, sets, costs).astar()
    assert ref["rc"] == 0
    assert [int(x) for x in b["vpar"]] == [int(x) for x in ref["vpar"]]
    assert list(b["order"]) == list(ref["order"]) and b["expanded"] == ref["expanded"]
    assert np.float32(b["cost"]).tobytes() == np.float32(ref["cost"]).tobytes()


# ---- 10: command line -------------------------------------------------------------
def _blocks(path):
    """.pss text -> per VAR block {parent names (tuple): the line's text}, in file order."""
    blocks, cur = [], None
    for ln in open(path).read().splitlines():
        if ln.startswith("VAR "):
            cur = {}
            blocks.append((ln[4:].strip(), cur))
        elif cur is not None and ln.strip() and not ln.startswith("META"):
            cur[tuple(ln.split()[1:])] = ln
    return blocks


def test_score_command_line_prune(ctx, tmp_path):
    full_pss, pss = tmp_path / "full.pss", tmp_path / "pruned.pss"
    r0 = subprocess.run([SCORE, HEP, str(full_pss), "-s"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and '"pruned"' not in r0.stderr and "pruning" not in r0.stdout, r0.stderr
    r = subprocess.run([SCORE, HEP, str(pss), "-s", "--prune"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    metrics = json.loads(re.search(r"ulg_metrics (\{.*\})", r.stderr).group(1))
    assert metrics["scored"] == 23200 and metrics["pruned"] == 23200 - metrics["stored"] > 0
    assert r.stdout.count("Size before pruning: 23200\n") == 1
    assert r.stdout.count(f"Size after pruning: {metrics['stored']}\n") == 1
    head = [ln for ln in open(pss).read().splitlines() if ln.startswith("META")]
    assert head == [ln for ln in open(full_pss).read().splitlines() if ln.startswith("META")]

    names, codes, arity = _hepatitis()
    ctx.load_discrete(codes, arity)
    st, _ = ctx.score_discrete(list(range(20)), [(1 << 20) - 1] * 20, 3, prune=True)
    assert st == metrics["stored"]
    want = _lists(ctx.fetch(st))
    got, plain = _blocks(pss), _blocks(full_pss)
    assert [nm for nm, _ in got] == names == [nm for nm, _ in plain]
    index = {nm: i for i, nm in enumerate(names)}
    for v in range(20):
        lines, all_lines = got[v][1], plain[v][1]
        assert [sum(1 << index[x] for x in key) for key in lines] == want[v][0], v
        assert len(all_lines) == 1160 and all(all_lines[key] == text for key, text in lines.items()), v

    found = []
    for p in (full_pss, pss):
        ra = subprocess.run([ASTAR, str(p)], capture_output=True, text=True, timeout=300)
        assert ra.returncode == 0, ra.stderr
        found.append(re.search(r"Found solution: (\S+)", ra.stdout).group(1))
    assert found[0] == found[1]
