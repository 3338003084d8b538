"""BGe on the GPU (ulg_bge_set_prior, ulg_bge_score, ulg_bge_score_sets, option
"bge_prune", `score --bge`) against bge_ref.py.

Tolerance: every value is within 1 float32 ulp of float32(reference).  A GPU
value is the FP64 result of the kernel's operation order rounded to float once;
test_bge.py bounds that FP64 result within 1e-3 float32 ulps of the long-double
reference on every input used here, so the rounded value is float32(reference)
or its neighbour.  The bound is not a measured number.  Sets, counts, list
order and the equalities between the two entry points are exact."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ulg
from bge_ref import case, list_order, members, ref
from conftest import PKG
from test_disc_prune import apply_rule

pytestmark = pytest.mark.gpu

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


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _within_one_ulp(got, want, what=""):
    """got: float32 from the GPU; want: long double reference (finite)."""
    w32 = want.astype(np.float32)
    ulps = np.abs(got.astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)
    worst = float(ulps.max()) if len(ulps) else 0.0
    print(f"{what}: {len(got)} values, at most {worst:g} float32 ulps from float32(reference), "
          f"{int((got != w32).sum())} not equal to it, {int((got > 0).sum())} positive")
    assert np.all(np.isfinite(got)) and worst <= 1.0, what


def _pairs(variables, cands, k):
    vs, ms, offs = [], [], [0]
    for v, c in zip(variables, cands):
        order = list_order([p for p in members(c) if p != v], k)
        vs += [v] * len(order)
        ms += order
        offs.append(len(vs))
    return vs, ms, offs


def _expected_lists(ctx, variables, cands, k, constraints=()):
    """The store rule (every finite value of a non-violating set) on ulg_bge_score_sets' values, in the
    scorer's order -> (offsets, sets, scores), and the number of pairs."""
    vs, ms, _ = _pairs(variables, cands, k)
    vals = ctx.score_sets_bge(vs, ms)
    offs, sets, scores = [0], [], []
    pos = 0
    for v, c in zip(variables, cands):
        alts = [(r, f) for cv, r, f in constraints if cv == v]
        while pos < len(vs) and vs[pos] == v:
            m, s = ms[pos], vals[pos]
            pos += 1
            if alts and not any((r & ~m) == 0 and (m & f) == 0 for r, f in alts):
                assert np.isnan(s), (v, m)
                continue
            if np.isfinite(s):
                sets.append(m)
                scores.append(s)
        offs.append(len(sets))
    return (np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32)), len(vs)


def _check_call(ctx, name, variables, cands, k, every=1, am=1.0, aw=None):
    """One ulg_bge_score call against ulg_bge_score_sets (bit for bit), itself (a second call), the list
    order, the counts and the reference (every `every`-th stored set)."""
    r = ref(name, am, aw)
    want, npairs = _expected_lists(ctx, variables, cands, k)
    st, sc = ctx.score_bge(variables, cands, k)
    got = ctx.fetch(st)
    assert sc == npairs == sum(sum(math.comb(len([p for p in members(c) if p != v]), l) for l in range(k + 1))
                               for v, c in zip(variables, cands))
    assert st == len(want[1])
    assert [int(x) for x in got[0]] == [int(x) for x in want[0]]
    assert _same(got[1:], want[1:]), "the lists differ from ulg_bge_score_sets"
    for i in range(len(variables)):
        lst = [int(m) for m in got[1][got[0][i]:got[0][i + 1]]]
        assert lst == sorted(lst, key=lambda m: (bin(m).count("1"), m)), "not in (|set|, value) order"
    st2, sc2 = ctx.score_bge(variables, cands, k)
    assert (st2, sc2) == (st, sc) and _same(ctx.fetch(st2), got), "two calls differ"
    vs = np.repeat(np.asarray(variables), np.diff(got[0]))[::every]
    sel = slice(None, None, every)
    _within_one_ulp(got[2][sel], r.scores(vs.tolist(), [int(m) for m in got[1][sel]]), name)
    return got, st, sc


# ---- shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n10_N8", "n10_N50", "n10_N1000"])
def test_every_layer_up_to_nine(ctx, name):
    """n = 10, full candidates, 9 parents: the unrolled instances 1 .. 8 and the generic one at 0 and 9.
    N = 8 has fewer records than parents: G is singular, R = G + t I is not."""
    X = case(name)
    ctx.load(X, 2.0)
    got, st, sc = _check_call(ctx, name, list(range(10)), [(1 << 10) - 1] * 10, 9)
    assert sc == 10 * 2 ** 9 and st == sc  # every value is finite, so every set is stored, the empty ones too
    assert ctx.info("highest_completed_layer") == 9 and ctx.info("out_of_time") == 0 and ctx.info("bge_pruned") == 0
    assert all(int(got[1][got[0][i]]) == 0 for i in range(10))


def test_thirty_one_parents(ctx):
    """n = 32, one variable with its 31 candidates and max_parents = 31: 2^31 slots.  26 required parents
    leave 2^5 sets to evaluate, of 26 .. 31 parents; every other slot is a violator and stays empty.
    The table, the masks and the output buffers of 2^31 slots take 48 GB of device memory until the
    context closes; the call takes about half a second."""
    r = ref("n32")
    ctx.load(case("n32"), 2.0)
    v = 7
    full = (1 << 32) - 1
    others = [p for p in range(32) if p != v]
    req = sum(1 << p for p in others[:26])
    free = others[26:]
    masks = sorted((req | sum(1 << p for p in c) for l in range(6) for c in itertools.combinations(free, l)),
                   key=lambda m: (bin(m).count("1"), m))
    direct = ctx.score_sets_bge([v] * 32, masks)  # before the constraints: plain values
    _within_one_ulp(direct, r.scores([v] * 32, masks), "n32 score_sets")
    assert bin(masks[-1]).count("1") == 31
    ctx.set_constraints([(v, req, 0)])
    st, sc = ctx.score_bge([v], [full], 31)
    offs, sets, scores = ctx.fetch(st)
    assert sc == 2 ** 31 and st == 32 and [int(x) for x in offs] == [0, 32]
    assert [int(m) for m in sets] == masks and scores.tobytes() == direct.tobytes()
    assert ctx.score_sets_bge([v] * 32, masks).tobytes() == direct.tobytes()
    assert np.isnan(ctx.score_sets_bge([v], [req & ~(1 << others[0])])[0])


def test_variables_and_candidates_above_bit_31(ctx):
    r = ref("n63")
    ctx.load(case("n63"), 2.0)
    variables = [62, 35]
    cands = [sum(1 << b for b in range(33, 45)), sum(1 << b for b in range(50, 62))]
    got, st, sc = _check_call(ctx, "n63", variables, cands, 6)
    assert sc == sum(math.comb(12, l) for l in range(7)) * 2 and st == sc
    assert all(int(m) >> 32 for m in got[1] if int(m))


def test_three_variables_of_three_seven_and_twelve_candidates(ctx):
    """One call whose variables end at different layers: 3, 7 and 12 (the generic instance from 9)."""
    ctx.load(case("mixed"), 2.0)
    variables = [2, 9, 13]
    cands = [0b00000000011010, 0b01110100110001, 0b00111111111111]
    assert [bin(c & ~(1 << v)).count("1") for v, c in zip(variables, cands)] == [3, 7, 12]
    got, st, sc = _check_call(ctx, "mixed", variables, cands, 13)
    assert sc == 2 ** 3 + 2 ** 7 + 2 ** 12 and st == sc
    assert [int(x) for x in got[0]] == [0, 8, 136, 4232]


def test_a_layer_larger_than_one_pass_of_the_grid(ctx):
    """n = 20, 6 parents: layer 6 has 542,640 sets against 2048 x 256 lanes.  All 875,920 values equal
    ulg_bge_score_sets'; every 9th is held to the reference."""
    ctx.load(case("n20"), 2.0)
    got, st, sc = _check_call(ctx, "n20", list(range(20)), [(1 << 20) - 1] * 20, 6, every=9)
    assert sc == 875920 and st == sc and 20 * math.comb(19, 6) == 542640 > 2048 * 256


def test_duplicate_affine_and_collinear_columns(ctx):
    """Column 3 = column 1, column 5 = 3 - 2.5 column 2, column 6 = column 0 + column 4 + 1e-9 noise, at the
    default prior: the positive scores are stored."""
    ctx.load(case("illcond"), 2.0)
    got, st, sc = _check_call(ctx, "illcond", list(range(8)), [(1 << 8) - 1] * 8, 7)
    assert sc == 8 * 2 ** 7 and st == sc
    assert (got[2] > 0).sum() > 100
    dup = ctx.score_sets_bge([3, 1, 5, 6], [0b10, 0b1000, 0b100, 0b10001])
    assert np.all(dup > 0)


def test_constant_column(ctx):
    """NaN iff the set touches the constant column, and nothing NaN is stored."""
    ctx.load(case("const"), 2.0)
    vs, ms, _ = _pairs(list(range(6)), [0b111111] * 6, 5)
    vals = ctx.score_sets_bge(vs, ms)
    touched = np.array([v == 2 or bool(m >> 2 & 1) for v, m in zip(vs, ms)])
    assert np.array_equal(np.isnan(vals), touched)
    _within_one_ulp(vals[~touched], ref("const").scores(vs, ms)[~touched], "const")
    st, sc = ctx.score_bge(list(range(6)), [0b111111] * 6, 5)
    offs, sets, scores = ctx.fetch(st)
    assert sc == 6 * 32 and st == int((~touched).sum()) == 5 * 16
    assert np.all(np.isfinite(scores)) and not any(int(m) >> 2 & 1 for m in sets)
    assert offs[3] == offs[2]  # the constant column's own list is empty
    assert scores.tobytes() == vals[~touched].tobytes()


def test_positive_scores_are_in_the_list(ctx):
    """Variable 5 = x0 + x1 + x2 + 1e-3 noise: its sets that hold all three parents score above zero."""
    ctx.load(case("sum"), 2.0)
    got, st, sc = _check_call(ctx, "sum", list(range(6)), [0b111111] * 6, 5)
    offs, sets, scores = got
    mine = {int(m): float(s) for m, s in zip(sets[offs[5]:offs[6]], scores[offs[5]:offs[6]])}
    assert len(mine) == 32
    assert all((s > 0) == ((m & 0b111) == 0b111) for m, s in mine.items())
    assert mine[0b111] > 100 and mine[0] < 0


# ---- constraints, prune, prior ----------------------------------------------------------------
def test_constraints(ctx):
    ctx.load(case("prior"), 2.0)
    full = [(1 << 8) - 1] * 8
    cons = [(0, 0b00000010, 0b00000100), (0, 0b00001000, 0),  # variable 0: (1 and not 2) or 3
            (3, 0, 0b00010001),                               # variable 3: neither 0 nor 4
            (4, 0b00000001, 0)]                               # variable 4: needs parent 0
    st0, sc0 = ctx.score_bge(list(range(8)), full, 4)
    plain = ctx.fetch(st0)
    ctx.set_constraints(cons)
    want, npairs = _expected_lists(ctx, list(range(8)), full, 4, constraints=cons)
    st, sc = ctx.score_bge(list(range(8)), full, 4)
    got = ctx.fetch(st)
    assert sc == sc0 == npairs and st == len(want[1]) < st0
    assert [int(x) for x in got[0]] == [int(x) for x in want[0]] and _same(got[1:], want[1:])
    assert 0 not in [int(m) for m in got[1][got[0][4]:got[0][5]]]  # the empty set violates "needs parent 0"
    assert all(int(m) & 1 for m in got[1][got[0][4]:got[0][5]])
    assert not any(int(m) & 0b10001 for m in got[1][got[0][3]:got[0][4]])
    # the kept values are the unconstrained ones
    lookup = {(v, int(m)): s for v in range(8) for m, s in zip(plain[1][plain[0][v]:plain[0][v + 1]],
                                                                 plain[2][plain[0][v]:plain[0][v + 1]])}
    for v in range(8):
        for m, s in zip(got[1][got[0][v]:got[0][v + 1]], got[2][got[0][v]:got[0][v + 1]]):
            assert lookup[(v, int(m))].tobytes() == s.tobytes()
    ctx.clear_constraints()
    st2, _ = ctx.score_bge(list(range(8)), full, 4)
    assert st2 == st0 and _same(ctx.fetch(st2), plain)


@pytest.mark.parametrize("name", ["prior", "sum"])
def test_prune(ctx, name):
    """bge_prune on = test_disc_prune.prune_rule on the unpruned lists, bit for bit; bge_pruned = the rest."""
    X = case(name)
    n = X.shape[1]
    full = [(1 << n) - 1] * n
    ctx.load(X, 2.0)
    st0, sc0 = ctx.score_bge(list(range(n)), full, 4, prune=False)
    plain = ctx.fetch(st0)
    assert ctx.info("bge_pruned") == 0 and ctx.info("bge_prune") == 0
    st1, sc1 = ctx.score_bge(list(range(n)), full, 4, prune=True)
    pruned = ctx.fetch(st1)
    assert sc1 == sc0 and ctx.info("bge_pruned") == st0 - st1 and 0 < st1 < st0
    assert _same(pruned, apply_rule(*plain))
    assert ctx.info("disc_pruned") == 0 and ctx.info("disc_prune") == 0
    for bad in (2, -1):
        with pytest.raises(ulg.ULGError) as e:
            ctx.set_option("bge_prune", bad)
        assert _status(e) == STATUS["ARG"]
    # sticky, and back
    assert ctx.score_bge(list(range(n)), full, 4) == (st1, sc1)
    assert ctx.score_bge(list(range(n)), full, 4, prune=False) == (st0, sc0) and _same(ctx.fetch(st0), plain)
    assert ctx.info("bge_pruned") == 0


def test_non_default_prior(ctx):
    """alpha_mu = 0.1, alpha_w = n + 5 on well-conditioned data, sticky, and back to the default."""
    X = case("prior")
    ctx.load(X, 2.0)
    full = [(1 << 8) - 1] * 8
    st0, _ = ctx.score_bge(list(range(8)), full, 7)
    default = ctx.fetch(st0)
    ctx.set_bge_prior(0.1, 8 + 5)
    got, st, sc = _check_call(ctx, "prior", list(range(8)), full, 7, am=0.1, aw=13.0)
    assert st == st0 and not np.array_equal(got[2], default[2])
    # the prior survives a load; the keyword form sets it too
    ctx.load(X, 0.5)
    assert _same(ctx.fetch(ctx.score_bge(list(range(8)), full, 7)[0]), got)
    st1, _ = ctx.score_bge(list(range(8)), full, 7, alpha_mu=1.0, alpha_w=0.0)
    assert _same(ctx.fetch(st1), default)
    vs, ms, _ = _pairs([0, 5], full[:2], 3)
    a = ctx.score_sets_bge(vs, ms, alpha_mu=0.1, alpha_w=13.0)
    _within_one_ulp(a, ref("prior", 0.1, 13.0).scores(vs, ms), "prior score_sets")
    # lambda does not enter
    ctx.load(X, 7.0)
    assert ctx.score_sets_bge(vs, ms).tobytes() == a.tobytes()


def test_errors(ctx):
    X = case("prior")
    full = [(1 << 8) - 1] * 8
    # no data at all
    for call in (lambda: ctx.score_bge([0], [0b10], 1), lambda: ctx.score_sets_bge([0], [0b10])):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS["STATE"]
    ctx.load(X, 2.0)
    st, sc = ctx.score_bge(list(range(8)), full, 3)
    before = ctx.fetch(st)
    for am, aw in ((0.0, 0.0), (-1.0, 0.0), (9e-4, 0.0), (1001.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0),
                   (1.0, 9.0), (1.0, 8.5), (1.0, -1.0), (1.0, 8 + 1e6 + 1), (1.0, float("nan")), (1.0, float("inf"))):
        with pytest.raises(ulg.ULGError) as e:
            ctx.set_bge_prior(am, aw)
        assert _status(e) == STATUS["ARG"], (am, aw)
    # the refused priors left the default: same lists
    assert ctx.score_bge(list(range(8)), full, 3) == (st, sc) and _same(ctx.fetch(st), before)
    ctx.set_bge_prior(1.0, 9.5)  # fine for n = 8 ...
    wide = np.random.default_rng(4).normal(size=(60, 12))
    ctx.load(wide, 2.0)          # ... and not for n = 12: checked again at scoring time
    for call in (lambda: ctx.score_bge([0], [0b10], 1), lambda: ctx.score_sets_bge([0], [0b10])):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS["ARG"]
    ctx.set_bge_prior(1.0, 0.0)
    ctx.load(X, 2.0)
    st, sc = ctx.score_bge(list(range(8)), full, 3)
    # refused calls leave the previous lists
    for call, status in ((lambda: ctx.score_bge([0, 9], full[:2], 3), "ARG"), (lambda: ctx.score_bge([1, 1], full[:2], 3), "ARG"),
                         (lambda: ctx.score_bge([], [], 3), "ARG"), (lambda: ctx.score_sets_bge([0], [1 << 9]), "ARG"),
                         (lambda: ctx.score_sets_bge([8], [1]), "ARG")):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS[status] and _same(ctx.fetch(st), before)
    # more than 31 parents
    big = np.random.default_rng(5).normal(size=(50, 40))
    ctx.load(big, 2.0)
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_bge([0], [(1 << 40) - 1], 39)
    assert _status(e) == STATUS["UNSUPPORTED"]
    with pytest.raises(ulg.ULGError) as e:
        ctx.score_sets_bge([0], [(1 << 34) - 2])
    assert _status(e) == STATUS["UNSUPPORTED"]
    assert np.isfinite(ctx.score_sets_bge([0], [(1 << 32) - 2])[0])
    # discrete data
    codes = (np.arange(120).reshape(30, 4) % 3).astype(np.uint8)
    ctx.load_discrete(codes, [3, 3, 3, 3])
    for call in (lambda: ctx.score_bge([0], [0b1110], 1), lambda: ctx.score_sets_bge([0], [0b10])):
        with pytest.raises(ulg.ULGError) as e:
            call()
        assert _status(e) == STATUS["STATE"]


def test_time_limit_keeps_complete_layers(ctx):
    """A budget that never runs out changes nothing; the layer bookkeeping is ulg_disc_score's."""
    ctx.load(case("prior"), 2.0)
    full = [(1 << 8) - 1] * 8
    st, sc = ctx.score_bge(list(range(8)), full, 5)
    first = ctx.fetch(st)
    ctx.set_option("time_limit_ms", 10 ** 9)
    assert ctx.score_bge(list(range(8)), full, 5) == (st, sc) and _same(ctx.fetch(st), first)
    assert ctx.info("out_of_time") == 0 and ctx.info("highest_completed_layer") == 5
    ctx.set_option("time_limit_ms", 0)


def test_cbic_and_bge_share_a_context(ctx):
    """The two continuous scorers alternate on one load: neither disturbs the other's lists."""
    ctx.load(case("prior"), 2.0)
    full = [(1 << 8) - 1] * 8
    c0 = ctx.score(list(range(8)), full, 3)
    cbic = ctx.fetch(c0[0])
    b0 = ctx.score_bge(list(range(8)), full, 3)
    bge = ctx.fetch(b0[0])
    assert b0[0] == 8 * (1 + 7 + 21 + 35) and b0[0] > c0[0]
    assert ctx.score(list(range(8)), full, 3) == c0 and _same(ctx.fetch(c0[0]), cbic)
    assert ctx.score_bge(list(range(8)), full, 3) == b0 and _same(ctx.fetch(b0[0]), bge)


# ---- end to end ---------------------------------------------------------------------------------
def _brute_force(offs, sets, costs, n):
    """The smallest float32 path sum over all n! orders: g <- float32(g + best cost of v within its predecessors)."""
    lists = [[(int(m), np.float32(c)) for m, c in zip(sets[offs[v]:offs[v + 1]], costs[offs[v]:offs[v + 1]])] for v in range(n)]
    best = {}
    for v in range(n):
        for U in range(1 << n):
            if not U >> v & 1:
                fits = [c for m, c in lists[v] if m & ~U == 0]
                best[(v, U)] = min(fits) if fits else None
    out = None
    for o in itertools.permutations(range(n)):
        g, U = np.float32(0.0), 0
        for v in o:
            g = np.float32(g + best[(v, U)])
            U |= 1 << v
        out = g if out is None or g < out else out
    return out


def test_end_to_end_with_negative_costs(ctx, tmp_path):
    """n = 6 with positive scores, hence negative costs: the lists through the "%f" round trip, the tables,
    A* in both modes against brute force over all 720 orders, and `score --bge`'s .pss against the lists."""
    X = case("e2e")
    n = 6
    full = [(1 << n) - 1] * n
    ctx.load(X, 2.0)
    got, st, sc = _check_call(ctx, "e2e", list(range(n)), full, 5)
    offs, sets, scores = got
    assert (scores > 0).sum() >= 10
    costs = ctx.quantize(scores)
    assert (costs < 0).sum() == (scores > 0).sum()
    assert all(np.float32(-float("%f" % float(s))) == c for s, c in zip(scores, costs))
    ctx.score_bge(list(range(n)), full, 5)
    ctx.search_from_scores()
    want = _brute_force(offs, sets, costs, n)
    for mode in (0, 1):
        res = ctx.astar(mode=mode)
        print(f"mode {mode}: cost {res['cost']!r}, brute force {float(want)!r}, expanded {res['expanded']}")
        assert np.float32(res["cost"]).tobytes() == np.float32(want).tobytes(), mode
        # the DAG it returns costs that much
        look = [{int(m): float(c) for m, c in zip(sets[offs[v]:offs[v + 1]], costs[offs[v]:offs[v + 1]])} for v in range(n)]
        total = math.fsum(look[v][int(res["vpar"][v])] for v in range(n))
        assert abs(total - float(want)) <= 1e-5 * abs(total)
        assert min(look[v][int(res["vpar"][v])] for v in range(n)) < 0  # ... through families of negative cost
    # the best-score lookups with negative costs
    q = ctx.bestscore([4, 5, 4], [0b000011, 0b001000, 0])
    lo4 = min(float(c) for m, c in zip(sets[offs[4]:offs[5]], costs[offs[4]:offs[5]]) if int(m) & ~0b11 == 0)
    assert float(q[0][0]) == lo4 < 0 and float(q[0][1]) < 0 < float(q[0][2])
    # the command line
    csv = tmp_path / "e2e.csv"
    np.savetxt(csv, X, delimiter=",", fmt="%.17g")
    pss = tmp_path / "e2e.pss"
    r = subprocess.run([SCORE, str(csv), str(pss), "--bge", "-p", "5", "--lambda", "3"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"function": "bge"' in r.stderr
    text = open(pss).read().splitlines()
    meta = {}
    for ln in text:
        if ln.startswith("VAR "):
            break
        if ln.startswith("META "):
            k, _, val = ln[5:].partition("=")
            meta[k.strip()] = val.strip()
    assert meta["score_type"] == "bge" and meta["parent_limit"] == "5" and meta["num_records"] == "250"
    names = [ln[4:].strip() for ln in text if ln.startswith("VAR ")]
    assert len(names) == n
    index = {nm: i for i, nm in enumerate(names)}
    v = -1
    seen = [[] for _ in range(n)]
    for ln in text:
        if ln.startswith("VAR "):
            v += 1
        elif v >= 0 and ln.strip() and not ln.startswith("META"):
            tok = ln.split()
            seen[v].append((tok[0], sum(1 << index[x] for x in tok[1:])))
    assert sum(len(b) for b in seen) == st
    for v in range(n):
        assert [m for _, m in seen[v]] == [int(x) for x in sets[offs[v]:offs[v + 1]]], v
        assert [t for t, _ in seen[v]] == ["%f" % float(s) for s in scores[offs[v]:offs[v + 1]]], v
    assert any(not t.startswith("-") for b in seen for t, _ in b)
    net = tmp_path / "net"
    r = subprocess.run([ASTAR, str(pss), "-n", str(net)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # with a non-default prior and --prune
    r = subprocess.run([SCORE, str(csv), str(tmp_path / "p.pss"), "--bge", "-p", "3", "--alpha-mu", "0.1", "--alpha-w", "11",
                        "--prune"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    st3, _ = ctx.score_bge(list(range(n)), full, 3, prune=True, alpha_mu=0.1, alpha_w=11.0)
    assert f'"stored": {st3},' in r.stderr and f'"pruned": {ctx.info("bge_pruned")}' in r.stderr
    assert f"Size after pruning: {st3}" in r.stdout
    with pytest.raises(Exception):
        subprocess.run([SCORE, str(csv), str(tmp_path / "q.pss"), "--bge", "--alpha-w", "6.5"], check=True,
                       capture_output=True, timeout=300)  # 6.5 <= n + 1: the library refuses it
