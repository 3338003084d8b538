"""The scorer's unrank tables (option score_unrank_lut).

The layer launches of 4 to 8 parents read each set's members from a table
rank -> set per (U candidates, l members) instead of computing unrank_colex in
every lane; waves whose 64 sets belong to one variable find that variable on
the scalar unit, waves that straddle a boundary search per lane.  None of it
touches the arithmetic of a score, so on every shape below a call with the
tables off (option 0) and a call with them on must give the same offsets, the
same sets and the same score BITS, with the error word 0.  What each shape can
break:

  n=9  k=6 full      layer 6 has 252 sets in one block: every wave straddles
                     variable boundaries (per-lane lookup, mixed offsets)
  n=12 k=6 full      5,544 layer-6 sets: waves inside one variable and waves
                     that straddle (scalar and per-lane lookup)
  n=12 k=6 edges     variables with and without variable 0 among their
                     candidates, m differing: all three (U, l) forms and
                     several tables in one launch
  ... constrained    the constrained twin kernels
  cap 1000 / 300     n=12: C(11, 6) = C(11, 5) = 462 and C(11, 4) = 330 entries
                     for variable 0, at most C(10, 5) = 252 for the others.
                     A cap of 1,000 keeps every table; a cap of 300 leaves
                     variable 0 to the computed path while the other
                     variables read tables, in the same launches.
  n=35 k=5, 3 vars   U = 34 and 33 > 32: no table may exist
  async rounds       tables built by the first call, replayed from the
                     captured graph afterwards, then the option changes
"""
import math

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

LAMBDA = 2.0


def _full(n):
    return list(range(n)), [(1 << n) - 1] * n


def _edges12():
    """n = 12: an edge-list skeleton whose neighbourhoods have 6 to 11 members;
    variables 3, 7 and 10 do not have variable 0 as a candidate."""
    n = 12
    rng = np.random.default_rng(1207)
    adj = np.zeros((n, n), dtype=bool)
    for i in range(n):
        for j in range(i + 1, n):
            adj[i, j] = adj[j, i] = rng.random() < 0.8
    for v in range(1, n):
        adj[0, v] = adj[v, 0] = v not in (3, 7, 10)
    cands = [int(sum(1 << j for j in range(n) if adj[i, j])) for i in range(n)]
    sizes = [bin(c).count("1") for c in cands]
    assert min(sizes) >= 6 and len(set(sizes)) >= 3, sizes  # layer 6 everywhere, several m
    assert [v for v in range(1, n) if not cands[v] & 1] == [3, 7, 10]
    return list(range(n)), cands


CONS12 = [(1, 0b100, 0), (1, 0, 0b1000000), (4, 0b1, 0b10), (9, 0, 0b111)]


def _run(ctx, variables, cands, k):
    st, _ = ctx.score(variables, cands, k)
    assert ctx.info("score_error_word") == 0
    offs, sets, scores = ctx.fetch(st)
    return offs.copy(), sets.copy(), scores.copy()


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "offsets")
    assert np.array_equal(a[1], b[1]), (what, "sets")
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), (what, "score bits")


def _expected_entries(variables, cands, k, cap):
    """the distinct (U, l) tables of the call: the rule restated"""
    pairs = set()
    for v, c in zip(variables, cands):
        c &= ~(1 << v)
        m, z = bin(c).count("1"), bool(c & 1)
        for L in range(4, min(k, m, 8) + 1):
            forms = [(m - 1, L - 1), (m - 1, L)] if z else [(m, L)]
            for U, l in forms:
                if U <= 32 and 0 < math.comb(U, l) <= cap:
                    pairs.add((U, l))
    return sum(math.comb(U, l) for U, l in pairs)


SHAPES = {
    "n9_full": (9, 300, 6, _full(9), None, None, True),
    "n12_full": (12, 300, 6, _full(12), None, None, True),
    "n12_edges": (12, 400, 6, _edges12(), None, None, False),
    "n12_edges_cons": (12, 400, 6, _edges12(), CONS12, None, False),
    "n12_cap1000": (12, 300, 6, _full(12), None, 1000, False),
    "n12_cap300": (12, 300, 6, _full(12), None, 300, False),
    "n35_k5_three": (35, 200, 5, ([0, 17, 34], [(1 << 35) - 1] * 3), None, None, False),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_tables_change_nothing(oracle_built, name):
    import ulg
    n, N, k, (variables, cands), cons, cap, with_oracle = SHAPES[name]
    X, _ = synth.gaussian_sem(n, N, 9200 + n)
    ctx = ulg.Context(0)
    try:
        default = ctx.info("score_unrank_lut")
        assert default > 0
        ctx.load(X, LAMBDA)
        if cons:
            ctx.set_constraints(cons)
        ctx.set_option("score_unrank_lut", 0)
        off = _run(ctx, variables, cands, k)
        assert ctx.info("unrank_lut_entries") == 0
        cap = default if cap is None else cap
        ctx.set_option("score_unrank_lut", cap)
        on = _run(ctx, variables, cands, k)
        _same(off, on, name)
        assert ctx.info("unrank_lut_entries") == _expected_entries(variables, cands, k, cap)
        if name == "n35_k5_three":
            assert ctx.info("unrank_lut_entries") == 0
        else:
            assert ctx.info("unrank_lut_entries") > 0
        if name == "n12_cap300":  # variable 0 computes, the others read tables
            assert _expected_entries(variables[:1], cands[:1], k, cap) == 0
            assert _expected_entries(variables[1:], cands[1:], k, cap) > 0
            # ... within one launch: the plan's own offsets (host/unrank_lut_check.cpp
            # prints them) leave variable 0 without a table in every phase-1
            # launch of layers 4 to 6 and give every other variable one
            from test_unrank_lut_host import run_plan
            (_, offs), = run_plan([(cap, k, n, list(zip(variables, cands)))])
            for L in (4, 5, 6):
                assert (L, 1, 0) not in offs, L
                assert all((L, 1, i) in offs for i in range(1, n)), L
        if with_oracle:
            ds = oracle_built.Dataset(X)
            for i, (v, c) in enumerate(zip(variables, cands)):
                ref = ds.score_variable(LAMBDA, v, c, k)[0]
                assert np.array_equal(on[1][on[0][i]:on[0][i + 1]], ref), (name, v)
    finally:
        ctx.close()


def test_async_rounds_and_option_change():
    import ulg
    n, N, k = 12, 300, 6
    variables, cands = _full(n)
    X, _ = synth.gaussian_sem(n, N, 9212)
    ctx = ulg.Context(0)
    try:
        ctx.load(X, LAMBDA)
        default = ctx.info("score_unrank_lut")
        ctx.set_option("score_unrank_lut", 0)
        ref = _run(ctx, variables, cands, k)
        ctx.set_option("score_unrank_lut", default)
        entries = None
        for caps in ([default] * 3, [300], [0], [default]):
            for cap in caps:
                ctx.set_option("score_unrank_lut", cap)
                ctx.score_async(variables, cands, k)
                st, _ = ctx.score_finish()
                assert ctx.info("score_error_word") == 0, cap
                offs, sets, scores = ctx.fetch(st)
                _same(ref, (offs, sets, scores), ("async", cap))
                if entries is None:  # the first round built every table; nothing is added later
                    entries = ctx.info("unrank_lut_entries")
                    assert entries == _expected_entries(variables, cands, k, default)
                assert ctx.info("unrank_lut_entries") == entries
    finally:
        ctx.close()
