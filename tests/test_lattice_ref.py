"""The lattice / pattern-database reference (lattice_ref.py) checked on the CPU:
its dense table against its own list scan by brute force, and the list scan,
the PDB values and h against the C oracle.  No GPU."""
import numpy as np
import pytest

import lattice_ref as lr

KINDS = ["ints", "wide", "real"]


def _small_case(kind, seed):
    """n = 8: supports of 0..7 parents (m <= 10), one empty list, one list
    without the empty set, one variable that stores only the empty set."""
    n = 8
    allm = (1 << n) - 1
    specs = [
        dict(support=allm & ~1, count=40, max_size=4),
        None,
        dict(support=0b11110011, count=25, max_size=3, empty=False),
        dict(support=0, count=0),
        dict(support=0b00000100, count=1, max_size=1),
        dict(support=0b11000011, count=12, max_size=4),
        dict(support=allm & ~(1 << 6), count=60, max_size=7),
        dict(support=0b00101010, count=6, max_size=2),
    ]
    offs, sets, costs, crafted = lr.make_lists(n, specs, seed, kind=kind)
    return n, offs, sets, costs, crafted


def test_order_key_is_the_ieee_order():
    rng = np.random.default_rng(5)
    c = lr._costs_of("wide", 4000, rng)
    c = np.concatenate([c, lr._costs_of("ints", 200, rng)])
    k = lr.order_key(c)
    i, j = rng.integers(0, len(c), 20000), rng.integers(0, len(c), 20000)
    assert np.array_equal(c[i] < c[j], k[i] < k[j])
    assert np.array_equal(c[i] == c[j], k[i] == k[j])
    assert not (k == 0xFFFFFFFF).any()
    assert lr.same_bits(lr.key_cost(k), c)
    assert lr.key_cost(np.array([0xFFFFFFFF], dtype=np.uint32))[0] == lr.FLT_MAX
    assert lr.order_key(np.float32(-0.0))[()] == lr.order_key(np.float32(0.0))[()]


@pytest.mark.parametrize("kind", KINDS)
def test_table_equals_best_by_brute_force(kind):
    n, offs, sets, costs, _ = _small_case(kind, 11)
    lat = lr.Lattice(n, offs, sets, costs)
    for scope in (None, 0b01110111, 0b00000001):
        for v in range(n):
            D, tc, tp = lat.table(v, scope)
            m = bin(D).count("1")
            assert m <= 10 and len(tc) == 1 << m
            if scope is None or (scope >> v) & 1:
                want = lat.support(v, scope)
                assert D == want
            else:
                assert D == 0
            Ss = lr.pdep(np.arange(1 << m, dtype=np.uint64), D)
            for i, S in enumerate(Ss):
                # inside the scope every stored subset of S lies inside D_v;
                # outside it (D_v empty) only the empty set is in the table
                c, p = lat.best(v, int(S))
                assert lr.same_bits(tc[i], c) and int(tp[i]) == p, (kind, scope, v, int(S))
            _, tc32, none = lat.table(v, scope, cost_only=True)
            assert none is None and lr.same_bits(tc32, tc)


@pytest.mark.parametrize("kind", KINDS)
def test_best_equals_the_oracle(kind, oracle_built):
    n, offs, sets, costs, crafted = _small_case(kind, 12)
    lat = lr.Lattice(n, offs, sets, costs)
    srch = oracle_built.Search(n, offs, sets, costs)
    vs, Ss = lr.queries(n, lat, crafted, 0, 3)
    assert len(vs) >= n << n
    mc, mp = lat.best_many(vs, Ss)
    for v, S, c, p in zip(vs, Ss, mc, mp):
        oc, op = srch.bestscore(int(v), int(S))
        assert lr.same_bits(c, np.float32(oc)) and int(p) == op, (kind, int(v), int(S))
        sc, sp = lat.best(int(v), int(S))
        assert lr.same_bits(sc, c) and sp == int(p)


def test_table_variants_agree_at_m16():
    n = 17
    specs = [dict(support=((1 << n) - 1) & ~1, count=3000, max_size=5)] + [None] * (n - 1)
    for kind in ("ints", "wide"):
        offs, sets, costs, _ = lr.make_lists(n, specs, 21, kind=kind)
        lat = lr.Lattice(n, offs, sets, costs)
        D, c64, par = lat.table(0)
        D2, c32, none = lat.table(0, cost_only=True)
        assert D == D2 == ((1 << n) - 1) & ~1 and len(c64) == 1 << 16 and none is None
        assert lr.same_bits(c64, c32)
        rng = np.random.default_rng(1)
        idx = rng.integers(0, 1 << 16, 300)
        Ss = lr.pdep(idx.astype(np.uint64), D)
        bc, bp = lat.best_many(np.zeros(len(idx), dtype=np.int64), Ss)
        assert lr.same_bits(c64[idx], bc) and np.array_equal(par[idx], bp)


PDB_CASES = [
    # (n, kind, pd_count, ancestors, scc, no_empty, hi)
    (5, "ints", 4, 0, 0b11111, None, None),             # groups 2, 2, 1, 0
    (3, "ints", 8, 0, 0b111, None, None),               # five empty groups
    (6, "ints", 1, 0, 0b111111, None, None),
    (6, "ints", 2, 0b100001, 0b011110, None, None),     # ancestors != 0
    (6, "ints", 3, 0, 0b010110, None, None),            # variables outside scc and ancestors
    (6, "real", 2, 0, 0b111111, 2, None),               # a variable without the empty set
    (6, "real", 3, 0b000011, 0b111100, 4, None),
    (6, "ints", 2, 0, sum(1 << b for b in (2, 31, 32, 40, 62, 63)), None, (2, 31, 32, 40, 62, 63)),
    (6, "ints", 3, 1 << 2, sum(1 << b for b in (31, 32, 40, 62, 63)), None, (2, 31, 32, 40, 62, 63)),
    (6, "real", 3, 0, sum(1 << b for b in (2, 31, 32, 40, 62, 63)), 1, (2, 31, 32, 40, 62, 63)),
]


@pytest.mark.parametrize("case", PDB_CASES, ids=lambda c: f"n{c[0]}-{c[1]}-pd{c[2]}-a{c[3]:x}-s{c[4]:x}")
def test_pdb_equals_the_oracle(case, oracle_built):
    n, kind, pd_count, anc, scc, no_empty, hi = case
    zero_seen = False
    for seed in (31, 32, 33):
        N, offs, sets, costs = lr.pdb_lists(n, kind, seed, no_empty, hi, N=(64 if hi else None))
        lat = lr.Lattice(N, offs, sets, costs)
        srch = oracle_built.Search(N, offs, sets, costs)
        assert srch.pdb_build(pd_count, anc, scc) == 0
        groups, pd = lat.pdb(pd_count, anc, scc)
        assert groups == srch.pdb_groups()
        for g, (grp, tab) in enumerate(zip(groups, pd)):
            Rs = lr.pdep(np.arange(len(tab), dtype=np.uint64), grp)
            want = np.array([srch.pdb_value(g, int(R)) for R in Rs], dtype=np.float32)
            assert lr.same_bits(tab, want), (seed, g)
            # the layer-at-a-time form used for large groups gives the same table
            assert lr.same_bits(lat.pdb_group_fold(grp, anc, scc), tab)
            assert lr.same_bits(lat.pdb_group_bfs(grp, anc, scc), tab)
        allm = (1 << N) - 1
        bits = lr.bits_of(scc | anc)
        for r in range(1 << len(bits)):
            S = sum(1 << bits[i] for i in range(len(bits)) if (r >> i) & 1)
            for S2 in (S, S | (allm & ~(scc | anc))):
                hv, comp = lat.h(S2)
                oh, oc = srch.pdb_h(S2)
                assert lr.same_bits(hv, np.float32(oh)) and comp == oc, (seed, S2)
        Ss = [S for r in range(1 << len(bits)) for S in [sum(1 << bits[i] for i in range(len(bits)) if (r >> i) & 1)]]
        hm, cm = lat.h_many(Ss)
        for S, hv, cv in zip(Ss, hm, cm):
            sh, sc = lat.h(S)
            assert lr.same_bits(hv, sh) and cv == sc
        zero_seen |= lat.zero_sum_share() > 0
    if kind == "ints":
        assert zero_seen, "the ints cases must reach partial sums that are exactly 0"


def test_keep_rule_depends_on_the_visiting_order():
    """The case that pins the order: with a zero partial sum the value kept is
    the one that comes last among {zero, then anything}, not the minimum."""
    n = 2
    offs = np.array([0, 2, 4], dtype=np.int64)
    sets = np.array([0, 2, 0, 1], dtype=np.uint64)
    # variable 0: {} 1, {1} -1;  variable 1: {} 1, {0} 0
    costs = np.array([1, -1, 1, 0], dtype=np.float32)
    lat = lr.Lattice(n, offs, sets, costs)
    _, (pd,) = lat.pdb(1)
    bfs = lat.pdb_group_bfs(0b11, 0, 0b11)
    fold = lat.pdb_group_fold(0b11, 0, 0b11)
    assert lr.same_bits(bfs, fold) and lr.same_bits(pd, bfs)
    # pd[{0}] = best(0, {0,1}) = -1; pd[{1}] = best(1, {0,1}) = 0
    assert pd[1] == -1 and pd[2] == 0
    # pd[{0,1}]: key {0} (r = 1) first: best(1, {1}) + pd[{0}] = 1 + -1 = 0;
    # then key {1} (r = 2): best(0, {0}) + pd[{1}] = 1 + 0 = 1, kept because oldG == 0
    assert pd[3] == 1


def test_make_lists_crafted_sets():
    n = 17
    D = ((1 << n) - 1) & ~(1 << 3)
    offs, sets, costs, crafted = lr.make_lists(n, [None] * 3 + [dict(support=D, count=50, max_size=3)], 9, kind="wide")
    s = set(int(x) for x in sets)
    assert len(s) == len(sets)  # distinct
    assert offs[3] == 0 and offs[4] == len(sets) and offs[-1] == len(sets)
    idx = set(int(x) for x in lr.pext(sets, D))
    for want in (0, (1 << 16) - 1, 1, 1 << 15, 16383, (2 << 14) + 16383, 2 << 14, 3 << 14, (3 << 14) + 16383):
        assert want in idx
    assert sum(1 for i in idx if i >> 14 == 2) >= 1500
    assert not np.isnan(costs).any()
    assert set(crafted[3]) <= s
