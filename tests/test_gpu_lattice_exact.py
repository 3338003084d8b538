"""Every entry of the device-built best-score tables and pattern databases
against the plain reference (lattice_ref.py), bit for bit, at the shapes where
search.hip changes path.  Inputs are synthetic lists from lattice_ref.make_lists
loaded with ulg_search_load: no scoring and no oracle on this path.  Tables are
read back with ulg_bestscore_table / ulg_pdb_table; values are compared as bit
patterns after folding -0.0 onto +0.0 (the contract in lattice_ref's
docstring); there is no tolerance anywhere in this file.

Which case reaches which kernel form is listed in DESIGN.md (section 4.2)."""
import functools

import numpy as np
import pytest

import torch  # at collection, before any test loads libulg.so: imported after it, torch reports no HIP GPU

import lattice_ref as lr
import pct_f_values
import ulg

pytestmark = pytest.mark.gpu

KINDS = ["ints", "wide"]
NQ = 20000


def _support(n, v, m, rng):
    others = [b for b in range(n) if b != v]
    return sum(1 << int(b) for b in rng.choice(others, m, replace=False))


def _specs(n, ms, seed, count=300, max_size=4):
    """One spec per variable with |D_v| = ms[v] (drawn from the other
    variables); m = 0 stores the empty set only."""
    rng = np.random.default_rng(seed)
    out = []
    for v in range(n):
        m = ms[v]
        out.append(dict(support=_support(n, v, m, rng), count=min(count, 1 << m) if m else 0, max_size=max_size))
    return out


@functools.lru_cache(maxsize=4)
def _case(name, kind):
    """(n, offsets, sets, costs, crafted) of a named case."""
    if name == "L1a1":
        n, specs = 1, [dict(support=0, count=0)]
    elif name == "L1a2":
        n, specs = 2, [dict(support=2, count=1, max_size=1), dict(support=1, count=1, max_size=1)]
    elif name == "L1b":
        # an empty list, a list without the empty set (m = 4), a variable that
        # stores only the empty set (m = 0), m = 1 and m = 2
        n = 5
        specs = [None, dict(support=0b11101, count=10, max_size=4, empty=False), dict(support=0, count=0),
                 dict(support=0b00001, count=1, max_size=1), dict(support=0b00011, count=3, max_size=2)]
    elif name == "L2":
        n = 17
        specs = _specs(n, [13, 14, 15, 16, 3, 0, 14, 9, 5, 1, 12, 7, 2, 10, 4, 8, 6], 102)
    elif name == "L3":
        n = 25
        specs = _specs(n, [24, 19, 6] + [(3 * i) % 11 for i in range(22)], 103, count=2500)
    elif name == "L4a":
        n = 25
        specs = _specs(n, [14] * 7 + [24] + [14] * 9 + [24] + [14] * 7, 104, count=2500)
    elif name == "L4b":
        n = 25
        specs = _specs(n, [14] * 3 + [15] + [14] * 12 + [24] + [14] * 8, 105, count=2500)
    elif name == "L4c":
        n = 16
        specs = _specs(n, [14] * n, 106)
        # one tile holding nothing but the empty set and D_v itself (without
        # D_v the support would not have 14 bits), one with the 1500 extra sets
        specs[5] = dict(support=specs[5]["support"], count=0, crafted="span", dense=False)
        specs[9]["dense"] = True
    elif name == "L5a":
        n = 26
        specs = _specs(n, [(5 * i) % 9 for i in range(11)] + [25] + [(3 * i) % 9 for i in range(14)], 107, count=2500)
    elif name == "L5b":
        n = 26
        specs = _specs(n, [14] * 20 + [25] + [14] * 5, 108, count=2500)
    elif name == "L6":
        n = 63  # the library's limit (a varset keeps bit 63 free)
        rng = np.random.default_rng(109)
        specs = [None] * n
        for v, m in ((0, 12), (31, 9), (32, 12), (62, 11)):
            pool = [b for b in range(30, 63) if b != v]
            specs[v] = dict(support=sum(1 << int(b) for b in rng.choice(pool, m, replace=False)), count=200, max_size=4)
    elif name in ("L7", "L7hole"):
        n = 12
        allm = (1 << n) - 1
        specs = [dict(support=allm & ~(1 << v), count=120, max_size=4) for v in range(n)]
        if name == "L7hole":
            specs[0]["support"] &= ~(1 << 5)
            specs[11]["support"] &= ~(1 << 0)
    elif name == "L8":
        n = 20
        specs = _specs(n, [12] * n, 110, count=400)
    elif name == "L9":
        n = 8
        specs = _specs(n, [7, 5, 7, 3, 6, 7, 0, 4], 111, count=40)
    else:
        raise KeyError(name)
    offs, sets, costs, crafted = lr.make_lists(n, specs, 1000 + sum(map(ord, name)), kind=kind)
    return n, offs, sets, costs, crafted


def _diff(got, want):
    bad = np.nonzero(lr.fold_zero(got) != lr.fold_zero(want))[0]
    return [(int(i), float(got[i]), float(want[i])) for i in bad[:5]]


def _check_tables(ctx, lat, scope=None, owned=None):
    for v in range(lat.n):
        sup, got = ctx.bestscore_table(v)
        if owned is not None and not (owned >> v) & 1:
            assert got.size == 0, v
            continue
        D, want, _ = lat.table(v, scope)
        assert sup == D, (v, hex(sup), hex(D))
        assert got.size == want.size == 1 << bin(D).count("1")
        assert not _diff(got, want), (v, len(want), _diff(got, want))


def _check_queries(ctx, lat, vs, Ss):
    gc, gp = ctx.bestscore(vs, Ss)
    wc, wp = lat.best_many(vs, Ss)
    bad = np.nonzero((lr.fold_zero(gc) != lr.fold_zero(wc)) | (gp != wp))[0]
    assert bad.size == 0, [(int(vs[i]), hex(int(Ss[i])), float(gc[i]), float(wc[i]), hex(int(gp[i])), hex(int(wp[i])))
                           for i in bad[:5]]


def _check_case(ctx, name, kind, only=None):
    n, offs, sets, costs, crafted = _case(name, kind)
    lat = lr.Lattice(n, offs, sets, costs)
    ctx.search_load(offs, sets, costs)
    _check_tables(ctx, lat)
    vs, Ss = lr.queries(n, lat, crafted, NQ, 7, only=only)
    _check_queries(ctx, lat, vs, Ss)
    return lat


@pytest.fixture
def ctx(ulg_ctx):
    try:
        yield ulg_ctx
    finally:
        ulg_ctx.set_option("table_budget_kb", 0)


# ---- lattice -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["L1a1", "L1a2", "L1b", "L2", "L4c", "L7", "L7hole"])
def test_small_tables(ctx, name, kind):
    """L1: one-entry tables, FLT_MAX entries, tiles below 2^14.  L2: the LDS
    tile kernel with 1, 2 and 4 tiles and the LDS strided kernel with G = 1
    and 2, at table offsets that are no multiple of the table size.  L4c: the
    register tile kernel with no pass B.  L7: bs_index's two-shift path at
    v = 0 and v = n - 1, and pext_sparse when one bit is missing."""
    lat = _check_case(ctx, name, kind)
    if name == "L7":
        assert all(lat.support(v) == lat.all & ~(1 << v) for v in range(lat.n))
    if name == "L7hole":
        assert bin(lat.support(0)).count("1") == 10 and bin(lat.support(11)).count("1") == 10
    if name == "L2":
        assert [bin(lat.support(v)).count("1") for v in range(8)] == [13, 14, 15, 16, 3, 0, 14, 9]
    if name == "L4c":
        assert all(bin(lat.support(v)).count("1") == 14 for v in range(lat.n))
        assert lat.offs[6] - lat.offs[5] == 2 and lat.offs[10] - lat.offs[9] >= 1500


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["L3", "L4a", "L4b"])
def test_tables_of_2_24(ctx, name, kind):
    """L3: LDS path, pass B with G = 10 and G = 5 in one launch.  L4a: sorted
    entries, register tile kernel, register strided kernel (full window).
    L4b: register tile kernel, then the LDS strided kernel (m = 15 leaves a
    window of one bit).  The sets behind the costs are checked through the
    queries; the reference transform for m = 24 is the uint32 one."""
    lat = _check_case(ctx, name, kind)
    ms = sorted(bin(lat.support(v)).count("1") for v in range(lat.n))
    assert ms[-1] == 24
    if name == "L3":
        assert ms[-2] == 19 and ms[0] < 14
    if name == "L4a":
        assert ms[-2] == 24 and ms[0] == 14
    if name == "L4b":
        assert ms[-2] == 15 and ms[0] == 14


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["L5a", "L5b"])
def test_tables_of_2_25(ctx, name, kind):
    """The second pass-B round (bit_lo = 24, G = 1, nlow = 20): after the LDS
    tile kernel (L5a) and after the register tile and strided kernels (L5b)."""
    lat = _check_case(ctx, name, kind)
    ms = sorted(bin(lat.support(v)).count("1") for v in range(lat.n))
    assert ms[-1] == 25 and (ms[0] == 14 if name == "L5b" else ms[0] < 14)


@pytest.mark.parametrize("kind", KINDS)
def test_top_variables(ctx, kind):
    """L6 at the widest problem the library takes: n = 63 (n = 64 is refused,
    a varset keeps bit 63 free), lists on variables 0, 31, 32 and 62, supports
    above bit 29, S with bit 62 set."""
    lat = _check_case(ctx, "L6", kind, only=[0, 31, 32, 62])
    sup = [lat.support(v) for v in (0, 31, 32, 62)]
    assert any(s >> 62 for s in sup[:3]) and all(s and s >> 30 << 30 == s for s in sup)
    top = (1 << 63) - 1
    vs = np.array([62, 62, 0, 31, 32], dtype=np.int32)
    Ss = np.array([top, top ^ (1 << 62), 1 << 62, (1 << 62) | (1 << 61), 3 << 61], dtype=np.uint64)
    _check_queries(ctx, lat, vs, Ss)
    offs = np.zeros(65, dtype=np.int64)
    with pytest.raises(ulg.ULGError, match="status 1"):
        ctx.search_load(offs, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float32))
    _check_queries(ctx, lat, vs, Ss)   # the refused load left the lists alone


def _need_kib(lat, scope, per_entry):
    """KiB of dense tables over the stored sets inside scope."""
    tot = sum(1 << bin(lat.support(v, scope)).count("1") for v in range(lat.n))
    return tot * per_entry / 1024.0


@pytest.mark.parametrize("kind", KINDS)
def test_scoped_build(ctx, kind):
    """L8: a budget below the full tables: no tables after the load, tables
    for the scope after pdb_build(2, anc, scc), one-entry tables outside it,
    queries inside and outside the scope, and the same PDB as with budget 0.
    Then a larger scope the budget refuses: the old tables stay and answer."""
    n, offs, sets, costs, crafted = _case("L8", kind)
    lat = lr.Lattice(n, offs, sets, costs)
    scc, anc = 0b00000101100100110010, 0b01001000000001000000
    scope = scc | anc
    assert bin(scope).count("1") == 10 and not scc & anc
    # 16 B per entry as test_gpu_scoped._need_kib counts; the build asks for 12
    budget = int(_need_kib(lat, scope, 16)) + 1
    assert _need_kib(lat, lat.all, 12) > budget
    ctx.set_option("table_budget_kb", budget)
    ctx.search_load(offs, sets, costs)
    with pytest.raises(ulg.ULGError, match="status 3"):
        ctx.bestscore_table(0)
    vs, Ss = lr.queries(n, lat, crafted, 4000, 8)
    _check_queries(ctx, lat, vs, Ss)          # list scans
    ctx.pdb_build(2, anc, scc)
    _check_tables(ctx, lat, scope)
    for v in range(n):
        if not (scope >> v) & 1:
            assert ctx.bestscore_table(v)[1].size == 1
    rng = np.random.default_rng(3)
    vin = rng.integers(0, n, 6000).astype(np.int32)   # variables inside and outside the scope
    Sin = rng.integers(0, 1 << n, 6000).astype(np.uint64) & np.uint64(scope)
    _check_queries(ctx, lat, np.concatenate([vs, vin]), np.concatenate([Ss, Sin]))
    groups, pd = lat.pdb(2, anc, scc)
    scoped = [ctx.pdb_table(g) for g in range(2)]
    for g in range(2):
        assert scoped[g][0] == groups[g] and not _diff(scoped[g][1], pd[g])
    # a scope the budget refuses: the tables built for `scope` stay in use
    scc2 = lat.all & ~0b11
    assert _need_kib(lat, scc2, 12) > budget
    _check_pdb(ctx, lat, 3, 0, scc2)
    _check_tables(ctx, lat, scope)
    _check_queries(ctx, lat, np.concatenate([vs, vin]), np.concatenate([Ss, Sin]))
    ctx.set_option("table_budget_kb", 0)
    ctx.search_load(offs, sets, costs)
    ctx.pdb_build(2, anc, scc)
    _check_tables(ctx, lat)
    for g in range(2):
        mask, vals = ctx.pdb_table(g)
        assert mask == scoped[g][0] and np.array_equal(vals.view(np.uint32), scoped[g][1].view(np.uint32))


@pytest.fixture
def own_ctx():
    c = ulg.Context(0)
    try:
        yield c
    finally:
        c.close()


@pytest.mark.parametrize("kind", KINDS)
def test_sharded_tables_and_back(own_ctx, kind):
    """L9: tables for the owned variables only, list scans for the others,
    and every table again after pdb_build on the same context (one of its
    own: the sharded sweep's state stays with it)."""
    ctx = own_ctx
    n, offs, sets, costs, crafted = _case("L9", kind)
    lat = lr.Lattice(n, offs, sets, costs)
    own = 0b00101101
    ctx.search_load(offs, sets, costs)
    ctx.sweep_shard_begin(own)
    _check_tables(ctx, lat, owned=own)
    vs, Ss = lr.queries(n, lat, crafted, 0, 9)
    assert len(vs) >= 8 * 256
    _check_queries(ctx, lat, vs, Ss)
    ctx.pdb_build(2)
    _check_tables(ctx, lat)
    _check_queries(ctx, lat, vs, Ss)
    groups, pd = lat.pdb(2)
    for g in range(2):
        mask, vals = ctx.pdb_table(g)
        assert mask == groups[g] and not _diff(vals, pd[g])


def test_load_paths_agree(ctx):
    """L10: ulg_search_load_scores from host pointers and from a device
    tensor, and ulg_search_load of ulg_quantize_costs' output, build the same
    tables: n = 6 with all 32 parent sets per variable, 16 rounds of 192
    scores from the once-per-binade "%f" sweep (3072 scores)."""
    n = 6
    sets, offs = [], [0]
    for v in range(n):
        others = [b for b in range(n) if b != v]
        sets += [sum(1 << others[i] for i in range(5) if (r >> i) & 1) for r in range(32)]
        offs.append(len(sets))
    sets = np.array(sets, dtype=np.uint64)
    offs = np.array(offs, dtype=np.int64)
    vals = pct_f_values.binade_sweep()
    rng = np.random.default_rng(10)
    scores = np.concatenate([vals[-256:], rng.permutation(vals[:-256])])[:16 * len(sets)]
    assert len(scores) == 3072
    dsets = torch.from_numpy(sets.view(np.int64)).cuda()
    for r in range(16):
        sc = np.ascontiguousarray(scores[r * len(sets):(r + 1) * len(sets)])
        costs = ctx.quantize(sc)
        want = np.array([pct_f_values.expected_cost(x) for x in sc], dtype=np.float32)
        assert np.array_equal(costs.view(np.uint32), want.view(np.uint32))
        lat = lr.Lattice(n, offs, sets, want)
        ctx.search_load(offs, sets, costs)
        _check_tables(ctx, lat)
        a = [ctx.bestscore_table(v) for v in range(n)]
        ctx.search_load_scores(offs, sets, sc)
        b = [ctx.bestscore_table(v) for v in range(n)]
        dsc = torch.from_numpy(sc).cuda()
        torch.cuda.synchronize()
        ctx.search_load_scores(offs, dsets.data_ptr(), dsc.data_ptr(), device_ptrs=True)
        c = [ctx.bestscore_table(v) for v in range(n)]
        for v in range(n):
            for other in (b[v], c[v]):
                assert other[0] == a[v][0] and np.array_equal(other[1].view(np.uint32), a[v][1].view(np.uint32)), (r, v)


def test_reload_leaves_nothing_stale(ctx):
    """L11: smaller lists loaded on a context that held L4a."""
    n, offs, sets, costs, _ = _case("L4a", "ints")
    ctx.search_load(offs, sets, costs)
    assert ctx.bestscore_table(7)[1].size == 1 << 24
    for name in ("L1b", "L1a1", "L2"):
        _check_case(ctx, name, "wide")


# ---- pattern database ----------------------------------------------------------
def _h_sets(n, scc, seed):
    if n <= 12:
        return np.arange(1 << n, dtype=np.uint64)
    rng = np.random.default_rng(seed)
    allm = (1 << n) - 1
    Ss = rng.integers(0, 1 << 63, NQ, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, NQ, dtype=np.uint64)
    Ss &= np.uint64(allm)
    Ss[::2] |= np.uint64(allm & ~scc)   # only scc variables remaining: the `complete` branch
    return np.concatenate([Ss, np.array([0, allm, scc & allm, ~scc & allm], dtype=np.uint64)])


def _check_pdb(ctx, lat, pd_count, anc, scc, seed=5):
    ctx.pdb_build(pd_count, anc, scc)
    groups, pd = lat.pdb(pd_count, anc, scc)
    for g in range(pd_count):
        mask, vals = ctx.pdb_table(g)
        assert mask == groups[g], (g, hex(mask), hex(groups[g]))
        assert vals.size == pd[g].size and not _diff(vals, pd[g]), (g, _diff(vals, pd[g]))
    Ss = _h_sets(lat.n, scc, seed)
    gh, gc = ctx.pdb_h(Ss)
    wh, wc = lat.h_many(Ss)
    bad = np.nonzero((lr.fold_zero(gh) != lr.fold_zero(wh)) | (gc != wc))[0]
    assert bad.size == 0, [(hex(int(Ss[i])), float(gh[i]), float(wh[i]), int(gc[i]), int(wc[i])) for i in bad[:5]]
    return lat.zero_sum_share()


def _pdb_case(ctx, n, kind, seed, no_empty=None, at=None, must=None, N=None):
    N, offs, sets, costs = lr.pdb_lists(n, kind, seed, no_empty, at, must=must, N=N)
    ctx.search_load(offs, sets, costs)
    return lr.Lattice(N, offs, sets, costs)


@pytest.mark.parametrize("kind", ["ints", "real"])
def test_pdb_small_shapes(ctx, kind):
    """P1: n = 1..6 x pd_count = 1..8 over the full scc: uneven and empty
    groups ((5, 4) -> 2,2,1,0; (3, 8) -> five empty groups).  The zero share
    is asserted over the family: single cases are too small to hold a tenth."""
    zero = []
    for n in range(1, 7):
        lat = _pdb_case(ctx, n, kind, 40 + n, no_empty=(n - 1 if kind == "real" else None))
        for pd_count in range(1, 9):
            zero.append(_check_pdb(ctx, lat, pd_count, 0, lat.all))
            if (n, pd_count) == (5, 4):
                assert [bin(g).count("1") for g in lat.groups] == [2, 2, 1, 0]
            if (n, pd_count) == (3, 8):
                assert [bin(g).count("1") for g in lat.groups] == [1, 1, 1, 0, 0, 0, 0, 0]
    if kind == "ints":
        assert np.mean(zero) >= 0.1, np.mean(zero)


P2_SCC = 0b1011001101101


@pytest.mark.parametrize("budget", [0, 1], ids=["tables", "listscan"])
@pytest.mark.parametrize("kind", ["ints", "real"])
def test_pdb_gaps_and_ancestors(ctx, kind, budget):
    """P2: n = 13, pd = 3: the full scc (5, 5, 3), a scc with gaps and the
    complement as ancestors, the same scc with no ancestors (variables outside
    both).  P5: the same under a 1 KiB budget: the first two scopes get no
    tables and every lookup scans the lists; the third is small enough to fit
    even 1 KiB and is held to table(v, scope)."""
    ctx.set_option("table_budget_kb", budget)
    # real: variables 2, 3 and 9 store no empty set and every set of theirs
    # holds variable 1, which lies outside P2_SCC
    lat = _pdb_case(ctx, 13, kind, 50, no_empty=((2, 3, 9) if kind == "real" else None), must=1)
    share, scanned = [], 0
    for anc, scc in ((0, lat.all), (lat.all & ~P2_SCC, P2_SCC), (0, P2_SCC)):
        share.append(_check_pdb(ctx, lat, 3, anc, scc))
        if scc == lat.all:
            assert [bin(g).count("1") for g in lat.groups] == [5, 5, 3]
        if not budget:
            _check_tables(ctx, lat)
        elif _need_kib(lat, anc | scc, 12) > budget:
            scanned += 1   # no tables: every lookup of this build scanned the lists
            with pytest.raises(ulg.ULGError, match="status 3"):
                ctx.bestscore_table(0)
        else:
            _check_tables(ctx, lat, anc | scc)   # a scope this small fits even 1 KiB
    assert not budget or scanned >= 2
    if kind == "ints":
        assert min(share) >= 0.1, share
    else:
        vals = np.concatenate(lat.pd)   # no admissible set for 2, 3 and 9: FLT_MAX + x, and inf in {0, 2, 3}
        assert (vals == lr.FLT_MAX).any() and np.isinf(vals).any()


@pytest.mark.parametrize("kind", ["ints", "real"])
def test_pdb_top_variables(ctx, kind):
    """P3 at n = 63 (the library's limit): scc inside bits {2, 31, 32, 40, 61,
    62}, pd = 2 and 3, with and without an ancestor."""
    at = (2, 31, 32, 40, 61, 62)
    lat = _pdb_case(ctx, 6, kind, 60, no_empty=(4 if kind == "real" else None), at=at, N=63)
    scc = sum(1 << b for b in at)
    share = [_check_pdb(ctx, lat, 2, 0, scc), _check_pdb(ctx, lat, 3, 0, scc),
             _check_pdb(ctx, lat, 2, 1 << 2, scc & ~(1 << 2)), _check_pdb(ctx, lat, 3, 1 << 62, scc & ~(1 << 62))]
    if kind == "ints":
        assert np.mean(share) >= 0.1, share


@pytest.mark.parametrize("kind", ["ints", "real"])
def test_pdb_one_group_of_18(ctx, kind):
    """P4: n = 18, pd = 1: 2.4 M leaf scores, layer launches of 1024 blocks."""
    lat = _pdb_case(ctx, 18, kind, 74, no_empty=(7 if kind == "real" else None))
    share = _check_pdb(ctx, lat, 1, 0, lat.all)
    if kind == "ints":
        assert share >= 0.1, share


def test_pdb_refusals(ctx):
    """P6: the argument limits with their status codes; the context goes on
    answering bestscore queries after each."""
    n = 26
    specs = [dict(support=1 << ((v + 1) % n), count=1, max_size=1) for v in range(n)]
    offs, sets, costs, crafted = lr.make_lists(n, specs, 80, kind="ints")
    lat = lr.Lattice(n, offs, sets, costs)
    ctx.search_load(offs, sets, costs)
    vs, Ss = lr.queries(n, lat, crafted, 500, 81)

    def refused(status, *args):
        with pytest.raises(ulg.ULGError, match=f"status {status}"):
            ctx.pdb_build(*args)
        _check_queries(ctx, lat, vs, Ss)
        for what in (lambda: ctx.pdb_h([0]), lambda: ctx.pdb_table(0)):
            with pytest.raises(ulg.ULGError, match="status 3"):
                what()

    with pytest.raises(ulg.ULGError, match="status 3"):
        ctx.pdb_h([0])
    with pytest.raises(ulg.ULGError, match="status 3"):
        ctx.pdb_table(0)
    refused(1, 0, 0, lat.all)
    refused(1, 9, 0, lat.all)
    refused(4, 1, 0, lat.all)              # one group of 26
    refused(4, 2, 0b0110, 0b1100)          # ancestors overlap the scc
    ctx.pdb_build(2, 0, lat.all)           # 13 + 13
    groups, pd = lat.pdb(2, 0, lat.all)
    for g in range(2):
        mask, vals = ctx.pdb_table(g)
        assert mask == groups[g] and not _diff(vals, pd[g])
    for g in (-1, 2):
        with pytest.raises(ulg.ULGError, match="status 1"):
            ctx.pdb_table(g)
    with pytest.raises(ulg.ULGError, match="status 1"):
        ctx.bestscore_table(n)
    # a refused build leaves no half-updated pattern database behind
    refused(4, 1, 0, lat.all)
