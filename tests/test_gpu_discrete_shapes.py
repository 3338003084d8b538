"""Discrete BIC on the GPU at the shapes test_gpu_discrete.py never reaches:
tables of thousands of cells and the 16384 / 32768-cell limits of the dense
path, the hash path at its natural size (in LDS and in the HBM slab), more work
items than workgroups with both paths in one launch, the slab-bounded grid,
compaction over hundreds of scan blocks with holes, variables from bit 32 up,
arities up to 255, and the fixed-point scale below 2^32.

Every value is held to the kernel's own contract, not to the reference's
float32 summation: |gpu - exact64| <= Bk with exact64 from
test_discrete.exact_value (math.fsum over numpy.unique counts) and
    Bk = ulp_f32(exact64) / 2 + 2 (T 2^-(shift+1) + (T + 3) 2^-52 (A + pen)),
derived term by term in test_discrete.py's docstring.  Counts, stored sets,
offsets and totals are exact, and the dense and the hash path must agree bit
for bit wherever both can run.  Tables of more than 10^6 cells (input b) are
penalty-dominated in float32: they check the table shape, the 64-bit q, that
probing terminates and, where read back, the counts -- not the log-likelihood.

Inputs and pair lists live in test_discrete.py (shape_input, shape_pairs) so
that the CPU suite can assert Bk's resolving power on the same data."""
import functools
import itertools
import math
import time

import numpy as np
import pytest

import ulg
from test_discrete import (CAND_A2, CAND_F, N_G, SAMPLE_A2, SETS_A, SETS_A2, SETS_B, SMALL_B, VARS_F, combos,
                           counts_table, disc_shift, exact_from_counts, exact_value, exact_value_batch, g_counts,
                           g_joint, kernel_bound, list_order, pairs_f, parents_of, q_of, shape_input, shape_pairs)

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def exact_of(name):
    """{(v, mask): (exact64, Bk)} for shape_pairs(name): computed once, never modified."""
    codes, arity = shape_input(name)
    N = codes.shape[0]
    out = {}
    for v, m in zip(*shape_pairs(name)):
        if (v, m) not in out:
            ex, T, A = exact_value(codes, arity, v, m)
            out[(v, m)] = (ex, kernel_bound(ex, T, A, arity[v], q_of(arity, v, m), N))
    return out


def _within(name, vs, ps, got, what=""):
    ex = exact_of(name)
    worst = 0.0
    for v, m, g in zip(vs, ps, got):
        e, bk = ex[(int(v), int(m))]
        assert abs(float(g) - e) <= bk, (name, what, int(v), hex(int(m)), float(g), e, bk)
        worst = max(worst, abs(float(g) - e) / bk)
    print(f"{name} {what}: {len(vs)} values, at most {worst:.3f} Bk")


def _cells(arity, vs, ps):
    return [q_of(arity, v, m) * arity[v] for v, m in zip(vs, ps)]


def _counts_equal(ctx, codes, arity, v, m):
    """discrete_counts against numpy.unique on the 64-bit cell index (no q r_v allocation on this side)."""
    got = ctx.discrete_counts(v, m)
    q = q_of(arity, v, m)
    assert got.dtype == np.int32 and len(got) == q * arity[v]
    idx = np.zeros(codes.shape[0], dtype=np.int64)
    b = 1
    for p in parents_of(m & ~(1 << v)):
        idx += codes[:, p].astype(np.int64) * b
        b *= arity[p]
    keys, cnt = np.unique(idx + codes[:, v].astype(np.int64) * q, return_counts=True)
    nz = np.flatnonzero(got)
    assert np.array_equal(nz, keys) and np.array_equal(got[nz], cnt), (v, hex(m))


def _want_list(name, v, cand, k, cons=()):
    """[(mask, exact64, Bk)] in list order: layers ascending, masks ascending, R3 / R5 / R6."""
    codes, arity = shape_input(name)
    N = codes.shape[0]
    cs = parents_of(cand & ~(1 << v))
    alts = [(r, f) for cv, r, f in cons if cv == v]
    out = []
    for L in range(min(len(cs), k) + 1):
        for m in sorted(sum(1 << p for p in comb) for comb in itertools.combinations(cs, L)):
            if alts and not any((r & ~m) == 0 and (m & f) == 0 for r, f in alts):
                continue
            if arity[v] == 1:
                if L == 0:
                    out.append((m, 0.0, 0.0))
                continue
            ex, T, A = exact_value(codes, arity, v, m)
            bk = kernel_bound(ex, T, A, arity[v], q_of(arity, v, m), N)
            assert ex < -1.0 - bk  # BIC is decisively negative: R3 keeps the set whatever the rounding
            out.append((m, ex, bk))
    return out


def _check_lists(got, want):
    offs, sets, scores = got
    assert len(offs) == len(want) + 1 and offs[0] == 0
    for i, lst in enumerate(want):
        assert offs[i + 1] - offs[i] == len(lst), f"list {i}: length"
        assert [int(x) for x in sets[offs[i]:offs[i + 1]]] == [m for m, _, _ in lst], f"list {i}: sets differ"
        for (m, e, bk), g in zip(lst, scores[offs[i]:offs[i + 1]]):
            assert abs(float(g) - e) <= bk, (i, hex(m), float(g), e, bk)
    assert offs[-1] == sum(len(lst) for lst in want)


# ---- a. large dense tables, the 16384 and 32768 boundaries ------------------------------
def test_a_large_dense_tables_and_the_default_limit(ctx):
    """Tables of 192 to 16384 cells in the LDS histogram (zeroing and the per-configuration reduction
    take their 256-stride up to 64 and 16 times), 49152 cells on the hash path at default options."""
    codes, arity = shape_input("a")
    vs, ps = [v for v, _ in SETS_A], [m for _, m in SETS_A]
    assert _cells(arity, vs, ps) == [192, 768, 1024, 3072, 4096, 12288, 12288, 16384, 49152, 49152]
    assert [q_of(arity, v, m) for v, m in SETS_A[2:8]] == [256, 1024, 1024, 4096, 3072, 4096]
    ctx.load_discrete(codes, arity)
    default = ctx.score_sets_discrete(vs, ps)
    _within("a", vs, ps, default, "default options")
    for v, m in SETS_A:
        _counts_equal(ctx, codes, arity, v, m)
    ctx.set_option("disc_dense_cells", 32768)  # 128 KB of LDS, the option's maximum
    assert ctx.score_sets_discrete(vs, ps).tobytes() == default.tobytes()
    for v, m in SETS_A[5:]:
        _counts_equal(ctx, codes, arity, v, m)
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete(vs, ps).tobytes() == default.tobytes(), "dense and sparse paths differ"
    for v, m in SETS_A[5:]:
        _counts_equal(ctx, codes, arity, v, m)
    # which path a set takes is only counted by score_discrete
    ctx.set_option("disc_dense_cells", 16384)
    for v, k in ((7, 6), (7, 7), (0, 7)):
        others = [p for p in range(8) if p != v]
        tables = [arity[v] * math.prod(arity[p] for p in comb) for L in range(k + 1)
                  for comb in itertools.combinations(others, L)]
        st, sc = ctx.score_discrete([v], [0xFF], k)
        assert sc == len(tables) == st
        assert ctx.info("disc_sparse_sets") == sum(t > 16384 for t in tables)
        assert ctx.info("disc_dense_sets") == sum(t <= 16384 for t in tables)
        # v = 7, k = 6: nothing above 3 * 4^6 = 12288 cells; k = 7: the one set of 3 * 4^7; v = 0: one table
        # of 4^7 = 16384 cells, still dense, and the one of 4^7 * 3
        assert max(tables) == (12288 if k == 6 else 49152) and (16384 in tables) == (v == 0)
        assert sum(t > 16384 for t in tables) == (0 if k == 6 else 1)
        _check_lists(ctx.fetch(st), [_want_list("a", v, 0xFF, k)])


def test_a_dense_limit_at_its_maximum(ctx):
    """Tables of 16385 to 32768 cells move from the hash path to the histogram at disc_dense_cells = 32768."""
    codes, arity = shape_input("a2")
    vs, ps = [v for v, _ in SETS_A2], [m for _, m in SETS_A2]
    assert _cells(arity, vs, ps) == [16384, 24576, 32768, 49152, 98304]
    ctx.load_discrete(codes, arity)
    default = ctx.score_sets_discrete(vs, ps)
    _within("a2", vs, ps, default, "default options")
    ctx.set_option("disc_dense_cells", 32768)
    assert ctx.score_sets_discrete(vs, ps).tobytes() == default.tobytes()
    for v, m in SETS_A2:
        _counts_equal(ctx, codes, arity, v, m)
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete(vs, ps).tobytes() == default.tobytes()
    # all 2^14 parent sets of variable 0 among the binary columns: one table of 32768 cells, 14 of 16384
    cand = CAND_A2
    lists = {}
    for limit, sparse in ((16384, 1), (32768, 0)):
        ctx.set_option("disc_dense_cells", limit)
        st, sc = ctx.score_discrete([0], [cand], 14)
        assert sc == 1 << 14 and ctx.info("disc_sparse_sets") == sparse
        assert ctx.info("disc_dense_sets") == (1 << 14) - sparse
        lists[limit] = ctx.fetch(st)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(lists[16384], lists[32768]))
    offs, sets, scores = lists[32768]
    assert offs.tolist() == [0, 1 << 14] and [int(m) for m in sets] == list_order(parents_of(cand), 14)
    _within("a2", [0] * len(SAMPLE_A2), [int(sets[i]) for i in SAMPLE_A2], scores[SAMPLE_A2], "sampled list entries")


# ---- b. the hash path at its natural size ------------------------------------------------
@pytest.mark.parametrize("name", ["b1500", "b2100"])
def test_b_sparse_tables_at_natural_size(ctx, name):
    """N = 1500: 8192 hash slots in LDS; N = 2100: 16384 slots in the HBM slab.  Arities 255 and 200:
    13,005,000 cells with the counts read back (a 52 MB table), then 2.08e8 and 5.5e16 cells, value
    only (penalty-dominated: q in 64 bits, probing terminates)."""
    codes, arity = shape_input(name)
    N = codes.shape[0]
    slots = 64
    while slots < 4 * N:
        slots *= 2
    assert slots == (8192 if name == "b1500" else 16384) and codes.max() == 254
    vs, ps = [v for v, _ in SETS_B], [m for _, m in SETS_B]
    cells = _cells(arity, vs, ps)
    assert cells[:2] == [13_005_000, 208_080_000] and 2 ** 40 < q_of(arity, *SETS_B[2]) and cells[2] < 2 ** 63
    assert len(parents_of(SETS_B[2][1])) == 6 and all(254 in codes[:, p] for p in (8, 9, 10, 11, 12, 13))
    ctx.load_discrete(codes, arity)
    got = ctx.score_sets_discrete(vs, ps)
    _within(name, vs, ps, got)
    assert ctx.score_sets_discrete(vs[::-1], ps[::-1])[::-1].tobytes() == got.tobytes()
    for i in range(3):
        assert ctx.score_sets_discrete(vs[i:i + 1], ps[i:i + 1]).tobytes() == got[i:i + 1].tobytes()
    _counts_equal(ctx, codes, arity, *SETS_B[0])
    # the same records, smaller tables: dense and hash path agree bit for bit
    small_v, small_p = [v for v, _ in SMALL_B], [m for _, m in SMALL_B]
    assert _cells(arity, small_v, small_p) == [1020, 3200, 1020, 3060]
    dense = ctx.score_sets_discrete(small_v, small_p)
    _within(name, small_v, small_p, dense, "small tables")
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete(small_v, small_p).tobytes() == dense.tobytes()
    for v, m in SMALL_B:
        _counts_equal(ctx, codes, arity, v, m)


# ---- c. more items than workgroups, both paths in one launch -----------------------------
@pytest.mark.parametrize("name", ["c300", "c2100"])
def test_c_grid_stride_with_mixed_paths(ctx, name):
    """disc_dense_cells = 64 splits the 2560 tables of n = 10, k <= 4 between the histogram and the hash
    table (in LDS at N = 300, in the slab at N = 2100).  One launch of 2560 shuffled items (2048
    workgroups), one of 7680: a workgroup takes dense and hash items in turn and reuses its LDS."""
    codes, arity = shape_input(name)
    vs, ps = shape_pairs(name)
    assert len(vs) == 2560
    cells = np.array(_cells(arity, vs, ps))
    n_sparse = int((cells > 64).sum())
    print(f"{name}: {n_sparse} of 2560 tables above 64 cells, largest {cells.max()}")
    assert n_sparse > 300 and 2560 - n_sparse > 300
    perm = np.random.default_rng(7).permutation(2560)
    pv, pp = [vs[i] for i in perm], [ps[i] for i in perm]
    ctx.load_discrete(codes, arity)
    ctx.set_option("disc_dense_cells", 64)
    got = ctx.score_sets_discrete(pv, pp)
    _within(name, pv, pp, got, "2560 shuffled items")
    value = {(v, m): g for v, m, g in zip(pv, pp, got)}
    # the layers of score_discrete: 10, 90, 360, 840 and 1260 items
    st, sc = ctx.score_discrete(list(range(10)), [1023] * 10, 4)
    assert (st, sc) == (2560, 2560)
    assert ctx.info("disc_sparse_sets") == n_sparse and ctx.info("disc_dense_sets") == 2560 - n_sparse
    offs, sets, scores = ctx.fetch(st)
    assert offs.tolist() == [256 * i for i in range(11)]
    for v in range(10):
        want = [m for x, m in zip(vs, ps) if x == v]  # pairs_up_to: layers ascending
        want = [m for L in range(5) for m in sorted(w for w in want if bin(w).count("1") == L)]
        assert [int(x) for x in sets[offs[v]:offs[v + 1]]] == want
        assert scores[offs[v]:offs[v + 1]].tobytes() == np.array([value[(v, m)] for m in want], np.float32).tobytes()
    # 7680 items over 2048 workgroups
    three = ctx.score_sets_discrete(pv * 3, pp * 3)
    assert three.tobytes() == np.tile(got, 3).tobytes()
    pick = np.random.default_rng(8).choice(2560, size=50, replace=False)
    for i in pick:
        assert ctx.score_sets_discrete(pv[i:i + 1], pp[i:i + 1])[0].tobytes() == got[i].tobytes(), (pv[i], pp[i])
    for limit in (16384, 512, 8):  # everything dense; another split; everything above 8 cells hashed
        ctx.set_option("disc_dense_cells", limit)
        assert ctx.score_sets_discrete(pv * 3, pp * 3).tobytes() == three.tobytes(), limit


# ---- d. the slab-bounded grid ------------------------------------------------------------
def test_d_slab_bounded_grid(ctx):
    """N = 20000: 131072 hash slots, 196608 words per workgroup, so disc_work caps the grid at
    floor(2^28 / 196608) = 1365 workgroups for the 1536 items.  Allocates 2.1 GB of slabs on the device."""
    codes, arity = shape_input("d")
    N = codes.shape[0]
    slots = 64
    while slots < 4 * N:
        slots *= 2
    per = slots + slots // 2
    assert (slots, per, (1 << 28) // per) == (131072, 196608, 1365)
    vs, ps = shape_pairs("d")
    assert len(vs) == 192
    ctx.load_discrete(codes, arity)
    dense = ctx.score_sets_discrete(vs * 8, ps * 8)
    _within("d", vs * 8, ps * 8, dense, "dense")
    ctx.set_option("disc_dense_cells", 8)
    t0 = time.perf_counter()
    sparse = ctx.score_sets_discrete(vs * 8, ps * 8)
    print(f"d: 1536 items on 1365 slab workgroups in {time.perf_counter() - t0:.2f} s")
    assert len(sparse) == 1536 > 1365 and sparse.tobytes() == dense.tobytes()
    for v, m in ((0, 0b111110), (5, 0b001011)):
        want, _ = counts_table(codes, arity, v, m)
        assert np.array_equal(ctx.discrete_counts(v, m), want)


# ---- e. compaction over many blocks, with holes ------------------------------------------
CONS_E = [(2, 1 << 20, 0),                          # requires a parent of index >= 16
          (5, 0, 1 << 3 | 1 << 25),                 # forbids two parents
          (11, 1 << 0, 1 << 1), (11, 1 << 28, 0),   # two alternatives
          (23, 1 << 4, 0), (23, 1 << 29, 1 << 4),   # every alternative requires a parent: no empty set
          (0, 1 << 7, 1 << 19),                     # requires one constant column, forbids the other
          (19, 1 << 3, 0)]                          # a constant variable whose empty set violates
PER_VAR_E = sum(math.comb(29, L) for L in range(5))


@functools.lru_cache(maxsize=None)
def _expected_e():
    """Per variable (masks uint64, exact64, Bk, kept under CONS_E) in list order, unconstrained lists:
    every set of the 28 two-valued variables (BIC < 0 for any counts), the empty set of the other two."""
    codes, arity = shape_input("e")
    N = codes.shape[0]
    ar = np.asarray(arity, dtype=np.int64)
    out = []
    for v in range(30):
        others = [p for p in range(30) if p != v]
        masks, exact, bound = [], [], []
        for L in range(5 if arity[v] > 1 else 1):
            sets = combos(others, L)
            mk = (np.uint64(1) << sets.astype(np.uint64)).sum(axis=1, dtype=np.uint64)
            ex, T, A = exact_value_batch(codes, arity, v, sets)
            pen = (arity[v] - 1) * ar[sets].prod(axis=1) * math.log(N) / 2
            bk = np.ldexp(1.0, np.frexp(np.abs(ex))[1] - 25) + \
                2.0 * (T * 2.0 ** -(disc_shift(N) + 1) + (T + 3) * 2.0 ** -52 * (A + pen))
            order = np.argsort(mk)
            masks.append(mk[order])
            exact.append(ex[order])
            bound.append(bk[order])
        masks, exact, bound = np.concatenate(masks), np.concatenate(exact), np.concatenate(bound)
        assert arity[v] == 1 or (exact < -1.0).all()
        alts = [(np.uint64(r), np.uint64(f)) for cv, r, f in CONS_E if cv == v]
        keep = np.ones(len(masks), dtype=bool)
        if alts:
            keep = np.zeros(len(masks), dtype=bool)
            for r, f in alts:
                keep |= ((r & ~masks) == 0) & ((masks & f) == 0)
        for a in (masks, exact, bound, keep):
            a.setflags(write=False)
        out.append((masks, exact, bound, keep))
    return out


def _check_e(got, variables, constrained):
    exp = _expected_e()
    offs, sets, scores = got
    at = 0
    for i, v in enumerate(variables):
        masks, exact, bound, keep = exp[v]
        sel = keep if constrained else np.ones(len(masks), dtype=bool)
        assert offs[i] == at, (i, v)
        at += int(sel.sum())
        assert np.array_equal(sets[offs[i]:at], masks[sel]), (i, v)
        assert (np.abs(scores[offs[i]:at].astype(np.float64) - exact[sel]) <= bound[sel]).all(), (i, v)
    assert offs[len(variables)] == at == len(sets)
    return at


def test_e_compaction_across_many_blocks_with_holes(ctx):
    """835,230 slots: 408 scan blocks, so disc_scan_kernel runs with two blocks per thread; layers 3 and 4
    are 109,620 and 712,530 items on 2048 workgroups.  Two constant columns and constraints on six
    variables leave holes of every size, across block boundaries."""
    codes, arity = shape_input("e")
    assert 30 * PER_VAR_E == 835_230 and -(-835_230 // 2048) == 408 > 256 and PER_VAR_E % 2048
    exp = _expected_e()
    full = [(1 << 30) - 1] * 30
    ctx.load_discrete(codes, arity)
    st0, sc0 = ctx.score_discrete(list(range(30)), full, 4)
    plain = ctx.fetch(st0)
    assert sc0 == 835_230 and st0 == 28 * PER_VAR_E + 2 == _check_e(plain, range(30), False)
    assert ctx.info("disc_sparse_sets") == 0 and ctx.info("disc_dense_sets") == 28 * PER_VAR_E
    # the same call with every table above 8 cells hashed: three or more parents that have two values.
    # Layers 3 and 4 then mix both paths (a constant parent halves the table), 2048 workgroups taking
    # dozens to hundreds of items each in disc_layer_kernel
    ar = np.asarray(arity)
    hashed = sum(int((2 * ar[combos([p for p in range(30) if p != v], L)].prod(axis=1) > 8).sum())
                 for v in range(30) if arity[v] > 1 for L in range(5))
    ctx.set_option("disc_dense_cells", 8)
    st8, sc8 = ctx.score_discrete(list(range(30)), full, 4)
    assert (st8, sc8) == (st0, sc0) and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.fetch(st8), plain))
    assert hashed == 28 * (math.comb(27, 3) + math.comb(27, 4) + 2 * math.comb(27, 3)) == 737_100
    assert ctx.info("disc_sparse_sets") == hashed
    assert ctx.info("disc_dense_sets") == 28 * PER_VAR_E - hashed == 42_448
    ctx.set_option("disc_dense_cells", 16384)
    ctx.set_constraints(CONS_E)
    st, sc = ctx.score_discrete(list(range(30)), full, 4)
    cons = ctx.fetch(st)
    assert sc == 835_230 and st == _check_e(cons, range(30), True) == sum(int(e[3].sum()) for e in exp)
    assert st < st0 and exp[19][3].sum() == 0 and not exp[23][3][0] and exp[7][3].tolist() == [True]
    # the constrained lists are the unconstrained ones minus the violating sets, bit for bit
    po, _, pv = plain
    offs, sets, scores = cons
    for v in range(30):
        assert pv[po[v]:po[v + 1]][exp[v][3]].tobytes() == scores[offs[v]:offs[v + 1]].tobytes(), v
    # 11 variables in another order: every toff[i * S] but the first lies inside a scan block
    some = [29, 3, 7, 14, 0, 23, 19, 8, 2, 11, 5]
    st2, sc2 = ctx.score_discrete(some, [full[0]] * 11, 4)
    assert sc2 == 11 * PER_VAR_E
    o2, s2, v2 = ctx.fetch(st2)
    assert st2 == _check_e((o2, s2, v2), some, True)
    for i, v in enumerate(some):
        assert s2[o2[i]:o2[i + 1]].tobytes() == sets[offs[v]:offs[v + 1]].tobytes()
        assert v2[o2[i]:o2[i + 1]].tobytes() == scores[offs[v]:offs[v + 1]].tobytes()
    ctx.clear_constraints()
    st3, _ = ctx.score_discrete(list(range(30)), full, 4)
    assert st3 == st0 and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.fetch(st3), plain))


# ---- f. variables from bit 32 up ---------------------------------------------------------
def test_f_variables_and_parents_from_bit_32_up(ctx):
    codes, arity = shape_input("f")
    cons = [(40, 0, 1 << 33)]
    ctx.load_discrete(codes, arity)
    vs, ps = pairs_f()
    assert all(m >> 30 and not m >> 44 for m in ps) and sum(1 for m in ps if m >> 32) > 150
    got = ctx.score_sets_discrete(vs, ps)
    _within("f", vs, ps, got, "200 pairs with parents in 30..43")
    st0, _ = ctx.score_discrete(VARS_F, [CAND_F] * 8, 3)
    plain = ctx.fetch(st0)
    want0 = [_want_list("f", v, CAND_F, 3) for v in VARS_F]
    _check_lists(plain, want0)
    want, _ = counts_table(codes, arity, 43, 1 << 32 | 1 << 5)
    assert np.array_equal(ctx.discrete_counts(43, 1 << 32 | 1 << 5), want)
    ctx.set_constraints(cons)
    st, sc = ctx.score_discrete(VARS_F, [CAND_F] * 8, 3)
    wantc = [_want_list("f", v, CAND_F, 3, cons) for v in VARS_F]
    assert sc == sum(sum(math.comb(len(parents_of(CAND_F & ~(1 << v))), L) for L in range(4)) for v in VARS_F)
    assert st == sum(len(w) for w in wantc) < st0
    constrained = ctx.fetch(st)
    _check_lists(constrained, wantc)
    assert ctx.score_sets_discrete([40, 40], [1 << 33, 1 << 33 | 1 << 43]).tolist() == [1.0, 1.0]
    ctx.clear_constraints()
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete(vs, ps).tobytes() == got.tobytes()
    st8, _ = ctx.score_discrete(VARS_F, [CAND_F] * 8, 3)
    assert st8 == st0 and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.fetch(st8), plain))
    assert ctx.info("disc_sparse_sets") > 0


def test_f_the_last_variable_of_63(ctx):
    codes, arity = shape_input("f63")
    assert codes.shape[1] == 63
    vs, ps = shape_pairs("f63")
    ctx.load_discrete(codes, arity)
    got = ctx.score_sets_discrete(vs, ps)
    _within("f63", vs, ps, got)
    for v, m in ((62, 1 << 33 | 1 << 2), (3, 1 << 62), (62, 1 << 61 | 1 << 0)):
        want, _ = counts_table(codes, arity, v, m)
        assert np.array_equal(ctx.discrete_counts(v, m), want), (v, hex(m))
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete(vs, ps).tobytes() == got.tobytes()
    want, _ = counts_table(codes, arity, 3, 1 << 62)
    assert np.array_equal(ctx.discrete_counts(3, 1 << 62), want)


# ---- g. the fixed-point scale below 2^32 (keep this test last: 124 MB of records) ---------
def test_g_fixed_point_scale_31(ctx):
    """N = 62,000,000: N ln N >= 2^30, so disc_data() takes shift = 31 and fix_nlogn / g2_of scale by
    2^-31.  The threshold is arithmetic: no smaller input reaches it.  The last step scores one pair on
    the hash path: 4N rounds up to 2^28 slots, a single workgroup's slab, and that slab allocates
    3.2 GB on the device (disc_work's 2 GiB bound on the slabs gives way to its minimum of one
    workgroup).  About 4.4 s on an MI355X, 1.8 s of it that step."""
    t0 = time.perf_counter()
    codes, arity = shape_input("g")
    N = N_G
    ex = math.frexp(N * math.log(N))[1]  # disc_data(): N ln N < 2^ex
    assert N * math.log(N) >= 2 ** 30 and min(32, 62 - ex) == 31 == disc_shift(N)
    joint = g_joint()
    t1 = time.perf_counter()
    ctx.load_discrete(codes, arity)
    vs, ps = shape_pairs("g")
    got = ctx.score_sets_discrete(vs, ps)
    for v, m, g in zip(vs, ps, got):
        tab, q = g_counts(v, m)
        nj = tab.reshape(-1, q).sum(axis=0)
        e, T, A = exact_from_counts(tab[tab > 0], nj[nj > 0], arity[v], q, N)
        bk = kernel_bound(e, T, A, arity[v], q, N)
        print(f"g: v={v} P={m:#x} gpu={float(g):.1f} exact={e:.3f} Bk={bk:.3g}")
        assert abs(float(g) - e) <= bk, (v, m, float(g), e, bk)
        assert np.array_equal(ctx.discrete_counts(v, m), tab)
    # G^2 of the two orders, under test_gpu_disc_mmpc.py's bound at shift 31
    g2, dof, cells = ctx.g2_discrete([0, 1], [1, 0], [0, 0])

    def nlogn(a):
        a = a[a > 1].astype(np.float64)
        return math.fsum((a * np.log(a)).tolist()), int(a.size)

    (sxt, c1), (sz, c2) = nlogn(joint.ravel()), nlogn(np.array([N]))
    (sx, c3), (st_, c4) = nlogn(joint.sum(axis=0)), nlogn(joint.sum(axis=1))
    want = max(2.0 * (sxt + sz - sx - st_), 0.0)
    terms, total = c1 + c2 + c3 + c4, sxt + sz + sx + st_
    bound = 2.0 * (terms * 2.0 ** -(31 + 1) + (terms + 4) * 2.0 ** -52 * total)
    print(f"g: G2 gpu={g2[0]:.9f} restated={want:.9f} bound={bound:.3g}")
    assert dof.tolist() == [6, 6] and cells.tolist() == [12, 12] and g2[0] == g2[1]
    assert abs(g2[0] - want) <= bound
    t2 = time.perf_counter()
    # the hash path: one workgroup, 2^28 slots in a 3.2 GB slab
    ctx.set_option("disc_dense_cells", 8)
    assert ctx.score_sets_discrete([0], [2]).tobytes() == got[2:3].tobytes()
    t3 = time.perf_counter()
    print(f"g: input {t1 - t0:.1f} s, load + dense + G2 {t2 - t1:.1f} s, hash path {t3 - t2:.1f} s")
