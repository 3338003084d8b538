"""Every node of the GPU order-graph sweep (csrc/search_gpu.hip) against the
plain reference tests/sweep_ref.py, bit for bit.

Per case and per form of the sweep -- layer_pull_kernel<false> (sweep_table
0, and every filtered component), layer_pull_w32_kernel (1, first build and
cached slices), layer_pull_kernel<true> (2), each with and without the XCD
remap, and layer_shard_kernel + shard_commit_kernel for 1, 2 and 3 simulated
ranks -- the goal cost bits, the order, the parent sets, `expanded` and the
leaf byte of every node in layers 1..m equal the reference's; for the sharded
form so does every node's all-reduced key.  Lists go in through
ulg_search_load, so the inputs are synthetic and small; every comparison is
bitwise or integer.  The reference itself is held by test_sweep_ref.py."""
import functools
from math import comb

import numpy as np
import pytest
import torch  # at collection, before any test loads libulg.so: imported after it, torch reports no HIP GPU

import sweep_ref as sr

gpu = pytest.mark.gpu  # the conditions on the inputs need none: they run everywhere

NEAR = 1 / 1_000_000  # the relative window the older goal-cost checks could not see inside


def _full(n):
    return [(1 << n) - 1] * n


def _others(n):
    return [[p for p in range(n) if p != v] for v in range(n)]


def _block_rows(n, blocks):
    rows = [0] * n
    for b in blocks:
        mask = sum(1 << v for v in b)
        for v in b:
            rows[v] = mask
    return rows


def _block_pools(n, blocks):
    pools = [[] for _ in range(n)]
    for b in blocks:
        for v in b:
            pools[v] = [p for p in b if p != v]
    return pools


def _sym_rows(n, pairs):
    rows = [0] * n
    for a, b in pairs:
        rows[a] |= 1 << b
        rows[b] |= 1 << a
    return rows


def _row_pools(rows):
    n = len(rows)
    return [[p for p in range(n) if (rows[v] >> p) & 1 and p != v] for v in range(n)]


def _tie_lists(m):
    """Integer ties: the empty set at an integer cost in [-66, 0), 30 sets of
    1..3 parents at integer costs in [-200, 0)."""
    rng = np.random.default_rng(7)
    return sr.make_lists(m, _others(m), rng, 30, lambda r, k: r.integers(-200, 0, k).astype(np.float32),
                         empty_cost=lambda r, k: r.integers(-66, 0, k).astype(np.float32))


HIGH_BLOCK = [3, 9, 17, 22, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39]


def _high_blocks():
    rest = [v for v in range(40) if v not in HIGH_BLOCK]  # 26 variables, 0..29
    return [rest[0::3], rest[1::3], rest[2::3], HIGH_BLOCK]  # lowest variables 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> dict(n, lists, rows, filtered, pd_count)."""
    kind, _, arg = name.partition("_")
    pd = 2
    filtered = False
    if kind == "full":  # every support is the rest of the component: sweep_w_tile_kernel
        n = int(arg)
        lists = sr.make_lists(n, _others(n), np.random.default_rng(100 + n), 3 * n, sr.float_costs, cover=True)
        rows = _full(n)
    elif kind == "ties":
        n = int(arg)
        lists, rows = _tie_lists(n), _full(n)
    elif name == "zeros_4":
        n = 4
        lists = sr.make_lists(n, _others(n), np.random.default_rng(11), 6,
                              lambda r, k: np.where(r.integers(0, 2, k) == 1, -0.0, 0.0).astype(np.float32))
        rows = _full(n)
    elif name == "support_12":  # 4 of the other 11 variables each: sweep_w_kernel, pext_sparse
        n = 12
        rng = np.random.default_rng(12)
        pools = [sorted(int(x) for x in rng.choice([p for p in range(n) if p != v], 4, replace=False))
                 for v in range(n)]
        lists, rows = sr.make_lists(n, pools, rng, 12, sr.float_costs, cover=True), _full(n)
    elif name == "blocks_20":
        n = 20
        blocks = [[0, 3, 5, 6, 9, 12, 13, 17, 19], [1, 2, 4, 7, 8, 10, 11, 14, 15, 16, 18]]
        lists = sr.make_lists(n, _block_pools(n, blocks), np.random.default_rng(20), 30, sr.float_costs, cover=True)
        rows = _block_rows(n, blocks)
    elif name == "high_40":
        n, pd = 40, 4  # pattern-database groups of 10 variables
        blocks = _high_blocks()
        lists = sr.make_lists(n, _block_pools(n, blocks), np.random.default_rng(40), 30, sr.float_costs, cover=True)
        rows = _block_rows(n, blocks)
    elif name == "symsparse_14":
        n, filtered = 14, True
        rows = _sym_rows(n, [(i, (i + 1) % n) for i in range(n)] + [(0, 7), (3, 10), (5, 12)])
        lists = sr.make_lists(n, _row_pools(rows), np.random.default_rng(14), 8, sr.float_costs, cover=True)
    elif name == "asym_12":
        n, filtered = 12, True
        rows = _sym_rows(n, [(i, i + 1) for i in range(n - 1)] + [(0, 5), (2, 9), (4, 11), (6, 10)])
        pools = _row_pools(rows)
        for i in range(0, n, 3):  # drop one direction of a few edges
            nb = [j for j in range(n) if (rows[i] >> j) & 1 and j > i]
            rows[i] &= ~(1 << nb[0])
        lists = sr.make_lists(n, pools, np.random.default_rng(15), 8, sr.float_costs, cover=True)
    elif name == "nogoal_5":
        # 4's row is empty (it can only come first) but 0's row names it, so it
        # stays in the component; 1 and 2 admit only each other, so neither
        # can follow {4, ...}: nothing enters last
        n, filtered = 5, True
        rows = [0b11010, 0b00100, 0b00010, 0b00001, 0]
        lists = sr.make_lists(n, _others(n), np.random.default_rng(5), 6, sr.float_costs, cover=True)
    elif name == "chain_33":
        n, pd, filtered = 40, 4, True
        rows = _sym_rows(n, [(i, i + 1) for i in range(32)])
        lists = sr.make_lists(n, _row_pools(rows), np.random.default_rng(33), 0, sr.float_costs, cover=True)
    else:
        raise KeyError(name)
    return dict(n=n, lists=lists, rows=rows, filtered=filtered, pd_count=pd)


def _expect(case, near_rel=None):
    res, expanded = sr.search(case["n"], *case["lists"], rows=case["rows"], near_rel=near_rel)
    return res, expanded


def _check(case, res, leaves, what, ref=None):
    """cost bits, order, parent sets, expanded and every leaf byte of the
    last component against the reference."""
    comps, expanded = ref if ref is not None else _expect(case)
    last = comps[-1]
    m, n = len(last["layers"]) - 1, case["n"]
    assert np.float32(res["cost"]).tobytes() == last["cost"].tobytes(), (what, res["cost"], float(last["cost"]))
    assert [int(x) for x in res["order"][:m]] == last["order"], what
    for v in range(n):
        if v == 0 and len(comps) > 1:
            continue  # the reference's reconstruct quirk (test_gpu_dag_valid_sparse_components)
        assert int(res["vpar"][v]) == last["parents"].get(v, 0), (what, v)
    assert res["expanded"] == expanded, (what, res["expanded"], expanded)
    _check_leaves(leaves, last, what)


def _check_leaves(leaves, last, what):
    assert leaves.shape == last["leaves"].shape, what
    bad = np.nonzero(leaves[1:] != last["leaves"][1:])[0]
    if len(bad):
        i = int(bad[0]) + 1
        layer = next(d for d in range(len(last["layers"])) if sum(len(x) for x in last["layers"][:d + 1]) > i)
        rank = i - sum(len(x) for x in last["layers"][:layer])
        raise AssertionError(f"{what}: {len(bad)} leaf bytes differ, first at layer {layer} rank {rank} "
                             f"(node {int(last['layers'][layer][rank]):#x}): {leaves[i]} != {last['leaves'][i]}")


def _run_forms(ctx, case, forms, ref=None):
    ctx.search_load(*case["lists"])
    try:
        for xcd in (0, 1):
            ctx.set_option("sweep_xcd", xcd)
            for table in forms:
                ctx.set_option("sweep_table", table)
                res = ctx.astar(edges=case["rows"], pd_count=case["pd_count"], mode=1, net_text=False)
                _check(case, res, ctx.sweep_leaves(), f"sweep_table={table} sweep_xcd={xcd}", ref)
    finally:  # the library defaults (ulg_internal.h): the context is the session's
        ctx.set_option("sweep_table", 1)
        ctx.set_option("sweep_xcd", 1)


UNFILTERED = ["full_1", "full_2", "full_3", "full_9", "full_11", "full_12", "full_13", "full_14", "full_16",
              "ties_9", "ties_14", "zeros_4", "support_12", "blocks_20", "high_40"]
SHARDED = [c for c in UNFILTERED if c not in ("full_1", "blocks_20", "high_40")]  # one component of n >= 2 variables


# ---- conditions on the inputs, from the reference alone -----------------------------
@pytest.mark.parametrize("m", [9, 14])
def test_tie_cases_tie_and_spread(m):
    last = _expect(_case(f"ties_{m}"))[0][-1]
    nodes = np.concatenate(last["layers"][2:])
    tied = float((last["nmin"][nodes] >= 2).mean())
    moved = float((last["leafpos"][nodes] != 0).mean())
    assert 0.20 <= tied <= 0.90, tied
    assert moved >= 0.30, moved


def test_signed_zero_case_has_both_signs_and_a_plus_zero_goal():
    case = _case("zeros_4")
    bits = case["lists"][2].view(np.uint32)
    assert set(int(b) for b in bits) == {0, 0x80000000}
    assert _expect(case)[0][-1]["cost"].tobytes() == np.float32(0.0).tobytes()


def _connected_subsets(rows, n):
    count = 0
    for T in range(1, 1 << n):
        seen = fr = T & -T
        while fr:
            nb = 0
            for v in range(n):
                if (fr >> v) & 1:
                    nb |= rows[v]
            fr = nb & T & ~seen
            seen |= fr
        count += seen == T
    return count


def test_sparse_skeleton_cases_leave_nodes_unreached():
    for name in ("symsparse_14", "asym_12"):
        case = _case(name)
        comps, expanded = _expect(case)
        assert len(comps) == 1
        last = comps[0]
        assert (last["leaves"][1:] == sr.UNREACHED).mean() >= 0.10, name
        assert last["order"] is not None and last["cost"] < sr.FLT_MAX, name
        if name == "symsparse_14":  # root + connected proper subsets
            assert expanded == _connected_subsets(case["rows"], case["n"])
        else:
            sym = all(((case["rows"][i] >> j) & 1) == ((case["rows"][j] >> i) & 1)
                      for i in range(case["n"]) for j in range(case["n"]) if i != j)
            assert not sym
    comps, _ = _expect(_case("nogoal_5"))
    assert len(comps) == 1 and comps[0]["order"] is None and comps[0]["cost"] == sr.FLT_MAX
    assert comps[0]["leaves"][-1] == sr.UNREACHED


def test_cases_take_the_paths_they_are_for():
    for name in UNFILTERED:
        case = _case(name)
        offsets, sets, _ = case["lists"]
        for v in range(case["n"]):
            s = [int(x) for x in sets[offsets[v]:offsets[v + 1]]]
            assert s[0] == 0 and len(set(s)) == len(s), (name, v)  # the empty set; merged lists
    for name in ("full_12", "full_13", "full_14", "blocks_20", "high_40"):  # complete supports: the tile builder
        case = _case(name)
        offsets, sets, _ = case["lists"]
        for v in range(case["n"]):
            sup = int(np.bitwise_or.reduce(sets[offsets[v]:offsets[v + 1]]))
            assert sup == case["rows"][v] & ~(1 << v), (name, v)
    case = _case("support_12")
    offsets, sets, _ = case["lists"]
    assert all(bin(int(np.bitwise_or.reduce(sets[offsets[v]:offsets[v + 1]]))).count("1") == 4 for v in range(12))
    assert [len(c["layers"]) - 1 for c in _expect(_case("high_40"))[0]] == [9, 9, 8, 14]
    assert comb(13, 6) <= 7 * 256 and (comb(14, 7) + 255) // 256 == 14 and (comb(16, 8) + 255) // 256 == 51


# ---- the single-GPU forms ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", UNFILTERED)
def test_unfiltered_forms_equal_reference(ulg_ctx, name):
    _run_forms(ulg_ctx, _case(name), (0, 1, 1, 2))


@gpu
@pytest.mark.parametrize("name", ["symsparse_14", "asym_12"])
def test_filtered_sweep_equals_reference(ulg_ctx, name):
    _run_forms(ulg_ctx, _case(name), (1,))


@gpu
def test_unreachable_goal_is_a_clean_state_error(ulg_ctx):
    case = _case("nogoal_5")
    last = _expect(case)[0][-1]
    ulg_ctx.search_load(*case["lists"])
    with pytest.raises(RuntimeError, match="status 3.*a component has no goal"):
        ulg_ctx.astar(edges=case["rows"], mode=1, net_text=False)
    _check_leaves(ulg_ctx.sweep_leaves(), last, "no goal")


@gpu
def test_component_of_33_variables_is_unsupported(ulg_ctx):
    case = _case("chain_33")
    assert len(sr.components(case["rows"], case["n"])[0]) == 33
    ulg_ctx.search_load(*case["lists"])
    with pytest.raises(RuntimeError, match="status 4.*larger than 32"):
        ulg_ctx.astar(edges=case["rows"], pd_count=case["pd_count"], mode=1, net_text=False)
    with pytest.raises(RuntimeError, match="status 3"):
        ulg_ctx.sweep_leaves()  # the refused search left no finished sweep behind


@gpu
def test_sweep_leaves_without_a_sweep():
    import ulg
    ctx = ulg.Context(0)
    try:
        with pytest.raises(RuntimeError, match="status 3"):
            ctx.sweep_leaves()
    finally:
        ctx.close()


# ---- C2's lists: costs with fractional digits at g ~ 1e5 ---------------------------
@pytest.fixture(scope="module")
def c2_case(ulg_ctx):
    import synth
    n, N, k = 20, 10000, 4
    X, _ = synth.gaussian_sem(n, N, 9200)
    ulg_ctx.load(X, 2.0)
    offsets, sets, scores = ulg_ctx.score_all(list(range(n)), _full(n), k)
    lists = (np.asarray(offsets, dtype=np.int64), np.asarray(sets, dtype=np.uint64), ulg_ctx.quantize(scores))
    return dict(n=n, lists=lists, rows=_full(n), filtered=False, pd_count=2)


@gpu
def test_c2_lists_forms_equal_reference(ulg_ctx, c2_case):
    """n = 20, real lists.  In every layer 3..19 some node (374 in layer 3,
    50731 in layer 11, 6 in layer 19) has two candidates that differ in their
    bits but by less than one part in a million, so a sweep that took the
    wrong one of them passes a relative goal-cost check and fails here.  Seed
    9200 gives no such node in layer 2 (190 nodes of two candidates each) nor
    in layer 20 (the goal alone); layer 1 has one candidate per node."""
    ref = _expect(c2_case, NEAR)
    near = ref[0][-1]["near"]
    print("nodes with near-tied candidates per layer:", near)
    assert all(x >= 1 for x in near[3:20]), near
    _run_forms(ulg_ctx, c2_case, (0, 1, 1, 2), ref)


# ---- the sharded form, ranks simulated in one process -------------------------------
@pytest.fixture(scope="module")
def rank_ctxs():
    import ulg
    ctxs = [ulg.Context(0) for _ in range(3)]
    yield ctxs
    for c in ctxs:
        c.close()


def _worlds(n):
    import shard
    every = (1 << n) - 1
    worlds = [[every]]
    if n >= 2:
        worlds.append(shard.table_owners(n, 2))
    if n >= 3:  # uneven: one rank owns a single variable
        one = 1 << (n - 2)
        low = ((1 << (n // 2)) - 1) & ~one
        worlds.append([one, low, every & ~one & ~low])
    return worlds


def _run_sharded(ctxs, case, ref=None):
    n = case["n"]
    comps, expanded = ref if ref is not None else _expect(case)
    last = comps[-1]
    want = sr.shard_keys(last)
    for c in ctxs:
        c.search_load(*case["lists"])
    for owns in _worlds(n):
        assert all(owns) and sum(owns) == (1 << n) - 1 and len(set(owns)) == len(owns)
        ranks = ctxs[:len(owns)]
        maxl = [c.sweep_shard_begin(own) for c, own in zip(ranks, owns)]
        assert maxl == [max(comb(n, d) for d in range(n + 1))] * len(owns)
        keys = [torch.empty(maxl[0], dtype=torch.int64, device="cuda") for _ in ranks]
        for d in range(1, n + 1):
            cnt = comb(n, d)
            for c, k in zip(ranks, keys):
                c.sweep_shard_layer(d, k.data_ptr())
            red = keys[0][:cnt]
            for k in keys[1:]:
                red = torch.minimum(red, k[:cnt])
            red = red.contiguous()
            torch.cuda.synchronize()
            got = red.cpu().numpy().view(np.uint64)
            bad = np.nonzero(got != want[d])[0]
            assert len(bad) == 0, (f"world {len(owns)} layer {d}: {len(bad)} keys differ, first at rank "
                                   f"{int(bad[0])}: {int(got[bad[0]]):#x} != {int(want[d][bad[0]]):#x}")
            for c in ranks:
                c.sweep_shard_commit(d, red.data_ptr())
        for r, c in enumerate(ranks):
            _check(case, c.sweep_shard_end(), c.sweep_leaves(), f"world {len(owns)} rank {r}", (comps, expanded))


@gpu
@pytest.mark.parametrize("name", SHARDED)
def test_sharded_forms_equal_reference(rank_ctxs, name):
    _run_sharded(rank_ctxs, _case(name))


@gpu
def test_c2_lists_sharded_equal_reference(rank_ctxs, c2_case):
    _run_sharded(rank_ctxs, c2_case, _expect(c2_case, NEAR))


@gpu
def test_sharded_sweep_refuses_one_variable(rank_ctxs):
    case = _case("full_1")
    rank_ctxs[0].search_load(*case["lists"])
    with pytest.raises(RuntimeError, match="status 4"):
        rank_ctxs[0].sweep_shard_begin(1)
