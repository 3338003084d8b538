"""GPU tests of ulg_order_edges (kernel: csrc/order_edges.hip) against
tests/order_edges_ref.py, whose docstring derives the cap used here; it is not
measured on the device.  Each comparison prints
"order-edges-observed <family> <input> max <fraction of its cap>".

Contract: order_mcmc_ref.term_cases() with term_orders() -- n = 1, 2, 5, 33, 63,
list lengths around a wave's stride, a list whose sum passes 2^64 in T, scores
beyond 745 nats apart and an order of probability 0.  "equal-14" / "equal-15":
sums past 2^64 in N as well, the values known to the bit.  Geometry: the same
bits at every grid, split and grouping.  Identity: all 120 orders of n = 5
weighted by the exact order law give the exact edge matrix.  Statistics: 4096
chains against Context.posterior, and the variance against the 0/1 indicator's.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so: imported after it, torch reports no HIP GPU

import order_edges_ref as oe
import order_mcmc_ref as om
import posterior_ref as pr
import ulg

pytestmark = pytest.mark.gpu

STATUS = {"OK": 0, "ARG": 1, "HIP": 2, "STATE": 3, "UNSUPPORTED": 4}
LD = np.longdouble


def _status(excinfo):
    return int(re.search(r"status (\d+)", str(excinfo.value)).group(1))


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _begin(ctx, L, init_order=None):
    if init_order is None:
        init_order = np.arange(L.n, dtype=np.uint8)[None, :]  # a shuffle may start at an order of probability 0
    ctx.order_mcmc_begin(*L.triple(), 1, seed=0, init_order=init_order)


def _hold(family, name, got, ref):
    """got uint64 (K, n, n) per-order tables against order_edges_ref.order_edges()."""
    g, want = got.astype(np.int64), ref["g"].astype(np.int64)
    assert np.array_equal(g[ref["exact"]], want[ref["exact"]]), (family, name, "an entry that is 0 or 2^40 by the contract")
    loose = ~ref["exact"]
    frac = float((np.abs(g[loose] - want[loose]) / ref["cap"][loose]).max()) if loose.any() else 0.0
    print(f"order-edges-observed {family} {name} max {frac:.3g} of its cap")
    assert frac <= 1.0, (family, name, frac)


# ---- 1. the contract -----------------------------------------------------------------------
@pytest.mark.parametrize("name", oe.CONTRACT_CASES)
def test_contract(ctx, name):
    L, orders = oe.gpu_inputs()[name]
    ref = oe.reference(name)
    _begin(ctx, L)
    got, zero = ctx.order_edges(orders, groups=len(orders))
    assert got.shape == (len(orders), L.n, L.n) and zero == int(ref["dead"].sum())
    _hold("contract", name, got, ref)
    assert not got[ref["dead"]].any()
    if name == "dynamic-6":
        assert zero >= 1 and got[~ref["dead"]].any()
    assert np.all(got <= oe.FULL) and not got[:, np.arange(L.n), np.arange(L.n)].any()


# ---- 2. sums past 2^64 in N, to the bit ----------------------------------------------------
@pytest.mark.parametrize("n", oe.EQUAL_SIZES)
def test_equal_scores_give_a_half_to_the_bit(ctx, n):
    name = f"equal-{n}"
    L, orders = oe.gpu_inputs()[name]
    last = n - 1
    _begin(ctx, L)
    got, zero = ctx.order_edges(orders, groups=len(orders))
    assert zero == 0
    pre = om.prefixes(orders)
    want = np.zeros(got.shape, dtype=np.uint64)
    for k in range(len(orders)):
        p = int(np.flatnonzero(orders[k] == last)[0])
        for u in range(n):
            if (int(pre[k, p]) >> u) & 1:
                want[k, u, last] = oe.FULL // 2
    assert np.array_equal(got, want)
    # the order with every other variable first: N_u = 2^(n-2) 2^52 >= 2^64 and T = 2^(n-1) 2^52 (the reference's integers)
    _, _, _, _, N, T = oe.row(L, last, (1 << last) - 1)
    assert all(x >= 1 << 64 for x in N[:last]) and T >= 1 << 65
    k = int(np.flatnonzero(orders[:, last] == last)[0])
    assert np.all(got[k, :last, last] == oe.FULL // 2)
    assert np.array_equal(got, oe.reference(name)["g"])


# ---- 3. geometry and batching --------------------------------------------------------------
def test_the_same_bits_at_every_grid_split_and_grouping(ctx):
    L, orders = oe.gpu_inputs()["sparse-33"]
    K, n = orders.shape
    _begin(ctx, L)
    per, zero = ctx.order_edges(orders, groups=K)
    assert zero == 0 and ctx.info("edges_grid") == (K * n + 3) // 4
    for grid in (1, 7):
        ctx.set_option("edges_grid", grid)
        again, _ = ctx.order_edges(orders, groups=K)
        assert ctx.info("edges_grid") == grid and np.array_equal(per, again)
    ctx.set_option("edges_grid", 0)
    for bad in (-1, 65537):
        with pytest.raises(ulg.ULGError):
            ctx.set_option("edges_grid", bad)
    # count split 1 + the rest
    first, _ = ctx.order_edges(orders[:1], groups=1)
    rest, _ = ctx.order_edges(orders[1:], groups=K - 1)
    assert np.array_equal(first[0], per[0]) and np.array_equal(rest, per[1:])
    one, _ = ctx.order_edges(orders, groups=1)
    tail, _ = ctx.order_edges(orders[1:], groups=1)
    assert np.array_equal(one[0], first[0] + tail[0])
    # the per-order tables summed on the host
    assert np.array_equal(one, oe.group_sum(per, 1))
    three, _ = ctx.order_edges(orders, groups=3)
    assert np.array_equal(three, oe.group_sum(per, 3))
    mean = ulg.order_edge_posterior(one, K)
    m3, se3 = ulg.order_edge_posterior(three, [len(range(r, K, 3)) for r in range(3)])
    assert np.array_equal(mean, m3) and se3.shape == (n, n) and np.all(se3 >= 0)


# ---- 4. the identity, on the device --------------------------------------------------------
def test_order_average_is_the_exact_edge_matrix(ctx):
    L, orders = oe.gpu_inputs()["all-5"]
    ref = oe.reference("all-5")
    _begin(ctx, L)
    got, zero = ctx.order_edges(orders, groups=len(orders))
    assert zero == 0
    _hold("identity", "all-5", got, ref)
    perms, pi = om.order_law(L)
    assert np.array_equal(np.array(perms, dtype=np.uint8), orders)
    mean = (pi[:, None, None] * got.astype(LD)).sum(axis=0) / LD(oe.FULL)
    want = pr.brute(L.n, *L.triple())["edge"]
    tol = (ref["cap"].max(axis=0) + 1) * 2.0 ** -oe.EDGE_BITS
    dev = np.abs(mean.astype(np.float64) - want)
    print(f"order-edges-observed identity-brute all-5 largest deviation {dev.max():.3g}, tolerance {tol.max():.3g}")
    assert np.all(dev <= tol), dev.max()


# ---- 5. statistics -------------------------------------------------------------------------
def test_chains_against_the_exact_posterior(ctx):
    L, seed, T, chains = om.stat_inputs()[6]
    n = L.n
    ctx.order_mcmc_begin(*L.triple(), chains, seed=seed)
    r = ctx.order_mcmc_run(T, T)
    assert r["records"] == 1
    orders, parents = r["order"][0], r["parents"][0]
    got, zero = ctx.order_edges(orders, groups=chains)
    assert zero == 0
    mean, se = ulg.order_edge_posterior(got, np.ones(chains, dtype=np.int64))
    x = got.astype(np.float64) / oe.FULL
    assert np.allclose(se, x.std(axis=0, ddof=1) / np.sqrt(chains), rtol=1e-9, atol=1e-15)
    _, exact, _ = ctx.posterior(*L.triple(), want_sets=False)
    flat = se == 0
    sigma = np.abs(mean - exact)[~flat] / se[~flat]
    rb, ind = oe.variances(got, parents)
    print(f"order-edges-observed statistics n=6: worst deviation {sigma.max():.2f} standard errors, variance summed over the edges: "
          f"Rao-Blackwell {rb:.4f}, indicator {ind:.4f}")
    assert sigma.max() <= 5.0
    if flat.any():  # every order gives the same value: the value itself, within its cap
        ref = oe.order_edges(L, orders[:1])
        u, v = np.nonzero(flat)
        assert np.all(np.abs(got[0][u, v].astype(np.int64) - ref["g"][0][u, v].astype(np.int64)) <= ref["cap"][0][u, v])
        assert np.all(np.abs(mean - exact)[flat] <= (ref["cap"][0][u, v] + 1) * 2.0 ** -oe.EDGE_BITS)
    assert rb < ind


# ---- 6. errors -----------------------------------------------------------------------------
def _raw(ctx, count, orders, groups, edge, zero=None):
    return ulg.lib().ulg_order_edges(ctx._h, count, None if orders is None else ulg._ptr(orders), groups,
                                     None if edge is None else ulg._ptr(edge), None if zero is None else C.byref(zero))


def test_errors(ctx):
    L, orders = oe.gpu_inputs()["full-5"]
    K, n = orders.shape
    mark = np.uint64(0xABCDEF)
    edge = np.full((K, n, n), mark, dtype=np.uint64)
    zero = C.c_int64(-7)
    untouched = lambda: np.all(edge == mark) and zero.value == -7  # noqa: E731
    # without a begin, and after a refused one
    assert _raw(ctx, K, orders, 1, edge, zero) == STATUS["STATE"] and untouched()
    with pytest.raises(ulg.ULGError) as e:
        ctx.order_edges(orders)
    assert _status(e) == STATUS["STATE"]
    _begin(ctx, L)
    with pytest.raises(ulg.ULGError):
        ctx.order_mcmc_begin(*L.triple(), 0)
    assert _raw(ctx, K, orders, 1, edge, zero) == STATUS["STATE"] and untouched()
    _begin(ctx, L)
    before = ctx.order_score(orders)
    state = ctx.order_mcmc_state()
    live = ctx.info("device_bytes_live")
    good, z = ctx.order_edges(orders, groups=K)
    grid = ctx.info("edges_grid")
    assert z == 0 and grid > 0
    bad_row = orders.copy()
    bad_row[3, 1] = bad_row[3, 0]
    high = orders.copy()
    high[K - 1, 2] = n
    for count, o, groups, out in ((-1, orders, 1, edge), ((1 << 22) + 1, orders, 1, edge), (K, orders, 0, edge), (K, orders, -2, edge),
                                  (K, orders, K + 1, edge), (0, orders, 2, edge), (K, None, 1, edge), (K, orders, 1, None),
                                  (K, bad_row, 1, edge), (K, high, K, edge)):
        assert _raw(ctx, count, o, groups, out, zero) == STATUS["ARG"], (count, groups)
        assert untouched() and ctx.info("edges_grid") == grid and ctx.info("device_bytes_live") == live
    assert _raw(ctx, K, bad_row, 1, edge, zero) == STATUS["ARG"] and "order 3 is not a permutation" in ulg.lib().ulg_last_error(ctx._h).decode()
    with pytest.raises(ulg.ULGError) as e:
        ctx.order_edges(orders, groups=K + 1)
    assert _status(e) == STATUS["ARG"]
    with pytest.raises(ulg.ULGError):
        ctx.order_edges(orders[:, :4])  # the binding's own shape check
    # count = 0: the tables zero-filled, whatever they held; orders may be NULL
    assert _raw(ctx, 0, None, 1, edge[:1], zero) == STATUS["OK"] and zero.value == 0 and not edge[0].any() and np.all(edge[1:] == mark)
    empty, z = ctx.order_edges(np.zeros((0, n), dtype=np.uint8))
    assert empty.shape == (1, n, n) and not empty.any() and z == 0 and ctx.info("edges_grid") == 0
    # zero may be NULL
    edge[:] = mark
    assert _raw(ctx, K, orders, K, edge, None) == STATUS["OK"] and np.array_equal(edge, good)
    # the call's buffers are its own: nothing is held after it, the chains and the terms are as they were
    assert ctx.info("device_bytes_live") == live
    assert np.array_equal(before, ctx.order_score(orders))
    assert all(np.array_equal(a, b) for a, b in zip(state, ctx.order_mcmc_state()))


def test_tables_beyond_the_device_memory_are_refused():
    """count (n + 1) + 8 groups n^2 bytes against the free device memory: refused before anything is allocated.
    No call the arguments allow asks for more than 133 GB (2^22 orders, a table each, n = 63), so the test asks
    for 2^20 tables, 33 GB, and first holds free memory itself, down to 2 GiB below that request and no
    further.  While it holds it (the one refused call, well under a second) another process on the same card
    finds about 31 GB free and not the whole card: the hold is no larger than the refusal needs, and it goes
    back to the device, not into torch's cache, before the test ends."""
    n, count = 63, 1 << 20
    need = count * (n + 1) + 8 * count * n * n
    L = om.term_cases()["sparse-63"]
    ctx = ulg.Context(0)
    hold = None
    try:
        _begin(ctx, L)
        free, _ = torch.cuda.mem_get_info(0)
        leave = need - (2 << 30)
        if free > leave:
            hold = torch.empty(free - leave, dtype=torch.uint8, device="cuda:0")
        free, _ = torch.cuda.mem_get_info(0)
        assert free < need, "the device has more free memory than the largest call asks for"
        orders = np.tile(np.arange(n, dtype=np.uint8), (count, 1))
        edge = np.full(1, 5, dtype=np.uint64)  # never written: the call is refused
        small, _ = ctx.order_edges(orders[:2], groups=2)
        live, grid = ctx.info("device_bytes_live"), ctx.info("edges_grid")
        assert grid > 0 and _raw(ctx, count, orders, count, edge) == STATUS["UNSUPPORTED"]
        assert ctx.info("edges_grid") == grid  # the last call that ran, not the refused one
        assert "bytes of device memory" in ulg.lib().ulg_last_error(ctx._h).decode()
        assert edge[0] == 5 and ctx.info("device_bytes_live") == live
        small, z = ctx.order_edges(orders[:2], groups=2)  # the context goes on
        assert z == 0 and np.array_equal(small[0], small[1]) and small.any()
    finally:
        del hold
        torch.cuda.empty_cache()  # back to the device, not into torch's cache: later tests size their tables by the free memory
        ctx.close()
