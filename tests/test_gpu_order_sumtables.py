"""GPU tests of the order MCMC over dense log-sum tables (option "mcmc_tables", ulg_order_mcmc_table;
kernels: csrc/order_sumtables.hip) against tests/order_sumtables_ref.py.  A table slot is held to the
long-double sum within the derived slot cap; a chain is then restated on the device's OWN read-back tables,
where every sum is the same IEEE adds of the same doubles: every comparison there is equality."""
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import order_mcmc_ref as om
import order_sumtables_ref as st
import ulg
from test_gpu_order_mcmc_cli import _sample_lines
from test_gpu_order_tables import READBACK_K, pooled_lists, readback_lists
from test_gpu_posterior_cli import _read_pss
from test_gpu_posterior_sample_cli import _run

pytestmark = pytest.mark.gpu

KEYS = ("order", "log_score", "parents", "log_weight", "trace_delta", "trace_accept", "accepted")


@pytest.fixture()
def ctx():
    c = ulg.Context(0)
    yield c
    c.close()


def _bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _status(call, *a, **kw):
    with pytest.raises(ulg.ULGError) as e:
        call(*a, **kw)
    return int(re.search(r"status (\d+)", str(e.value)).group(1)), str(e.value)


@pytest.mark.parametrize("v", sorted(READBACK_K), ids=lambda v: f"K{READBACK_K[v]}")
def test_table_is_the_log_sum_of_every_subset(ctx, v):
    L = readback_lists()
    ctx.order_mcmc_begin(*L.triple(), 1, init_order=np.arange(62, -1, -1, dtype=np.uint8)[None], tables=True)
    C, T = ctx.order_mcmc_table(v)
    want, count, cap = st.direct(L, v)
    assert C == int(np.bitwise_or.reduce(L.sets[v])) and len(T) == 1 << READBACK_K[v] == len(want)
    assert all(u > 31 for u in st.members(C)) and (T[0] == -np.inf) == (v == 7)
    assert np.array_equal(T == -np.inf, count == 0) and not np.isnan(T).any()
    assert _bits(T[count == 1], want[count == 1].astype(np.float64))  # a single entry: that score's bits
    many = count > 1
    err = np.abs(T[many].astype(np.longdouble) - want[many]).astype(np.float64)
    print(f"K = {READBACK_K[v]}: the largest error is {float((err / cap[many]).max(initial=0.0)):.3f} of its cap")
    assert np.all(err <= cap[many])


@pytest.mark.parametrize("n", [5, 8, 33, 63])
def test_chains_equal_the_restatement_on_the_device_tables(ctx, n):
    L, seed = st.chain_inputs()[n]
    ctx.order_mcmc_begin(*L.triple(), st.CHAINS, seed=seed, tables=True)
    tables = [ctx.order_mcmc_table(v) for v in range(n)]
    if n == 63:
        assert sorted({len(T) for _, T in tables}) == [1 << 4, 1 << 13, 1 << 14, 1 << 15]
    r = ctx.order_mcmc_run(st.STEPS, st.THIN, trace=True)
    ref = st.run(L, tables, seed, st.CHAINS, st.STEPS, st.THIN)
    assert _bits(r["trace_delta"], ref["trace_delta"])  # IEEE adds of the same doubles
    u_acc = np.stack([om.moves(seed, t, np.arange(st.CHAINS), n)[2] for t in range(1, st.STEPS + 1)])
    acc, margin, slack = om.decide(r["trace_delta"], None, u_acc)  # each decision from the device's delta, exp's 8 units apart
    assert np.array_equal(acc, r["trace_accept"].astype(bool)) and np.all(margin >= slack) and ref["min_excess"] >= 0
    for k in KEYS:
        assert _bits(r[k], ref[k]), k
    order, terms, step = ctx.order_mcmc_state()
    assert step == st.STEPS and _bits(order, ref["final_order"]) and _bits(terms, ref["final_terms"])
    assert 0 < r["accepted"].sum() < st.CHAINS * st.STEPS
    # the two contracts meet: the table terms against the list terms of the same orders
    lists = ctx.order_score(order)
    _, term_cap, _ = om.order_terms(L, order)
    caps = [st.direct(L, v)[2] for v in range(n)]
    slot_cap = np.array([[caps[v][st.index(st.members(tables[v][0]), U)] for v, U in zip(o, p)] for o, p in zip(order, om.prefixes(order))])
    assert np.all(np.abs(terms - lists) <= term_cap + slot_cap)


def test_invariance(ctx):
    L, seed = st.chain_inputs()[33]

    def begin(chains):
        ctx.order_mcmc_begin(*L.triple(), chains, seed=seed, tables=True)

    begin(64)
    whole = ctx.order_mcmc_run(st.STEPS, st.THIN, trace=True)
    state = ctx.order_mcmc_state()
    for chains in (1, 4):
        begin(chains)
        part = ctx.order_mcmc_run(st.STEPS, st.THIN, trace=True)
        for k in KEYS:
            assert _bits(part[k], np.ascontiguousarray(whole[k][..., :chains, :] if whole[k].ndim == 3 else whole[k][..., :chains])), k
    begin(64)
    a, b = ctx.order_mcmc_run(70, st.THIN, trace=True), ctx.order_mcmc_run(80, st.THIN, trace=True)
    for k in KEYS:
        assert _bits(b[k] if k == "accepted" else np.concatenate([a[k], b[k]]), whole[k]), k
    assert all(_bits(x, y) for x, y in zip(ctx.order_mcmc_state(), state))
    ctx.set_option("mcmc_launch_steps", 7)
    begin(64)
    r = ctx.order_mcmc_run(st.STEPS, st.THIN, trace=True)
    ctx.set_option("mcmc_launch_steps", 4096)
    assert all(_bits(r[k], whole[k]) for k in KEYS)


def test_orders_follow_their_exact_law_at_n4(ctx):
    L, seed, T, chains = om.stat_inputs()[4]
    ctx.order_mcmc_begin(*L.triple(), chains, seed=seed, tables=True)
    r = ctx.order_mcmc_run(T, T, want_parents=False)
    perms, pi = om.order_law(L)
    counts = {}
    for o in r["order"][0]:
        key = tuple(int(x) for x in o)
        counts[key] = counts.get(key, 0) + 1
    om.chi_square("orders-4 over tables", counts, {p: float(x) for p, x in zip(perms, pi)}, chains, ulg.chi2_log_sf)


def test_refusals(ctx):
    UNSUPPORTED, STATE = 4, 3
    wide = pooled_lists(30, 1, lambda v: 27 if v == 2 else 1, lambda v: 0)  # variable 2: 27 single-parent sets
    code, text = _status(ctx.order_mcmc_begin, *wide.triple(), 2, tables=True)
    assert code == UNSUPPORTED and "variable 2 " in text and str(8 << 27) in text
    assert _status(ctx.order_mcmc_run, 1)[0] == STATE
    ctx.order_mcmc_begin(*wide.triple(), 2)  # the lists themselves are fine
    assert _status(ctx.order_mcmc_table, 2)[0] == STATE and ctx.info("mcmc_tables") == 0
    ctx.order_mcmc_begin(*wide.triple(), 2, init_order=np.tile(np.arange(30, dtype=np.uint8), (2, 1)))
    assert ctx.order_mcmc_run(5)["records"] == 5


def test_command_line(ctx, tmp_path):
    L = pooled_lists(30, 77, lambda v: 5, lambda v: 12, max_parents=3)
    names = [f"X{v}" for v in range(30)]
    text = "META pss_version = 0.1\nMETA input_file=none\nMETA num_records=100\n\n"
    for v in range(30):
        text += f"VAR {names[v]}\nMETA arity=2\n" + "".join(
            f"{x:f} " + "".join(names[u] + " " for u in range(30) if (int(S) >> u) & 1) + "\n" for S, x in zip(L.sets[v], L.sc[v])) + "\n"
    pss, dags = tmp_path / "n30.pss", tmp_path / "dags.txt"
    pss.write_text(text)
    _, offs, sets, scores = _read_pss(pss)
    args = ("--mcmc", "--tables", "--chains", 8, "--burn", 50, "--thin", 5, "--sample", 40, "--seed", 3)
    r = _run(pss, *args, "-g", dags, "-o", os.devnull)
    assert r.returncode == 0, r.stderr
    ctx.order_mcmc_begin(offs, sets, scores, 8, seed=3, tables=True)
    ctx.order_mcmc_run(50, 5, want_order=False, want_score=False, want_parents=False)
    got = ctx.order_mcmc_run(25, 5)
    assert r.stdout.splitlines()[0].endswith(f", tables (K_max = 5, {8 * 30 * 32} bytes)") and r.stdout.startswith("order MCMC: 8 chains, 75 ")
    assert open(dags).read().splitlines() == _sample_lines(got, names, 40)
    r = _run(pss, *args, "--temper", 2)
    assert r.returncode == 2 and "--tables" in r.stderr
