"""GPU tests of a record's DAG drawn from the order MCMC's tables (option "mcmc_table_picks",
ulg_order_mcmc_stage_table; kernels: csrc/order_picktables.hip and the build kernels' snapshots in
csrc/order_sumtables.hip) against tests/order_picktables_ref.py.  A stage slot is held to its long-double
sum within the slot cap of the rounds that made it; the picks are then restated in Python integers on the
device's OWN read-back tables, where every comparison is equality."""
import functools
import os

import numpy as np
import pytest
import torch

import order_mcmc_ref as om
import order_picktables_ref as pk
import order_sumtables_ref as st
import ulg
from test_gpu_order_mcmc_cli import _sample_lines
from test_gpu_order_sumtables import _bits, _status, ctx  # noqa: F401  the context fixture and the two helpers
from test_gpu_order_tables import pooled_lists
from test_gpu_posterior_cli import _read_pss
from test_gpu_posterior_sample_cli import _run

pytestmark = pytest.mark.gpu

STEPS, THIN = 150, 7
CHAIN_KEYS = ("order", "log_score", "trace_delta", "trace_accept", "accepted")
KEYS = CHAIN_KEYS + ("parents", "log_weight")
STAGE_K = {0: 1, 1: 6, 2: 7, 3: 12, 4: 13, 5: 14, 6: 19, 7: 3}  # by variable: one to four chunks, both build paths; 7 has no empty set


@functools.lru_cache(maxsize=None)
def stage_lists():
    return pooled_lists(63, 3, lambda v: STAGE_K.get(v, 2), lambda v: 25 if v == 6 else 60, rooted=(7,), grid=2.0)


@functools.lru_cache(maxsize=None)
def chain_lists():
    """n -> (Lists, seed): K_v of one to four chunks among the variables of one order."""
    big33, big63 = {3: 7, 4: 12, 5: 13}, {40: 14, 41: 19, 42: 13, 43: 6, 44: 1}
    return {5: om.chain_inputs()["full-5"], 8: om.chain_inputs()["k3-8"],
            33: (pooled_lists(33, 31, lambda v: big33.get(v, 5), lambda v: 40, max_parents=3), 7),
            63: (pooled_lists(63, 41, lambda v: big63.get(v, 4), lambda v: 30, max_parents=6, grid=1.0), 9)}


@functools.lru_cache(maxsize=None)
def prefix_lists(n=28, K=25, wide=1):
    """Each of the variables 0 .. wide - 1 has the K + 1 nested prefixes of its candidates, the K least
    variables but itself, with scores 100 |P| (n = 28: variable 0, candidates 1 .. 25, five chunks); every
    other variable the empty set and one single parent."""
    offs, sets, scores = [0], [], []
    for v in range(n):
        pool = [u for u in range(n) if u != v][:K]
        mine = [sum(1 << u for u in pool[:k]) for k in range(K + 1)] if v < wide else [0, 1 << ((v + 3) % (n - 1) + 1)]
        sets += mine
        scores += [100.0 * bin(S).count("1") for S in mine] if v < wide else [-1.0, -1.5]
        offs.append(len(sets))
    return om.Lists(n, offs, np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))


@pytest.mark.parametrize("v", sorted(STAGE_K), ids=lambda v: f"K{STAGE_K[v]}")
def test_stage_tables_and_entry_map(ctx, v):
    L = stage_lists()
    init = np.arange(62, -1, -1, dtype=np.uint8)[None]
    ctx.order_mcmc_begin(*L.triple(), 1, init_order=init, tables=True, table_picks=True)
    C, T = ctx.order_mcmc_table(v)
    K, nch = STAGE_K[v], pk.chunks(STAGE_K[v])
    assert C == int(np.bitwise_or.reduce(L.sets[v])) and all(u > 31 for u in st.members(C)) and len(T) == 1 << K
    _, _, _, E = pk.build(L, v)
    assert np.array_equal(ctx.order_mcmc_stage_table(v, 0), E)
    for c in range(1, nch):
        S = ctx.order_mcmc_stage_table(v, c)
        want, count, cap = pk.direct(L, v, c)
        assert len(S) == 1 << K and np.array_equal(S == -np.inf, count == 0) and not np.isnan(S).any()
        assert _bits(S[count == 1], want[count == 1].astype(np.float64))
        many = count > 1
        err = np.abs(S[many].astype(np.longdouble) - want[many]).astype(np.float64)
        print(f"K = {K}, stage {c}: the largest error is {float((err / cap[many]).max(initial=0.0)):.3f} of its cap")
        assert np.all(err <= cap[many])
    assert _status(ctx.order_mcmc_stage_table, v, nch)[0] == 1 and _status(ctx.order_mcmc_stage_table, 63, 0)[0] == 1
    off = ulg.Context(0)  # the final table does not know of the snapshots
    try:
        off.order_mcmc_begin(*L.triple(), 1, init_order=init, tables=True)
        assert _bits(off.order_mcmc_table(v)[1], T)
    finally:
        off.close()


@pytest.mark.parametrize("n", [5, 8, 33, 63])
def test_records_equal_the_restatement_on_the_device_tables(ctx, n):
    L, seed = chain_lists()[n]
    chains = 2
    ctx.order_mcmc_begin(*L.triple(), chains, seed=seed, tables=True, table_picks=True)
    tables = [ctx.order_mcmc_table(v) for v in range(n)]
    staged = [([ctx.order_mcmc_stage_table(v, c) for c in range(1, pk.chunks(len(st.members(C))))], ctx.order_mcmc_stage_table(v, 0))
              for v, (C, _) in enumerate(tables)]
    if n >= 33:
        assert {pk.chunks(len(st.members(C))) for C, _ in tables} == ({1, 2, 3} if n == 33 else {1, 3, 4})
    r = ctx.order_mcmc_run(STEPS, THIN, trace=True)
    parents, lw = pk.run_records(L, tables, staged, seed, chains, zip(range(THIN, STEPS + 1, THIN), r["order"]))
    assert _bits(r["parents"], parents) and _bits(r["log_weight"], lw)
    pre = np.stack([om.prefixes(o) for o in r["order"]])
    stored = [set(int(S) for S in L.sets[v]) for v in range(n)]
    for o, p, par in zip(r["order"].reshape(-1, n), pre.reshape(-1, n), r["parents"].reshape(-1, n)):
        assert all(int(par[v]) in stored[v] and int(par[v]) & ~int(U) == 0 for v, U in zip(o, p))
    # the chains are the option-off chains of the same seed: only the DAGs differ
    ctx.order_mcmc_begin(*L.triple(), chains, seed=seed, tables=True)
    off = ctx.order_mcmc_run(STEPS, THIN, trace=True)
    assert all(_bits(r[k], off[k]) for k in CHAIN_KEYS)
    assert not _bits(r["parents"], off["parents"])


def test_invariance(ctx):
    L, seed = chain_lists()[33]

    def begin(chains):
        ctx.order_mcmc_begin(*L.triple(), chains, seed=seed, tables=True, table_picks=True)

    begin(64)
    whole = ctx.order_mcmc_run(STEPS, THIN, trace=True)
    for chains in (1, 4):
        begin(chains)
        part = ctx.order_mcmc_run(STEPS, THIN, trace=True)
        for k in KEYS:
            assert _bits(part[k], np.ascontiguousarray(whole[k][..., :chains, :] if whole[k].ndim == 3 else whole[k][..., :chains])), k
    begin(64)
    a, b = ctx.order_mcmc_run(70, THIN, trace=True), ctx.order_mcmc_run(80, THIN, trace=True)
    for k in KEYS:
        assert _bits(b[k] if k == "accepted" else np.concatenate([a[k], b[k]]), whole[k]), k
    ctx.set_option("mcmc_launch_steps", 7)
    begin(64)
    r = ctx.order_mcmc_run(STEPS, THIN, trace=True)
    ctx.set_option("mcmc_launch_steps", 4096)
    assert all(_bits(r[k], whole[k]) for k in KEYS)


def test_five_chunks_pick_the_dominant_prefix(ctx):
    L = prefix_lists()
    ctx.order_mcmc_begin(*L.triple(), 8, seed=5, tables=True, table_picks=True)
    r = ctx.order_mcmc_run(100, 10)
    seen = set()
    for o, par in zip(r["order"].reshape(-1, 28), r["parents"].reshape(-1, 28)):
        before = [int(u) for u in o[:list(o).index(0)]]
        k = next(k for k in range(27) if k + 1 not in before or k == 25)  # the largest prefix 1 .. k among them
        assert int(par[0]) == sum(1 << u for u in range(1, k + 1))
        seen.add(k)
    assert len(seen) >= 2


def test_refusals(ctx):
    ARG, STATE, UNSUPPORTED = 1, 3, 4
    L, seed = chain_lists()[8]
    code, text = _status(ctx.order_mcmc_begin, *L.triple(), 2, table_picks=True)
    assert code == ARG and "mcmc_tables" in text and ctx.info("mcmc_table_picks") == 0
    assert _status(ctx.order_mcmc_run, 1)[0] == STATE
    ctx.order_mcmc_begin(*L.triple(), 2, tables=True)
    assert _status(ctx.order_mcmc_stage_table, 0, 0)[0] == STATE
    ctx.order_mcmc_begin(*L.triple(), 2, tables=True, table_picks=True)
    assert _status(ctx.order_mcmc_stage_table, 0, 2)[0] == ARG and _status(ctx.order_mcmc_stage_table, -1, 0)[0] == ARG
    # the memory refusal.  Nothing the K <= 26 limit allows needs more than 63 x 44 x 2^26 bytes (186 GB), so the
    # test asks for 20 variables of K = 26, 59 GB, and first holds free memory itself: once, down to 2 GiB below
    # that need and no further, for the one refused begin.  Another process on the card finds about 57 GB free
    # meanwhile, not nothing, and the hold goes back to the device, not into torch's cache.
    need, hold, live = 20 * (44 << 26), None, ctx.info("device_bytes_live")  # the process's, the small chains above included
    try:
        free, _ = torch.cuda.mem_get_info(0)
        if free > need - (2 << 30):
            hold = torch.empty(free - (need - (2 << 30)), dtype=torch.uint8, device="cuda:0")
        assert torch.cuda.mem_get_info(0)[0] < need, "the device has more free memory than the begin asks for"
        code, text = _status(ctx.order_mcmc_begin, *prefix_lists(47, 26, 20).triple(), 2, tables=True, table_picks=True)
    finally:
        del hold
        torch.cuda.empty_cache()
    assert code == UNSUPPORTED and "variable 0's" in text and str(44 << 26) in text
    assert _status(ctx.order_mcmc_run, 1)[0] == STATE and ctx.info("device_bytes_live") <= live + (1 << 20)  # no chains, no table kept (the lists are)


def test_command_line(ctx, tmp_path):
    L = pooled_lists(30, 77, lambda v: 8 if v == 3 else 5, lambda v: 12, max_parents=3)
    names = [f"X{v}" for v in range(30)]
    text = "META pss_version = 0.1\nMETA input_file=none\nMETA num_records=100\n\n"
    for v in range(30):
        text += f"VAR {names[v]}\nMETA arity=2\n" + "".join(
            f"{x:f} " + "".join(names[u] + " " for u in range(30) if (int(S) >> u) & 1) + "\n" for S, x in zip(L.sets[v], L.sc[v])) + "\n"
    pss, dags = tmp_path / "n30.pss", tmp_path / "dags.txt"
    pss.write_text(text)
    _, offs, sets, scores = _read_pss(pss)
    args = ("--mcmc", "--chains", 8, "--burn", 50, "--thin", 5, "--sample", 40, "--seed", 3)
    r = _run(pss, *args, "--tables", "--table-picks", "-g", dags, "-o", os.devnull)
    assert r.returncode == 0, r.stderr
    ctx.order_mcmc_begin(offs, sets, scores, 8, seed=3, tables=True, table_picks=True)
    ctx.order_mcmc_run(50, 5, want_order=False, want_score=False, want_parents=False)
    got = ctx.order_mcmc_run(25, 5)
    more = 29 * 4 * 32 + 12 * 256
    assert r.stdout.splitlines()[0].endswith(f", tables (K_max = 8, {8 * (29 * 32 + 256)} bytes), table picks ({more} bytes more)")
    assert open(dags).read().splitlines() == _sample_lines(got, names, 40)
    r = _run(pss, *args, "--table-picks")
    assert r.returncode == 2 and "--table-picks" in r.stderr
