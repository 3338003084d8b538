"""bin/posterior --mcmc --partition on a .pss of 30 variables, where the exact path ends (plain
`posterior` exits 1): the status line, the sample lines and the edge matrix are those formatted from
Context.partition_mcmc_begin / partition_mcmc_run / dag_features; every sampled DAG is acyclic with stored
families; the refused flag combinations exit 2 without a GPU."""
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import ulg
from test_gpu_order_mcmc_cli import POSTERIOR, N, _matrix_text, _write_pss
from test_gpu_posterior_cli import _read_pss
from test_gpu_posterior_sample_cli import _parse, _run


@pytest.mark.gpu
def test_partition_samples_of_a_30_variable_pss(tmp_path):
    pss = tmp_path / "n30.pss"
    _write_pss(pss)
    names, offs, sets, scores = _read_pss(pss)
    assert _run(pss).returncode == 1
    dags, edges = tmp_path / "dags.txt", tmp_path / "edges.csv"
    r = _run(pss, "--mcmc", "--partition", "--chains", 8, "--burn", 50, "--thin", 5, "--sample", 64, "--seed", 3, "-g", dags, "-o", edges)
    assert r.returncode == 0, r.stderr
    ctx = ulg.Context(0)
    try:
        ctx.partition_mcmc_begin(offs, sets, scores, 8, seed=3)
        ctx.partition_mcmc_run(50, 5, want_part=False, want_score=False, want_parents=False)
        got = ctx.partition_mcmc_run(40, 5)  # to step 5 (50 // 5 + 8) = 90
        assert got["records"] == 8 and got["step"] == 90
        assert r.stdout.splitlines() == [
            f"partition MCMC: 8 chains, 90 steps each, acceptance = {got['accepted'].sum() / (8 * 90):.3f}, "
            f"mean parts = {got['parts'].mean():.3f}, R-hat(log score) = {ulg.order_rhat(got['log_score']):.3f}"]
        lines = open(dags).read().splitlines()
        order, parents = _parse(lines, names)[1:3]
        assert np.array_equal(parents, got["parents"].reshape(-1, N))
        part = got["part"].reshape(-1, N)
        stored = [set(int(S) for S in sets[offs[v]:offs[v + 1]]) for v in range(N)]
        for k in range(64):
            # the line's order is by part, ascending within a part, and every parent stands in an earlier part
            assert [int(v) for v in order[k]] == sorted(range(N), key=lambda v: (part[k, v], v))
            for v in range(N):
                assert int(parents[k, v]) in stored[v]
                assert all(part[k, u] < part[k, v] for u in range(N) if (int(parents[k, v]) >> u) & 1)
        f = ctx.dag_features(parents)
        assert f["total"] == 64 and f["cyclic"] == 0 and open(edges).read() == _matrix_text(f["edge"], 64)
    finally:
        ctx.close()


@pytest.mark.parametrize("args,message", [
    (("--partition", "--sample", "5"), "--partition needs --mcmc"),
    (("--mcmc", "--partition", "--sample", "5", "--uniform"), "already follow the uniform prior"),
    (("--mcmc", "--partition", "--sample", "5", "--uniform", "--uniform-edges", "f.txt"), "already follow the uniform prior"),
    (("--mcmc", "--partition", "--sample", "5", "--rb-edges", "f.txt"), "order-based"),
    (("--mcmc", "--partition", "--sample", "5", "--temper", "4"), "order-based")])
def test_refused_partition_options_exit_2(tmp_path, args, message):
    r = subprocess.run([POSTERIOR, str(tmp_path / "none.pss"), *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.startswith("posterior: ") and message in r.stderr, (args, r.stderr)
    assert not (tmp_path / "f.txt").exists()
