"""bin/posterior --mcmc --temper on the 30-variable .pss of tests/test_gpu_order_mcmc_cli.py: the status
line with its new fields, the sample lines and the Rao-Blackwellised matrix are those formatted from
Context.order_mc3_begin / order_mc3_run / order_edges on the lists the file holds; the misuse cases exit 2
without a GPU."""
import subprocess

import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import ulg
from test_gpu_order_edges_cli import _matrix_text
from test_gpu_order_mcmc_cli import N, POSTERIOR, _sample_lines, _write_pss
from test_gpu_posterior_cli import _read_pss
from test_gpu_posterior_sample_cli import _run


@pytest.mark.gpu
def test_tempered_samples_of_a_30_variable_pss(tmp_path):
    pss = tmp_path / "n30.pss"
    _write_pss(pss)
    names, offs, sets, scores = _read_pss(pss)
    dags, rbe = tmp_path / "dags.txt", tmp_path / "rb.csv"
    r = _run(pss, "--mcmc", "--temper", 3, "--swap-every", 4, "--chains", 8, "--burn", 50, "--thin", 5, "--sample", 40, "--seed", 3,
             "-g", dags, "--rb-edges", rbe, "-o", tmp_path / "edges.csv")
    assert r.returncode == 0, r.stderr
    ctx = ulg.Context(0)
    try:
        ctx.order_mc3_begin(offs, sets, scores, 8, ulg.geometric_betas(3, 0.1), swap_every=4, seed=3)
        ctx.order_mc3_run(50, 5, want_order=False, want_score=False, want_parents=False)
        got = ctx.order_mc3_run(25, 5)
        edge, zero = ctx.order_edges(got["order"].reshape(-1, N), groups=8)
    finally:
        ctx.close()
    tried = (75 // 4 // 2, (75 // 4 + 1) // 2)  # rounds 1 .. 18: pair 0 in the even ones, pair 1 in the odd ones
    swap = "/".join(f"{got['swaps'][:, p].sum() / (8 * tried[p]):.3f}" for p in range(2))
    line = r.stdout.splitlines()[0]
    assert line == (f"order MCMC: 8 chains, 75 steps each, acceptance = {got['accepted'][:, 0].sum() / (8 * 75):.3f}, "
                    f"R-hat(log score) = {ulg.order_rhat(got['log_score']):.3f}, 3 rungs, swap acceptance = {swap}")
    assert got["swaps"].sum() > 0 and open(dags).read().splitlines() == _sample_lines(got, names, 40)
    assert zero == 0 and open(rbe).read() == _matrix_text(ulg.order_edge_posterior(edge, [5] * 8)[0])


@pytest.mark.parametrize("args,message", [
    (("--sample", "5", "--temper", "3"), "--temper needs --mcmc"),
    (("--mcmc", "--sample", "5", "--beta-min", "0.5"), "need --temper"),
    (("--mcmc", "--sample", "5", "--swap-every", "5"), "need --temper"),
    (("--mcmc", "--sample", "5", "--temper", "1"), "--temper takes an integer 2..16, not '1'"),
    (("--mcmc", "--sample", "5", "--temper", "17"), "--temper takes an integer 2..16, not '17'"),
    (("--mcmc", "--sample", "5", "--temper", "x"), "--temper takes an integer 2..16, not 'x'"),
    (("--mcmc", "--sample", "5", "--temper", "2", "--beta-min", "1"), "--beta-min takes a number between 0 and 1, not '1'"),
    (("--mcmc", "--sample", "5", "--temper", "2", "--beta-min", "0"), "--beta-min takes a number between 0 and 1, not '0'"),
    (("--mcmc", "--sample", "5", "--temper", "2", "--beta-min", "nan"), "--beta-min takes a number between 0 and 1"),
    (("--mcmc", "--sample", "5", "--temper", "2", "--swap-every", "0"), "--swap-every takes an integer 1.."),
    (("--mcmc", "--sample", "5", "--temper", "4", "--chains", "262145"), "--chains x --temper is at most 1048576")])
def test_bad_temper_options_exit_2(tmp_path, args, message):
    r = subprocess.run([POSTERIOR, str(tmp_path / "none.pss"), *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.startswith("posterior: ") and message in r.stderr, (args, r.stderr)
