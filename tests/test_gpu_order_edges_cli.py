"""bin/posterior --mcmc --rb-edges on a .pss of 30 variables: the file is the matrix of
ulg.order_edge_posterior over Context.order_edges of the very orders the run recorded, for the same seed,
chains, burn and thin, to -o's printed precision; the line after the order MCMC line names the orders and
the largest standard error across chains; -o's file is byte-identical with and without it; the misuse
cases exit 2 without a GPU."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so (tests/test_gpu_posterior.py)

import ulg
from conftest import PKG
from test_gpu_order_mcmc_cli import N, _write_pss
from test_gpu_posterior_cli import _read_pss
from test_gpu_posterior_sample_cli import _run

POSTERIOR = os.path.join(PKG, "bin", "posterior")


def _matrix_text(m):
    return "".join(",".join(f"{x:.6f}" for x in row) + "\n" for row in m)


@pytest.mark.gpu
def test_rb_edges_of_a_30_variable_pss(tmp_path):
    pss = tmp_path / "n30.pss"
    _write_pss(pss)
    names, offs, sets, scores = _read_pss(pss)
    ctx = ulg.Context(0)
    try:
        for K, chains in ((37, 8), (5, 8), (12, 1)):  # a part of the last record; fewer orders than chains; one chain
            rbf, edges, plain = tmp_path / f"rb{K}.csv", tmp_path / f"edges{K}.csv", tmp_path / f"plain{K}.csv"
            common = ("--mcmc", "--chains", chains, "--burn", 50, "--thin", 5, "--sample", K, "--seed", 3, "-g", tmp_path / "dags.txt")
            r = _run(pss, *common, "-o", edges, "--rb-edges", rbf)
            assert r.returncode == 0, r.stderr
            if K == 37:  # -o's file and the first line do not know of --rb-edges
                r0 = _run(pss, *common, "-o", plain)
                assert r0.returncode == 0, r0.stderr
                assert open(edges, "rb").read() == open(plain, "rb").read() and r.stdout.splitlines()[:1] == r0.stdout.splitlines()
            recs = -(-K // chains)
            ctx.order_mcmc_begin(offs, sets, scores, chains, seed=3)
            ctx.order_mcmc_run(50, 5, want_order=False, want_score=False, want_parents=False)
            got = ctx.order_mcmc_run(5 * recs, 5, want_parents=False)
            assert got["records"] == recs
            orders = got["order"].reshape(-1, N)[:K]
            groups = chains if chains >= 2 and K >= chains else 1
            tab, zero = ctx.order_edges(orders, groups=groups)
            assert zero == 0
            out = r.stdout.splitlines()
            assert len(out) == 2 and out[0].startswith(f"order MCMC: {chains} chains, ")
            if groups >= 2:
                mean, se = ulg.order_edge_posterior(tab, [len(range(g, K, groups)) for g in range(groups)])
                tail = f"largest standard error = {se.max():.6f}"
            else:
                mean, tail = ulg.order_edge_posterior(tab, K), "standard error not computed"
            assert out[1] == f"Rao-Blackwell edges: {K} orders, 0 of probability 0, {tail}"
            assert open(rbf).read() == _matrix_text(mean)
            assert open(rbf).read() != open(edges).read()  # not the sample mean
    finally:
        ctx.close()


@pytest.mark.parametrize("args,message", [
    (("--rb-edges", "f.csv"), "--rb-edges needs --mcmc"),
    (("--sample", "5", "--rb-edges", "f.csv"), "--rb-edges needs --mcmc"),
    (("--mcmc", "--rb-edges", "f.csv"), "--mcmc needs --sample"),
    (("--mcmc", "--sample", "4194305", "--rb-edges", "f.csv"), "--rb-edges takes at most 4194304 samples")])
def test_bad_rb_edges_options_exit_2(tmp_path, args, message):
    """The command line is read before the .pss is opened: the file need not exist, nor a GPU."""
    r = subprocess.run([POSTERIOR, str(tmp_path / "none.pss"), *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.startswith("posterior: ") and message in r.stderr, (args, r.stderr)
    assert not (tmp_path / "f.csv").exists()


def test_help_names_rb_edges():
    r = subprocess.run([POSTERIOR, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--rb-edges" in r.stdout and "Rao-Blackwellised" in r.stdout
