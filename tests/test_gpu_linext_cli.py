"""bin/posterior --sample K --uniform [--uniform-edges FILE] on a .pss of `score --bge`: every
line's second field is the exact number of linear extensions of the DAG on that line, the rest of
the line and everything else the command prints is what it prints without --uniform, the ESS line
and the reweighted matrix are ulg.uniform_prior_edges of the same samples, and the misuse cases
exit 2."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so (tests/test_gpu_posterior.py)

import linext_ref as lx
import ulg
from conftest import GOLDEN, PKG
from test_gpu_posterior_cli import _read_pss
from test_gpu_posterior_sample_cli import _parse, _run

pytestmark = pytest.mark.gpu

SCORE = os.path.join(PKG, "bin", "score")


def test_uniform_reweighting_of_a_bge_pss(tmp_path):
    pss, dags, plain_dags, edges = tmp_path / "fig2.pss", tmp_path / "dags.txt", tmp_path / "plain.txt", tmp_path / "uni.csv"
    r = subprocess.run([SCORE, os.path.join(GOLDEN, "fig2_raw_data_5000.csv"), str(pss), "--bge"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    K = 300
    plain = _run(pss, "--sample", K, "--seed", 3, "-g", plain_dags)
    assert plain.returncode == 0, plain.stderr
    r = _run(pss, "--sample", K, "--seed", 3, "--uniform", "-g", dags, "--uniform-edges", edges)
    assert r.returncode == 0, r.stderr
    names, offs, sets, scores = _read_pss(pss)
    n = len(names)
    lines = open(dags).read().splitlines()
    assert len(lines) == K
    # the second field out: the file without --uniform, byte for byte
    stripped = "".join(" ".join(ln.split(" ")[:1] + ln.split(" ")[2:]) + "\n" for ln in lines)
    assert stripped == open(plain_dags).read()
    _, _, parents = _parse(stripped.splitlines(), names)
    counts = [ln.split(" ")[1] for ln in lines]
    want = [lx.count(n, [int(x) for x in row]) for row in parents]
    assert counts == [str(w) for w in want] and min(want) >= 1
    # standard output: one more line, right after ln Z
    out, base = r.stdout.splitlines(), plain.stdout.splitlines()
    assert out[0] == base[0] and out[2:] == base[1:] and out[1].startswith("uniform-prior ESS = ")
    ctx = ulg.Context(0)
    try:
        ext, le = ctx.dag_linear_extensions(parents)
    finally:
        ctx.close()
    assert ext == want
    edge, ess = ulg.uniform_prior_edges(parents, le)
    assert out[1] == f"uniform-prior ESS = {ess:.1f} of {K}"
    got = open(edges).read().splitlines()
    assert got == [",".join(f"{edge[u, v]:.6f}" for v in range(n)) for u in range(n)]
    # without -g the reweighted lines follow the rest of the output
    r2 = _run(pss, "--sample", K, "--seed", 3, "--uniform")
    assert r2.returncode == 0 and r2.stdout.splitlines() == out + lines
    assert max(want) <= math.factorial(n)


@pytest.mark.parametrize("args", [("--uniform",), ("--uniform-edges", "e.csv"), ("--uniform", "--uniform-edges", "e.csv"),
                                  ("--uniform", "--seed", "3"), ("--sample", "5", "--uniform-edges", "e.csv"),
                                  ("--sample", "5", "--uniform-edges")])
def test_bad_uniform_options_exit_2(tmp_path, args):
    """The command line is read before the .pss is opened: the file need not exist."""
    r = subprocess.run([os.path.join(PKG, "bin", "posterior"), str(tmp_path / "none.pss"), *args], capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.startswith("posterior: "), (args, r.stderr)
    assert not (tmp_path / "e.csv").exists()
