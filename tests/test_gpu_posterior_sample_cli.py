"""bin/posterior --sample on a .pss of `score --bge`: the lines parse, they are
the samples Context.posterior_sample draws from the same lists, everything the
command printed before is printed as before, and the option errors exit 2."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so (tests/test_gpu_posterior.py)

import ulg
from conftest import GOLDEN, PKG
from test_gpu_posterior_cli import _read_pss

pytestmark = pytest.mark.gpu

SCORE = os.path.join(PKG, "bin", "score")
POSTERIOR = os.path.join(PKG, "bin", "posterior")


def _run(*args):
    return subprocess.run([POSTERIOR, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def _parse(lines, names):
    """-> (log weights as printed, order (K, n), parents (K, n))."""
    index = {nm: i for i, nm in enumerate(names)}
    n = len(names)
    text, order, parents = [], [], []
    for ln in lines:
        tok = ln.split(" ")
        assert len(tok) == n + 1 and len(tok[0].split(".")[1]) == 6, ln
        text.append(tok[0])
        o, p = [], [0] * n
        for t in tok[1:]:
            child, arrow, pa = t.partition("<-")
            assert arrow == "<-" and child in index, ln
            o.append(index[child])
            p[index[child]] = sum(1 << index[x] for x in pa.split(",")) if pa else 0
        order.append(o)
        parents.append(p)
    return text, np.array(order), np.array(parents, dtype=np.uint64)


def test_samples_of_a_bge_pss(tmp_path):
    pss, dags = tmp_path / "fig2.pss", tmp_path / "dags.txt"
    r = subprocess.run([SCORE, os.path.join(GOLDEN, "fig2_raw_data_5000.csv"), str(pss), "--bge"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = _run(pss)
    assert plain.returncode == 0, plain.stderr
    r = _run(pss, "--sample", 50, "--seed", 7, "-g", dags)
    assert r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout  # ln Z and the edge matrix, byte for byte
    names, offs, sets, scores = _read_pss(pss)
    n = len(names)
    lines = open(dags).read().splitlines()
    assert len(lines) == 50
    text, order, parents = _parse(lines, names)
    ctx = ulg.Context(0)
    try:
        ctx.posterior(offs, sets, scores)
        want = ctx.posterior_sample(50, seed=7)
        other = ctx.posterior_sample(50, seed=8)
    finally:
        ctx.close()
    assert np.array_equal(order, want[1]) and np.array_equal(parents, want[0])
    assert text == [f"{w:.6f}" for w in want[2]]
    assert np.all(np.sort(order, axis=1) == np.arange(n))
    assert not np.array_equal(other[0], want[0])  # the seed matters
    # without -g the lines follow the existing output; without --seed the seed is 0
    r2 = _run(pss, "--sample", 50, "--seed", 7)
    assert r2.returncode == 0 and r2.stdout.splitlines() == plain.stdout.splitlines() + lines
    r3, r4 = _run(pss, "--sample=3"), _run(pss, "--sample", 3, "--seed", 0)
    assert r3.returncode == 0 and r3.stdout == r4.stdout and len(r3.stdout.splitlines()) == len(plain.stdout.splitlines()) + 3


@pytest.mark.parametrize("args", [("--seed", "3"), ("-g", "dags.txt"), ("--seed", "3", "-g", "dags.txt"), ("--sample", "0"),
                                  ("--sample", "-3"), ("--sample", "2.5"), ("--sample", "many"), ("--sample", ""),
                                  ("--sample", "3", "--seed", "-1"), ("--sample", "3", "--seed", "x"), ("--sample",)])
def test_bad_sampling_options_exit_2(tmp_path, args):
    """The command line is read before the .pss is opened: the file need not exist."""
    r = _run(tmp_path / "none.pss", *args)
    assert r.returncode == 2 and r.stderr.startswith("posterior: "), (args, r.stderr)
    assert not (tmp_path / "dags.txt").exists()
