"""bin/posterior --sample K [--uniform] --paths / --blankets / --compelled / --vstructs FILE on a
.pss of `score --bge`: the four files are Context.dag_features of the samples the command prints,
divided by the total as doubles and formatted as the command formats them; with --uniform the
weights are ulg.uniform_prior_weights of the counts on the sample lines; everything else the
command prints or writes is what it prints and writes without the new flags; and the misuse cases
exit 2."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so (tests/test_gpu_posterior.py)

import ulg
from conftest import GOLDEN, PKG
from test_gpu_posterior_cli import _read_pss
from test_gpu_posterior_sample_cli import _parse, _run

pytestmark = pytest.mark.gpu

SCORE = os.path.join(PKG, "bin", "score")
FILES = (("--paths", "ancestor"), ("--blankets", "blanket"), ("--compelled", "compelled"), ("--vstructs", "vstruct"))


def _formatted(f, names):
    """name of dag_features' table -> the text of its file"""
    n, total = len(names), np.float64(f["total"])
    out = {k: "".join(",".join(f"{np.float64(f[k][u, v]) / total:.6f}" for v in range(n)) + "\n" for u in range(n))
           for k in ("ancestor", "blanket", "compelled")}
    out["vstruct"] = "".join(f"{names[u]} -> {names[v]} <- {names[w]} {np.float64(f['vstruct'][v, u, w]) / total:.6f}\n"
                             for v in range(n) for u in range(n) for w in range(u + 1, n) if f["vstruct"][v, u, w])
    return out


def test_feature_files_of_a_bge_pss(tmp_path):
    pss = tmp_path / "fig2.pss"
    r = subprocess.run([SCORE, os.path.join(GOLDEN, "fig2_raw_data_5000.csv"), str(pss), "--bge"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    names = _read_pss(pss)[0]
    K = 300
    ctx = ulg.Context(0)
    try:
        for tag, extra in (("plain", ()), ("uniform", ("--uniform",))):
            base_dags, dags = tmp_path / f"{tag}_base.txt", tmp_path / f"{tag}_dags.txt"
            base = _run(pss, "--sample", K, "--seed", 3, *extra, "-g", base_dags)
            assert base.returncode == 0, base.stderr
            paths = {flag: tmp_path / f"{tag}_{name}.txt" for flag, name in FILES}
            r = _run(pss, "--sample", K, "--seed", 3, *extra, "-g", dags, *[x for flag in paths for x in (flag, paths[flag])])
            assert r.returncode == 0, r.stderr
            # nothing the command printed or wrote before changes
            assert r.stdout == base.stdout and open(dags).read() == open(base_dags).read()
            lines = open(dags).read().splitlines()
            assert len(lines) == K
            if extra:
                stripped = [" ".join(ln.split(" ")[:1] + ln.split(" ")[2:]) for ln in lines]
            else:
                stripped = lines
            parents = _parse(stripped, names)[2]
            weight = None
            if extra:
                ext, le = ctx.dag_linear_extensions(parents)
                assert [str(x) for x in ext] == [ln.split(" ")[1] for ln in lines]
                weight = ulg.uniform_prior_weights(le)
                assert len(set(ext)) > 1, "every sample has the same count: the weights test nothing here"
            f = ctx.dag_features(parents, weight)
            assert f["cyclic"] == 0 and f["total"] == (K if weight is None else sum(int(x) for x in weight))
            want = _formatted(f, names)
            for flag, name in FILES:
                assert open(paths[flag]).read() == want[name], (tag, flag)
            assert want["ancestor"].count("\n") == len(names) and float(want["ancestor"].split(",")[0]) == 0.0
            # one file alone: the same text
            alone = tmp_path / f"{tag}_alone.txt"
            r = _run(pss, "--sample", K, "--seed", 3, *extra, "-g", dags, "--compelled", alone)
            assert r.returncode == 0 and open(alone).read() == want["compelled"] and r.stdout == base.stdout
    finally:
        ctx.close()
    # compelled never exceeds edge-by-path: p(u -> v compelled) <= p(u ~> v)
    cmp_ = np.array([[float(x) for x in ln.split(",")] for ln in want["compelled"].splitlines()])
    anc = np.array([[float(x) for x in ln.split(",")] for ln in want["ancestor"].splitlines()])
    assert np.all(cmp_ <= anc) and anc.max() > 0.0


@pytest.mark.parametrize("args", [("--paths", "f.csv"), ("--blankets", "f.csv"), ("--compelled", "f.csv"), ("--vstructs", "f.csv"),
                                  ("--uniform", "--paths", "f.csv"), ("--seed", "3", "--compelled", "f.csv"),
                                  ("--sample", "5", "--paths"), ("--sample", "0", "--paths", "f.csv")])
def test_bad_feature_options_exit_2(tmp_path, args):
    """The command line is read before the .pss is opened: the file need not exist."""
    r = subprocess.run([os.path.join(PKG, "bin", "posterior"), str(tmp_path / "none.pss"), *args], capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.startswith("posterior: "), (args, r.stderr)
    assert not (tmp_path / "f.csv").exists()
