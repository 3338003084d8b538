"""bin/posterior --mcmc on a .pss of 30 variables, where the exact path ends (plain `posterior` exits 1):
the line that stands for ln Z, the sample lines, the edge matrix and a feature file are those formatted
from Context.order_mcmc_begin / order_mcmc_run / dag_features and ulg.order_rhat on the lists the file
holds; and the misuse cases exit 2 without a GPU."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so (tests/test_gpu_posterior.py)

import order_mcmc_ref as om
import ulg
from conftest import PKG
from test_gpu_posterior_cli import _read_pss
from test_gpu_posterior_sample_cli import _parse, _run

POSTERIOR = os.path.join(PKG, "bin", "posterior")
N = 30


def _write_pss(path):
    L = om.make_lists(N, 3030, max_parents=3, per_var=20)
    names = [f"X{v}" for v in range(N)]
    text = "META pss_version = 0.1\nMETA input_file=none\nMETA num_records=100\n\n"
    for v in range(N):
        text += f"VAR {names[v]}\nMETA arity=2\n"
        for S, x in zip(L.sets[v], L.sc[v]):
            text += f"{x:f} " + "".join(names[u] + " " for u in range(N) if (int(S) >> u) & 1) + "\n"
        text += "\n"
    path.write_text(text)


def _matrix_text(table, total):
    n = table.shape[0]
    return "".join(",".join(f"{np.float64(table[u, v]) / np.float64(total):.6f}" for v in range(n)) + "\n" for u in range(n))


def _sample_lines(r, names, K):
    n = len(names)
    order, par, lw = r["order"].reshape(-1, n), r["parents"].reshape(-1, n), r["log_weight"].reshape(-1)
    lines = []
    for k in range(K):
        tok = [f"{lw[k]:.6f}"]
        for v in order[k]:
            tok.append(names[v] + "<-" + ",".join(names[u] for u in range(n) if (int(par[k, v]) >> u) & 1))
        lines.append(" ".join(tok))
    return lines


@pytest.mark.gpu
def test_mcmc_samples_of_a_30_variable_pss(tmp_path):
    pss = tmp_path / "n30.pss"
    _write_pss(pss)
    names, offs, sets, scores = _read_pss(pss)
    assert len(names) == N and offs[-1] == 20 * N
    plain = _run(pss)
    assert plain.returncode == 1 and "at most 28 variables" in plain.stderr
    ctx = ulg.Context(0)
    try:
        for K in (40, 37):  # 5 records of 8 chains; the first 37 of them
            dags, edges, paths = tmp_path / f"dags{K}.txt", tmp_path / f"edges{K}.csv", tmp_path / f"paths{K}.csv"
            r = _run(pss, "--mcmc", "--chains", 8, "--burn", 50, "--thin", 5, "--sample", K, "--seed", 3, "-g", dags, "-o", edges,
                     "--paths", paths)
            assert r.returncode == 0, r.stderr
            ctx.order_mcmc_begin(offs, sets, scores, 8, seed=3)
            ctx.order_mcmc_run(50, 5, want_order=False, want_score=False, want_parents=False)
            got = ctx.order_mcmc_run(25, 5)  # to step 5 (50 // 5 + 5) = 75
            assert got["records"] == 5 and got["step"] == 75
            rhat = ulg.order_rhat(got["log_score"])
            want_line = (f"order MCMC: 8 chains, 75 steps each, acceptance = {got['accepted'].sum() / (8 * 75):.3f}, "
                         f"R-hat(log score) = {rhat:.3f}")
            assert r.stdout.splitlines() == [want_line] and "ln Z" not in r.stdout
            lines = open(dags).read().splitlines()
            assert lines == _sample_lines(got, names, K)
            parents = got["parents"].reshape(-1, N)[:K]
            assert np.array_equal(_parse(lines, names)[2], parents)
            f = ctx.dag_features(parents)
            assert f["total"] == K and f["cyclic"] == 0
            assert open(edges).read() == _matrix_text(f["edge"], K) and open(paths).read() == _matrix_text(f["ancestor"], K)
        # without -o the matrix follows the first line, the samples come last; one record per chain: R-hat n/a
        r = _run(pss, "--mcmc", "--chains", 8, "--burn", 50, "--thin", 5, "--sample", 8, "--seed", 3)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        assert len(out) == 1 + N + 8 and out[0].startswith("order MCMC: 8 chains, 55 steps each") and out[0].endswith("= n/a")
        # --uniform keeps the linear-extension count's own limit
        r = _run(pss, "--mcmc", "--chains", 8, "--burn", 5, "--thin", 5, "--sample", 8, "--uniform")
        assert r.returncode == 1 and "28" in r.stderr
    finally:
        ctx.close()


@pytest.mark.parametrize("args,message", [
    (("--mcmc",), "--mcmc needs --sample"),
    (("--mcmc", "--seed", "3"), "need --sample"),
    (("--chains", "4"), "need --mcmc"),
    (("--burn", "10", "--sample", "5"), "need --mcmc"),
    (("--thin", "2", "--sample", "5"), "need --mcmc"),
    (("--mcmc", "--sample", "5", "-s", "f.txt"), "does not go with -s"),
    (("--mcmc", "--sample", "5", "--chains", "0"), "--chains takes an integer 1..1048576, not '0'"),
    (("--mcmc", "--sample", "5", "--chains", "1048577"), "--chains takes an integer 1..1048576, not '1048577'"),
    (("--mcmc", "--sample", "5", "--chains", "x"), "--chains takes an integer 1..1048576, not 'x'"),
    (("--mcmc", "--sample", "5", "--thin", "0"), "--thin takes an integer 1..1099511627776, not '0'"),
    (("--mcmc", "--sample", "5", "--burn", "-1"), "--burn takes an integer 0..1099511627776, not '-1'"),
    (("--mcmc", "--sample", "9223372036854775807", "--chains", "1", "--thin", "2"), "pass 2^62 steps"),
    (("--mcmc", "--sample", "4194304", "--chains", "1", "--thin", "1099511627776", "--burn", "1099511627776"), "pass 2^62 steps")])
def test_bad_mcmc_options_exit_2(tmp_path, args, message):
    """The command line is read before the .pss is opened: the file need not exist, nor a GPU.  Each case is
    refused by the check that is there for it, which its message shows (an unknown option exits 2 as well)."""
    r = subprocess.run([POSTERIOR, str(tmp_path / "none.pss"), *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.startswith("posterior: ") and message in r.stderr, (args, r.stderr)
    assert not (tmp_path / "f.txt").exists()


def test_help_names_the_mcmc_options():
    r = subprocess.run([POSTERIOR, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(x in r.stdout for x in ("--mcmc", "--chains", "--burn", "--thin", "mean edge frequencies"))
