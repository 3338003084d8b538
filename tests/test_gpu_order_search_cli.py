"""bin/ordersearch on a small generated .pss (n = 8, the reachability input's lists): the
network it writes is acyclic, scores under bin/calc_dag_score what the tool printed, and a
seed gives the same bytes twice."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

import order_search_ref as osr
from conftest import PKG

TOOL = os.path.join(PKG, "bin", "ordersearch")
CDS = os.path.join(PKG, "bin", "calc_dag_score")


def _run(pss, net, seed):
    r = subprocess.run([TOOL, str(pss), "-n", str(net), "--searches", "16", "--steps", "100", "--seed", str(seed)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout, open(net).read(), open(str(net) + ".csv").read()


@pytest.mark.gpu
def test_ordersearch_writes_the_network_it_reports(tmp_path):
    L = osr.inputs()["n8"][0]
    n, names = L.n, [f"X{v}" for v in range(L.n)]
    text = "META pss_version = 0.1\nMETA input_file=none\nMETA num_records=100\n\n"
    for v in range(n):
        text += f"VAR {names[v]}\nMETA arity=2\n"
        for S, x in zip(L.sets[v], L.sc[v]):
            text += f"{x:f} " + "".join(names[u] + " " for u in range(n) if (int(S) >> u) & 1) + "\n"
        text += "\n"
    pss = tmp_path / "n8.pss"
    pss.write_text(text)
    out, net, csv = _run(pss, tmp_path / "net", 7)
    assert (out, net, csv) == _run(pss, tmp_path / "again", 7)
    m = re.fullmatch(r"best score = (-?[\d.]+), search (\d+), (\d+) of 16 searches share it, (\d+) moves, (\d+) kicks\n", out)
    assert m and 1 <= int(m.group(3)) <= 16 and int(m.group(4)) > 0
    A = np.array([[int(x) for x in row.split(",")] for row in csv.splitlines()])  # row v, column u: u -> v
    assert A.shape == (n, n)
    left = list(range(n))
    while left:  # acyclic: a variable whose parents are all placed can always be taken
        free = [v for v in left if not any(A[v, u] for u in left)]
        assert free, "a cycle"
        left = [v for v in left if v not in free]
    r = subprocess.run([CDS, str(pss), str(tmp_path / "net.csv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    scored = float(r.stdout.split()[1])
    # both read the file's 6 decimals; calc_dag_score adds n float32 values (an ulp of 2^-24 relative each)
    # and both print 6 decimals
    best = float(m.group(1))
    assert abs(abs(scored) - abs(best)) <= n * 2.0 ** -24 * abs(best) + 1e-6, (scored, best)
