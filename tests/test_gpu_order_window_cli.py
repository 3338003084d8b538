"""bin/ordersearch --window on a small score file (tests/golden/order_window_n12.pss): the
re-optimised report is no worse than the plain one, and the network it writes is acyclic
along its order and scores under bin/calc_dag_score what the tool printed.  The score file
is generated, not data of the reference: order_search_ref.random_lists(12, 51, 16, 3)
written as a .pss (12 variables, up to 17 parent sets each, scores on a grid of 0.25)."""
import os
import re
import subprocess

import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so

from conftest import PKG

TOOL = os.path.join(PKG, "bin", "ordersearch")
CDS = os.path.join(PKG, "bin", "calc_dag_score")
PSS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "order_window_n12.pss")
N = 12


def _run(*more):
    # few, short searches: the plain run need not be at the optimum
    r = subprocess.run([TOOL, PSS, "--searches", "8", "--steps", "3", "--seed", "4", *more], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.gpu
def test_ordersearch_window_improves_and_writes_what_it_reports(tmp_path):
    plain = _run()
    assert len(plain) == 1
    net = tmp_path / "net"
    out = _run("--window", "6", "--rounds", "2", "-n", str(net))
    assert len(out) == 2
    score = lambda line: float(re.match(r"best score = (-?[\d.]+), ", line).group(1))  # noqa: E731
    m = re.fullmatch(r"window 6: (\d+) windows improved in (\d+) of 8 searches, best score before = (-?[\d.]+)", out[1])
    assert m and int(m.group(1)) >= int(m.group(2)) > 0
    assert score(out[0]) >= float(m.group(3)) and score(out[0]) >= score(plain[0])
    placed = set()  # acyclic along its order: every parent stands before its child
    for line in open(net).read().splitlines()[1:]:
        v, *parents = [int(x) for x in re.findall(r"\d+", line)]
        assert set(parents) <= placed, line
        placed.add(v)
    assert placed == set(range(1, N + 1))
    r = subprocess.run([CDS, PSS, str(net) + ".csv"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # both read the file's 6 decimals; calc_dag_score adds n float32 values (an ulp of 2^-24 relative each)
    # and both print 6 decimals (tests/test_gpu_order_search_cli.py)
    best = score(out[0])
    assert abs(abs(float(r.stdout.split()[1])) - abs(best)) <= N * 2.0 ** -24 * abs(best) + 1e-6, (r.stdout, best)
