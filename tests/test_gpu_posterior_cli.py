"""bin/posterior on a .pss of `score --bge`: the printed edge matrix equals the
sum over all orderings (tests/posterior_ref.py brute) on the file's printed
scores to the six printed decimals, and the option errors follow the other
command lines."""
import os
import subprocess

import numpy as np
import pytest

import posterior_ref as pr
from conftest import GOLDEN, PKG

SCORE = os.path.join(PKG, "bin", "score")
POSTERIOR = os.path.join(PKG, "bin", "posterior")


def _read_pss(path):
    """-> (names, offsets, sets, scores) with scores = float32 of the printed text, as read_pss takes them."""
    names, blocks = [], []
    for ln in open(path).read().splitlines():
        if ln.startswith("VAR "):
            names.append(ln[4:].strip())
            blocks.append([])
        elif blocks and ln.strip() and not ln.startswith("META"):
            tok = ln.split()
            blocks[-1].append((tok[0], tok[1:]))
    index = {nm: i for i, nm in enumerate(names)}
    offs, sets, scores = [0], [], []
    for b in blocks:
        for text, parents in b:
            sets.append(sum(1 << index[p] for p in parents))
            scores.append(np.float32(float(text)))
        offs.append(len(sets))
    return names, np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32)


@pytest.mark.gpu
def test_posterior_of_a_bge_pss(tmp_path):
    pss, edges, sets_txt = tmp_path / "fig2.pss", tmp_path / "edges.csv", tmp_path / "sets.txt"
    r = subprocess.run([SCORE, os.path.join(GOLDEN, "fig2_raw_data_5000.csv"), str(pss), "--bge"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([POSTERIOR, str(pss), "-o", str(edges), "-s", str(sets_txt)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    names, offs, sets, scores = _read_pss(pss)
    n = len(names)
    assert 2 <= n <= 7 and len(sets) == offs[-1] > n
    want = pr.brute(n, offs, sets, scores)
    ref = pr.reference("cli-fig2", n, offs, sets, scores)
    cap = ref["cap"]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("ln Z = ")
    assert abs(float(lines[0][7:]) - float(want["log_z"])) <= 0.5e-10 + cap
    rows = open(edges).read().splitlines()
    assert len(rows) == n and all(len(row.split(",")) == n and all(len(x.split(".")[1]) == 6 for x in row.split(","))
                                  for row in rows)
    got = np.array([[float(x) for x in row.split(",")] for row in rows])
    worst = float(np.abs(got - want["edge"].astype(np.float64)).max())
    print(f"posterior-observed cli fig2 max {worst:.3g} cap {0.5e-6 + cap:.3g} e64 {ref['e64']:.3g}")
    assert worst <= 0.5e-6 + cap  # the six printed decimals
    assert np.all(np.diag(got) == 0) and got.max() > 0.5
    # one line per stored set, in the file's order: "<name>: <posterior> <parents ...>"
    out = open(sets_txt).read().splitlines()
    assert len(out) == len(sets)
    p = np.exp(want["set_logpost"].astype(np.float64))
    for i, ln in enumerate(out):
        v = int(np.searchsorted(offs, i, side="right") - 1)
        head, _, rest = ln.partition(": ")
        tok = rest.split()
        assert head == names[v] and tok[1:] == [names[u] for u in range(n) if (int(sets[i]) >> u) & 1]
        assert abs(float(tok[0]) - p[i]) <= 0.5e-6 + cap
    # without -o the matrix follows the ln Z line
    r2 = subprocess.run([POSTERIOR, str(pss)], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout.splitlines() == [lines[0]] + rows


def test_option_errors(tmp_path):
    """Needs no GPU: the command line is read, and the .pss opened, before the device is."""
    r = subprocess.run([POSTERIOR], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage" in r.stdout
    r = subprocess.run([POSTERIOR, "--no-such-option"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "unrecognised option" in r.stderr
    r = subprocess.run([POSTERIOR, "a.pss", "-o"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "missing" in r.stderr
    r = subprocess.run([POSTERIOR, str(tmp_path / "missing.pss")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr.startswith("posterior: ")
