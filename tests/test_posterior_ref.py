"""The references of the exact model averaging (tests/posterior_ref.py) against
each other, and the host arithmetic of csrc/posterior_dev.h (bin/posterior_check).

The lattice recursion in longdouble is held to the sum over all n! orderings at
n = 1 .. 7 -- dense lists, sparse lists, lists that lack the empty set, a
variable whose only set is the empty one, a variable with no list -- within
256 longdouble roundings at the tables' magnitude.  It is the reference of
tests/test_gpu_posterior.py; the float64 recursion with the kernels' cut gives
e64, what float64 itself loses on each input, and with it the GPU tests' cap
8 max(e64, 2^-52 (1 + M)).
"""
import os
import subprocess

import numpy as np
import pytest

import posterior_ref as pr
from conftest import PKG

CHECK = os.path.join(PKG, "bin", "posterior_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "posterior_check")
LD_EPS = float(np.finfo(np.longdouble).eps)

BRUTE = [(n, kind) for n in range(1, 8) for kind in pr.BRUTE_KINDS]


def _magnitude(r):
    vals = np.concatenate([r[k][np.isfinite(r[k])].ravel() for k in ("alpha", "f", "b", "gamma")])
    return float(np.abs(vals).max()) if vals.size else 0.0


@pytest.mark.skipif(LD_EPS > 2e-19, reason="np.longdouble is not the 80-bit type here")
@pytest.mark.parametrize("n,kind", BRUTE)
def test_lattice_in_longdouble_equals_the_sum_over_all_orderings(n, kind):
    name = f"brute-{kind}-{n}"
    _, offs, sets, scores = pr.gpu_inputs()[name]
    a = pr.brute(n, offs, sets, scores)
    b = pr.reference(name, n, offs, sets, scores)["ld"]
    tol = 256 * LD_EPS * (1.0 + _magnitude(b))
    if kind == "nolist":
        assert a["log_z"] == -np.inf and b["log_z"] == -np.inf
        assert np.all(b["set_logpost"] == -np.inf) and np.all(b["edge"] == 0)
        return
    assert np.isfinite(a["log_z"])
    fin = np.isfinite(a["set_logpost"])
    assert np.array_equal(fin, np.isfinite(b["set_logpost"]))
    d = max(float(abs(a["log_z"] - b["log_z"])), float(np.abs(a["set_logpost"][fin] - b["set_logpost"][fin]).max()))
    de = float(np.abs(a["edge"] - b["edge"]).max())
    print(f"{name}: {len(sets)} sets, ln Z {float(b['log_z']):.6f}, log-domain deviation {d:.3g}, edges {de:.3g}, tol {tol:.3g}")
    assert d <= tol and de <= tol
    if kind == "solo":  # the only set of the last variable: certain, and no edge into it
        assert b["set_logpost"][-1] == 0.0 and np.all(b["edge"][:, n - 1] == 0)


@pytest.mark.parametrize("name", sorted(pr.gpu_inputs()))
def test_invariants_and_e64_on_every_gpu_input(name):
    """b(V) = f(V); sum_S g_v(S) alpha_v(S) = Z for every v (as L_v, the sum of w gamma over the stored
    sets); each variable's posteriors sum to 1; edges are the sums of their sets.  Prints e64 and the cap."""
    n, offs, sets, scores = pr.gpu_inputs()[name]
    r = pr.reference(name, n, offs, sets, scores)
    ld, e64, M, cap = r["ld"], r["e64"], r["M"], r["cap"]
    print(f"{name}: n {n}, {len(sets)} sets, M {M:.6g}, e64 {e64:.3g}, cap {cap:.3g}")
    tol = 256 * LD_EPS * (1.0 + M) if LD_EPS < 2e-19 else cap
    allv = (1 << n) - 1
    lz = ld["log_z"]
    if lz == -np.inf:
        assert ld["b"][allv] == -np.inf and np.all(ld["L"] == -np.inf) and np.all(ld["edge"] == 0)
        return
    assert abs(ld["b"][allv] - lz) <= tol
    assert float(np.abs(ld["L"] - lz).max()) <= tol
    for v in range(n):
        sl = slice(offs[v], offs[v + 1])
        p = np.exp(ld["set_logpost"][sl])
        assert abs(p.sum() - 1) <= tol  # t - L_v carries the roundings of values of magnitude M
        for u in range(n):
            has = ((sets[sl].astype(np.int64) >> u) & 1) == 1
            assert abs(p[has].sum() - ld["edge"][u, v]) <= tol
    # what float64 loses stays near its rounding unit at the tables' magnitude: the cap means something
    assert e64 <= 64 * 2.0 ** -52 * (1.0 + M)
    f64 = r["f64"]
    assert np.array_equal(np.isfinite(f64["set_logpost"]), np.isfinite(ld["set_logpost"]))


def test_the_cut_is_met_from_both_sides_in_the_dynamic_inputs():
    for name in ("dynamic-6", "dynamic-9"):
        n, offs, sets, scores = pr.gpu_inputs()[name]
        assert float(np.abs(scores).max()) > 1e4
        below = above = 0
        for v in range(n):
            s = np.sort(scores[offs[v]:offs[v + 1]].astype(np.float64))
            gaps = np.abs(s[:, None] - s[None, :])
            below += int(((gaps > 36.5) & (gaps <= pr.CUT)).sum())
            above += int(((gaps > pr.CUT) & (gaps < 39.5)).sum())
        assert below > 0 and above > 0, (name, below, above)
        # ... and the recursion itself meets such operands: logaddexp counts them
        pr.NEAR_CUT = [0, 0]
        try:
            pr.lattice(n, offs, sets, scores, dtype=np.float64, cut=pr.CUT, tables=False)
            within, beyond = pr.NEAR_CUT
        finally:
            pr.NEAR_CUT = None
        print(f"{name}: logaddexp operand gaps within 1.5 nats below the cut {within}, above it {beyond}")
        assert within > 0 and beyond > 0, (name, within, beyond)
        # a linear-space sum of these weights overflows or vanishes
        with np.errstate(over="ignore", under="ignore"):
            w = np.exp(scores.astype(np.float64))
        assert np.all((w == 0) | np.isinf(w))


def test_posterior_check():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "posterior_check ok" in r.stdout, (r.stdout, r.stderr)


def test_posterior_check_under_sanitizers():
    if not os.path.exists(SAN_CHECK):
        subprocess.run(["make", "-C", PKG, "bin/san/posterior_check"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([SAN_CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "posterior_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
