"""CPU tests of the order search's restatement (tests/order_search_ref.py) and of
its arithmetic on the host (bin/order_search_check, plain and under ASan + UBSan).

The events -- an aspiration move, a non-improving move, a kick, an undone kick,
a step without an admissible swap -- are asked of the GPU tests' inputs taken
together: the input with tenure 0 can have no tabu swap, so no single input
could be asked for all of them on every input; n5 alone does meet all five."""
import os
import subprocess

import numpy as np
import pytest

import order_search_ref as osr

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "urlearning-cpp_amd")
STEPS = 150  # the GPU tests compare these


@pytest.mark.parametrize("path", ["bin/order_search_check", "bin/san/order_search_check"])
def test_order_search_check(path):
    if not os.path.exists(os.path.join(PKG, path)):
        subprocess.run(["make", "-C", PKG, path], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(PKG, path)], capture_output=True, text=True)
    assert r.returncode == 0 and "order_search_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_cached_gains_equal_a_recompute_and_every_event_is_met():
    met = {}
    for name, (L, seed, tenure, patience) in osr.inputs().items():
        searches = [osr.Search(L, seed, c, tenure, patience) for c in range(4)]
        for s in searches:
            for _ in range(STEPS):
                s.step()
                assert np.array_equal(np.array(s.gains()), np.array(s.fresh_gains())), (name, s.c, s.t)
                assert np.array_equal(s.term, osr.order_best(L, s.order)[0])
        met[name] = set().union(*(s.events for s in searches))
    assert met["n5"] == {"aspiration", "nonimproving", "kick", "undone", "stuck"}, met
    assert all({"nonimproving", "kick"} <= ev for ev in met.values()), met


def optimum(L):
    """The best network's score by the subset DP: opt(W) = max over the sink v of W of opt(W - v) + b_v(W - v)."""
    n, LD = L.n, np.longdouble
    opt = [LD(0)] + [LD(-np.inf)] * ((1 << n) - 1)
    for W in range(1, 1 << n):
        for v in range(n):
            if (W >> v) & 1:
                rest = W & ~(1 << v)
                opt[W] = max(opt[W], opt[rest] + LD(osr.best(L, v, rest)[0]))
    return opt[-1]


def test_reachability_input_reaches_the_optimum():
    L, seed, tenure, patience = osr.inputs()["n8"]
    out = osr.run([osr.Search(L, seed, c, tenure, patience) for c in range(64)], STEPS)
    assert np.longdouble(out["best_score"].max()) == optimum(L)
