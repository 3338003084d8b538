"""CPU tests of the window re-optimisation's restatement (tests/order_window_ref.py) and of
its arithmetic on the host (bin/order_window_check, plain and under ASan + UBSan): a window
as wide as the order is the exact optimum, S never falls, and the GPU tests' cases meet
every event the contract names."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import order_search_ref as osr
import order_window_ref as owr
from test_order_search_ref import PKG, optimum


@pytest.mark.parametrize("path", ["bin/order_window_check", "bin/san/order_window_check"])
def test_order_window_check(path):
    if not os.path.exists(os.path.join(PKG, path)):
        subprocess.run(["make", "-C", PKG, path], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(PKG, path)], capture_output=True, text=True)
    assert r.returncode == 0 and "order_window_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_window_as_wide_as_the_order_is_the_optimum():
    L = osr.inputs()["n5"][0]
    top = max(owr.F64(0.0) + sum(osr.order_best(L, o)[0]) for o in itertools.permutations(range(5)))  # sum(): ascending
    assert np.isfinite(top)
    for order in owr.case_orders("n5"):  # the last one starts at -inf
        got, terms, S, _, accepted, _ = owr.run(L, order, 5, 1, 4)
        assert S == top and accepted <= 1 and np.array_equal(terms, osr.order_best(L, got)[0])
    L = osr.inputs()["n8"][0]
    want = optimum(L)
    for order in owr.case_orders("n8"):
        assert np.longdouble(owr.run(L, order, 8, 4, 4)[2]) == want


def test_score_never_falls_and_every_event_is_met():
    met = set()
    for name, width, stride, max_sweeps in owr.CASES:
        for order in owr.case_orders(name):
            trace = []
            owr.run(osr.inputs()[name][0], order, width, stride, max_sweeps, met, trace)
            assert all(a <= b for a, b in zip(trace, trace[1:])), (name, width, order)
    assert met == {"accepted", "rejected", "repaired", "clamped", "converged", "capped"}, met
