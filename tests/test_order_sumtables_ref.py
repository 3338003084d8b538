"""tests/order_sumtables_ref.py against itself, without a GPU: the float64 butterfly meets the slot cap
against the long-double sum on the GPU tests' inputs, -inf stands exactly where no entry is compatible, and
no step or pick of the GPU chain tests' seeds comes within its slack of deciding otherwise for any table
inside the cap -- so tests/test_gpu_order_sumtables.py may demand equality."""
import numpy as np
import pytest

import order_sumtables_ref as st
from test_gpu_order_tables import READBACK_K, readback_lists


def _check_tables(L, variables):
    worst = 0.0
    for v in variables:
        (C, T), (want, count, cap) = st.butterfly(L, v), st.direct(L, v)
        assert C == int(np.bitwise_or.reduce(L.sets[v])) and len(T) == len(want)
        assert np.array_equal(T == -np.inf, count == 0) and not np.isnan(T).any()
        assert np.array_equal(T[count == 1], want[count == 1].astype(np.float64))
        some = count > 1
        err = np.abs(T[some].astype(np.longdouble) - want[some]).astype(np.float64)
        assert np.all(err <= cap[some]), (v, float((err / cap[some]).max()))
        worst = max(worst, float((err / cap[some]).max(initial=0.0)))
    return worst


def test_butterfly_meets_the_cap_on_the_readback_lists():
    L = readback_lists()
    worst = _check_tables(L, sorted(READBACK_K))
    assert st.butterfly(L, 7)[1][0] == -np.inf and st.butterfly(L, 0)[1].tolist() == [L.sc[0][0]]  # no empty set; K = 0
    print(f"float64 butterfly: the largest error is {worst:.3f} of its cap")


@pytest.mark.parametrize("n", [5, 8, 33, 63])
def test_no_undecided_step_in_the_chain_inputs(n):
    L, seed = st.chain_inputs()[n]
    big = [v for v in range(n) if len(st.members(int(np.bitwise_or.reduce(L.sets[v])))) > 12] or [0]
    _check_tables(L, big)  # the tables on both sides of the LDS limit at n = 63, one elsewhere
    tables = [st.butterfly(L, v) for v in range(n)]
    caps = [st.direct(L, v)[2] for v in range(n)]
    r = st.run(L, tables, seed, st.CHAINS, st.STEPS, st.THIN, caps=caps)
    assert r["min_excess"] >= 0, r["min_excess"]
    assert 0 < r["accepted"].sum() < st.CHAINS * st.STEPS
