"""tests/order_picktables_ref.py against itself, without a GPU: on stage tables built by the float64 rounds,
the product of the levels' T-normalised conditionals (exact integers) is w(P) / A(U) from long-double sums
within law_bound, for every compatible stored set -- what stands in for a chi-square on the device."""
import numpy as np
import pytest

import order_picktables_ref as pk
import order_sumtables_ref as st
from test_gpu_order_tables import pooled_lists

LD = np.longdouble
K_OF = {0: 7, 1: 13, 2: 7}  # variable 2 has no empty set


def _ld(n):
    """A Python int as a long double, to its leading 63 bits."""
    s = max(0, n.bit_length() - 63)
    m = n >> s
    return np.ldexp(LD(m >> 32) * LD(2.0 ** 32) + LD(m & 0xFFFFFFFF), s)


@pytest.mark.parametrize("v", sorted(K_OF), ids=["K7", "K13", "K7-no-empty-set"])
def test_product_of_chunk_conditionals_is_the_posterior(v):
    L = pooled_lists(20, 5, lambda u: K_OF.get(u, 2), lambda u: 40, rooted=(2,), grid=0.5)
    C, T, stages, E = pk.build(L, v)
    K, nch = K_OF[v], pk.chunks(K_OF[v])
    assert len(T) == 1 << K and len(stages) == nch - 1 and np.array_equal(T, st.butterfly(L, v)[1])
    caps = {c: pk.direct(L, v, c)[2] for c in range(1, nch)}
    A = st.direct(L, v)[0]
    mem = st.members(C)
    idx = np.array([st.index(mem, S) for S in L.sets[v]])
    xs = range(1 << K) if K == 7 else [(1 << K) - 1] + list(np.random.default_rng(1).integers(0, 1 << K, 60))
    worst, seen = 0.0, 0
    for x in xs:
        x = int(x)
        if T[x] == -np.inf:
            continue
        for i in np.flatnonzero((idx & ~x) == 0):
            num, den, rel, floors = pk.law(K, stages, E, L.sc[v], x, T[x], int(idx[i]), caps)
            p = np.exp(LD(L.sc[v][i]) - A[x])
            err, bound = float(abs(_ld(num) / _ld(den) - p)), float(p) * rel + floors
            assert err <= bound, (x, i, err, bound)
            worst, seen = max(worst, err / bound), seen + 1
    assert seen > 100 and (v != 2 or T[0] == -np.inf)
    print(f"K = {K}: {seen} sets, the largest error is {worst:.3f} of law_bound")
