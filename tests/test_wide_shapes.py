"""CPU proofs behind tests/test_gpu_wide_shapes.py (no GPU here).

  * tests/wide_walk_ref.py (the step-counting literal walk) against the oracle:
    on weak-signal data (synth.gaussian_sem, n = 11) and on the designed inputs
    at m = 12, every set with a negative own score is decided as the oracle's
    full list has it; at m = 14 the sampled sets are.
  * the two structural claims of tests/wide_shapes.py against the oracle's full
    list at m = 12 and 14: with only strong candidates all 2^m sets are stored;
    with junk the stored sets are exactly the junk-free ones plus the sets
    whose own score ts is positive, and their number is expected_count().
  * ora_decide_stop (the oracle's decision that leaves the recursion at the
    first key >= -ts) equals ora_decide and the full list on the same inputs.
    The GPU tests need it: the literal ora_decide took 0.79 s for the full set
    of m20_j3_zero_junk and doubles with every further member (the recursion
    visits every absent subset of a dominated set), against 0.05 s for all
    1103 sampled sets with the stop.
  * the step budget: for every input the GPU tests use, over exactly the sets
    they re-decide (wide_shapes.sample_sets), the literal walk stays under
    WALK_BUDGET = 10^5 steps, against the by-construction list.  Measured
    maxima: 26 steps on the all-strong inputs (m + 1), 20 at m21_j2, 7267 at
    m20_j3, 12751 at m24_j3, 14457 at m25_j3, 27084 at m22_j4, 40527 at m25_j4
    and on the mixed input's m = 25 variable.
  * the design's margins: no (|S|, |J|) class has ts within 0.5 of zero, and
    every strong column gains at least 2.5 beyond its penalty."""
import numpy as np
import pytest

import synth
import wide_shapes as ws
import wide_walk_ref as wr


def _lookup(sets, scores):
    d = {int(a): np.float32(b) for a, b in zip(sets, scores)}
    return d.get, d


@pytest.mark.parametrize("v", [0, 5])
def test_walk_helper_decides_as_the_oracle_weak_signal(oracle_built, v):
    n = 11
    X, _ = synth.gaussian_sem(n, 200, 9400)
    ds = oracle_built.Dataset(X)
    s, sc = ds.score_variable(2.0, v, (1 << n) - 1, n - 1)
    look, d = _lookup(s, sc)
    cache = oracle_built.Cache(s, sc)
    others = [u for u in range(n) if u != v]
    walked = dominated = 0
    for r in range(1, 1 << (n - 1)):
        P = ws.bits(others[b] for b in range(n - 1) if (r >> b) & 1)
        ts = ds.cbic_raw(2.0, v, P)
        if ts >= 0:
            continue
        dom, _ = wr.decide_walk(P, look, np.float32(-ts), v != 0)
        assert dom == (P not in d), (v, hex(P))
        st, val = ds.decide(2.0, v, P, cache, stop=True)
        assert st == (P in d) and val == np.float32(-ts), (v, hex(P))
        walked += 1
        dominated += dom
    assert walked >= 500 and 100 <= dominated <= walked - 10


@pytest.fixture(scope="module")
def full_lists(oracle_built):
    out = {}

    def get(name):
        if name not in out:
            c = ws.case(name)
            out[name] = oracle_built.Dataset(c.X).score_variable(ws.LAM, c.variables[0], c.cands[0], c.k)
        return out[name]
    return get


@pytest.mark.parametrize("name", ws.CPU_FULL)
def test_structure_equals_the_full_oracle_list(full_lists, name):
    c = ws.case(name)
    s, sc = full_lists(name)
    got = set(int(x) for x in s)
    cand = [u for u in range(c.n) if (c.cands[0] >> u) & 1]
    want = set()
    for r in range(1 << len(cand)):
        P = ws.bits(cand[b] for b in range(len(cand)) if (r >> b) & 1)
        if c.stored(0, P):
            want.add(P)
    assert got == want
    assert len(got) == c.expected_count(0)
    if not c.junk[0]:
        assert len(got) == 1 << c.mv[0]
    jm = c.junk_mask(0)
    assert sum(1 for P in got if not (P & jm)) == 1 << len(c.strong[0])
    for P, f in zip(s, sc):  # a stored set with junk: a non-negative own score, stored negative
        if int(P) & jm:
            assert f < 0


@pytest.mark.parametrize("name", ws.CPU_FULL)
def test_walk_helper_and_decide_stop_on_the_designed_inputs(oracle_built, full_lists, name):
    c = ws.case(name)
    v = c.variables[0]
    s, sc = full_lists(name)
    look, d = _lookup(s, sc)
    ds = oracle_built.Dataset(c.X)
    cache = oracle_built.Cache(s, sc)
    picks = ws.sample_sets(c, 0)
    if c.mv[0] <= 12:
        cand = [u for u in range(c.n) if (c.cands[0] >> u) & 1]
        picks = [ws.bits(cand[b] for b in range(len(cand)) if (r >> b) & 1) for r in range(1, 1 << len(cand))]
    for P in picks:
        st, val = ds.decide(ws.LAM, v, P, cache)
        assert st == (P in d), hex(P)
        assert ds.decide(ws.LAM, v, P, cache, stop=True) == (st, val), hex(P)
        ts = ds.cbic_raw(ws.LAM, v, P)
        if P and ts < 0:
            dom, steps = wr.decide_walk(P, look, np.float32(-ts), c.z(0))
            assert dom == (P not in d), hex(P)
            # the by-construction list gives the same walk
            assert wr.decide_walk(P, c.lookup(0), np.float32(-ts), c.z(0)) == (dom, steps), hex(P)


def test_walk_helper_budget_raises():
    c = ws.case("m14_j4_zero_absent")
    P = c.cands[0]
    with pytest.raises(wr.BudgetExceeded):
        wr.decide_walk(P, c.lookup(0), np.float32(-c.ts(0, P)), c.z(0), budget=5)


@pytest.mark.parametrize("name", ws.GPU_SINGLE + [ws.MIXED])
def test_gpu_inputs_margins_and_step_budget(name):
    c = ws.case(name)
    worst = 0
    for i in range(len(c.variables)):
        cl = c.sign_classes(i)
        ms = len(c.strong[i])
        for (k, j), (lo, hi) in cl.items():
            if k + j:
                assert lo * hi > 0 and min(abs(lo), abs(hi)) >= 0.5, (name, i, k, j, lo, hi)
        assert min(cl[(k, 0)][0] - cl[(k + 1, 0)][1] for k in range(ms)) >= 2.5
        assert c.expected_count(i) >= 1 << ms
        look = c.lookup(i)
        for P in ws.sample_sets(c, i):
            ts = c.ts(i, P)
            if ts >= 0:
                assert c.stored(i, P)
                continue
            dom, steps = wr.decide_walk(P, look, np.float32(-np.float32(ts)), c.z(i), budget=ws.WALK_BUDGET)
            assert dom == (not c.stored(i, P)), (name, i, hex(P))
            worst = max(worst, steps)
    print(f"{name}: worst literal walk over the sampled sets {worst} steps")
    assert worst < ws.WALK_BUDGET
