"""ulg_cbic_score_async / ulg_cbic_score_finish: a scoring call queued
without waiting gives the lists ulg_cbic_score gives, also with two
contexts' calls in flight at once on one GPU (the throughput loop of
scripts/slots_probe.py), and a later scorer call, fetch or load collects a
pending one first."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


def _lists(ctx, stored):
    offs, sets, scores = ctx.fetch(stored)
    return np.asarray(offs).copy(), np.asarray(sets).copy(), np.asarray(scores).copy()


@pytest.mark.parametrize("n,k", [(20, 4), (25, 6)])
def test_async_scoring_equals_sync(n, k):
    import ulg
    X, _ = synth.gaussian_sem(n, 10000, 9200)
    full = [(1 << n) - 1] * n
    a, b = ulg.Context(0), ulg.Context(0)
    try:
        for c in (a, b):
            c.load(X, 2.0)
        st, sc = a.score(list(range(n)), full, k)
        ref = _lists(a, st)
        half = list(range(0, n, 2))
        st_h, _ = a.score(half, [full[v] for v in half], k)
        ref_h = _lists(a, st_h)
        for _ in range(3):
            # two calls in flight on two contexts, finished in launch order
            a.score_async(list(range(n)), full, k)
            b.score_async(half, [full[v] for v in half], k)
            assert a.score_finish() == (st, sc)
            sb, _ = b.score_finish()
            assert sb == st_h
            for got, want in ((_lists(a, st), ref), (_lists(b, sb), ref_h)):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                assert got[2].tobytes() == want[2].tobytes()
        # a pending call is collected by the next call / fetch on its context
        a.score_async(list(range(n)), full, k)
        got = _lists(a, st)
        assert np.array_equal(got[1], ref[1]) and got[2].tobytes() == ref[2].tobytes()
        a.score_async(half, [full[v] for v in half], k)
        assert a.score(list(range(n)), full, k) == (st, sc)
    finally:
        a.close()
        b.close()


def test_load_collects_a_pending_async_call():
    """score_async, load, then any scorer call: ulg_cbic_load collects the
    pending call (as ulg_disc_load does) instead of leaving its flag set over
    scored = false, which made the third call fail once with "nothing scored".
    The lists after the reload are a fresh context's."""
    import ulg
    n, k = 12, 4
    X, _ = synth.gaussian_sem(n, 2000, 9300)
    X2, _ = synth.gaussian_sem(n, 2000, 9301)
    full = [(1 << n) - 1] * n
    a, fresh = ulg.Context(0), ulg.Context(0)
    try:
        fresh.load(X2, 2.0)
        st, sc = fresh.score(list(range(n)), full, k)
        ref = _lists(fresh, st)
        a.load(X, 2.0)
        a.score_async(list(range(n)), full, k)
        a.load(X2, 2.0)
        assert a.score(list(range(n)), full, k) == (st, sc)
        got = _lists(a, st)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert got[2].tobytes() == ref[2].tobytes()
        # ... and with score_sets and the async form as the third call
        a.score_async(list(range(n)), full, k)
        a.load(X, 2.0)
        a.load(X2, 2.0)
        vals = a.score_sets([3, 5], [0b110, 0b1011])
        assert vals.tobytes() == fresh.score_sets([3, 5], [0b110, 0b1011]).tobytes()
        a.score_async(list(range(n)), full, k)
        a.load(X2, 2.0)
        a.score_async(list(range(n)), full, k)
        assert a.score_finish() == (st, sc)
        got = _lists(a, st)
        assert np.array_equal(got[1], ref[1]) and got[2].tobytes() == ref[2].tobytes()
    finally:
        a.close()
        fresh.close()
