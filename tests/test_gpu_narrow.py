"""The layer kernels' narrow form (option score_narrow).

A layer-5 or layer-6 launch of the default variant whose every set mask, rank,
launch-local index and table slot fits 32 bits runs a kernel that carries them
in 32-bit registers; any other launch runs the 64-bit kernel.  Nothing about a
score changes, so on every shape below a call with the option on and a call
with it off must give the same offsets, the same sets and the same score BITS
(error word 0), "narrow_launches" must say which form ran, and the lists must
hold the library's tolerance against the CPU oracle (sets equal, scores within
1e-6 relative) on a sample.  N = 500 rows throughout.  What each shape is for:

  n=9 k=6 full       the smallest shape with both phases of layers 5 and 6;
                     every wave straddles variables (the per-lane search reads
                     the low words of the work prefixes)
  ... constrained    two constraints: the constrained twin kernels
  ... without var 0  three variables lose variable 0 as a candidate: one
                     launch mixes shifted and unshifted masks
  n=36 m=32          one variable with 32 candidates that include variable 0
                     (phase 0: U = 31 shifted to bit 31; phase 1 likewise), one
                     with 32 that do not (phase 1: U = 32, bit 31 unshifted),
                     the others 6 to 8: C(32, 6) = 906,192 sets
  n=36 m=33          the same with 33 candidates for the first: every launch
                     must run the 64-bit kernel
  graph              capture, replay, the option flips (a new graph key), back
  no unrank table    score_unrank_lut = 0: every lane computes its mask in the
                     narrow form
"""
import numpy as np
import pytest

import synth
from test_gpu_cbic import REL_TOL
from test_gpu_unrank_lut import _full, _run, _same

pytestmark = pytest.mark.gpu

LAMBDA = 2.0
N = 500
CONS9 = [(2, 0b1000, 0), (5, 0, 0b10001)]  # (variable, required, forbidden)


def _without_var0(n, losers):
    variables, cands = _full(n)
    return variables, [c & ~1 if v in losers else c for v, c in zip(variables, cands)]


def _wide36(first):
    """n = 36: variable 35 with `first` candidates from variable 0 up, variable
    34 with 32 candidates from variable 1 up, variables 0..33 with 6 to 8."""
    n = 36
    rng = np.random.default_rng(3600)
    variables, cands = [], []
    for v in range(34):
        m = 6 + v % 3
        pool = [u for u in range(n) if u != v]
        pick = rng.choice(pool, size=m, replace=False)
        variables.append(v)
        cands.append(int(sum(1 << int(u) for u in pick)))
    variables += [34, 35]
    cands += [((1 << 32) - 1) << 1, (1 << first) - 1]
    sizes = [bin(c).count("1") for c in cands]
    assert sizes[-2:] == [32, first] and not cands[-2] & 1 and cands[-1] & 1
    assert all(6 <= s <= 8 for s in sizes[:-2]) and any(c & 1 for c in cands[:34]) and not all(c & 1 for c in cands[:34])
    return variables, cands


# name: (n, k, (variables, candidates), constraints, score_unrank_lut, narrow launches expected)
SHAPES = {
    "n9_full": (9, 6, _full(9), None, None, True),
    "n9_cons": (9, 6, _full(9), CONS9, None, True),
    "n9_without_var0": (9, 6, _without_var0(9, (3, 5, 8)), None, None, True),
    "n36_m32": (36, 6, _wide36(32), None, None, True),
    "n36_m33": (36, 6, _wide36(33), None, None, False),
    "n9_nolut": (9, 6, _full(9), None, 0, True),
}


def _planned(n, k, variables, cands):
    """the plan's own count of narrow launches for this call (host/narrow_check.cpp)"""
    from test_narrow_host import CHECK, run_plan
    plan, launches = run_plan(CHECK, (1, 241, 3, k, n, list(zip(variables, cands))))
    return plan["narrow_launches"], launches


def _check_oracle(oracle, X, variables, cands, k, cons, got, name):
    """Sets equal and scores within REL_TOL for the variables whose lists the
    oracle can rebuild in a moment; for a variable of 32 or 33 candidates
    (1.1 M sets) a sample of its stored sets' scores, the sets with the
    highest candidates among them."""
    offs, sets, scores = got
    ds = oracle.Dataset(X)
    small = [i for i, c in enumerate(cands) if bin(c).count("1") <= 12]
    small = small if len(small) <= 9 else small[::4]
    if cons:
        import test_constraints as tc
        want = tc.restate_lists(oracle, X, LAMBDA, [variables[i] for i in small], [cands[i] for i in small], k, cons)
        assert want[3] > 5 * REL_TOL, (name, "decision margin", want[3])
    for j, i in enumerate(small):
        if cons:
            ref_sets, ref_scores = want[1][want[0][j]:want[0][j + 1]], want[2][want[0][j]:want[0][j + 1]]
        else:
            ref_sets, ref_scores = ds.score_variable(LAMBDA, variables[i], cands[i], k)
        mine, vals = sets[offs[i]:offs[i + 1]], scores[offs[i]:offs[i + 1]].astype(np.float64)
        assert np.array_equal(mine, ref_sets), (name, variables[i])
        ref = np.asarray(ref_scores, dtype=np.float64)
        assert (np.abs(vals - ref) / np.maximum(np.abs(ref), 1.0)).max(initial=0.0) <= REL_TOL, (name, variables[i])
    for i, c in enumerate(cands):
        if bin(c).count("1") <= 12:
            continue
        mine, vals = sets[offs[i]:offs[i + 1]], scores[offs[i]:offs[i + 1]]
        assert len(mine) > 64, (name, variables[i], len(mine))
        top = int(c).bit_length() - 1  # the highest candidate: compact bit 31 (or 32)
        with_top = np.flatnonzero((mine >> np.uint64(top)) & np.uint64(1))
        assert len(with_top) > 0, (name, variables[i])
        pick = sorted(set(np.linspace(0, len(mine) - 1, 48).astype(int)) | set(with_top[-16:].tolist()))
        for j in pick:
            ref = -float(ds.cbic_raw(LAMBDA, variables[i], int(mine[j])))
            assert abs(float(vals[j]) - ref) <= REL_TOL * max(abs(ref), 1.0), (name, variables[i], hex(int(mine[j])))


@pytest.mark.parametrize("name", list(SHAPES))
def test_narrow_changes_nothing(oracle_built, name):
    import ulg
    n, k, (variables, cands), cons, lut, narrow = SHAPES[name]
    X, _ = synth.gaussian_sem(n, N, 9401 + n)
    want_launches, launches = _planned(n, k, variables, cands)
    assert (want_launches > 0) == narrow, (name, want_launches)
    ctx = ulg.Context(0)
    try:
        assert ctx.info("score_narrow") == 1
        ctx.load(X, LAMBDA)
        if cons:
            ctx.set_constraints(cons)
        if lut is not None:
            ctx.set_option("score_unrank_lut", lut)
        ctx.set_option("score_narrow", 0)
        off = _run(ctx, variables, cands, k)
        assert ctx.info("narrow_launches") == 0
        ctx.set_option("score_narrow", 1)
        on = _run(ctx, variables, cands, k)
        assert ctx.info("narrow_launches") == want_launches
        if lut == 0:
            assert ctx.info("unrank_lut_entries") == 0
        _same(off, on, name)
        if narrow:  # both phases of layers 5 and 6 ran narrow
            assert {(L, ph) for (_, L, ph), (_, nw) in launches.items() if nw} == {(5, 0), (5, 1), (6, 0), (6, 1)}
        if name == "n9_without_var0":  # one phase-1 launch holds variables with and without variable 0
            assert sum(1 for c in cands if c & 1) == 6
        _check_oracle(oracle_built, X, variables, cands, k, cons, on, name)
    finally:
        ctx.close()


def test_graph_replay_and_option_flip():
    import ulg
    n, k = 9, 6
    variables, cands = _full(n)
    X, _ = synth.gaussian_sem(n, N, 9401 + n)
    want_launches, _ = _planned(n, k, variables, cands)
    ctx = ulg.Context(0)
    try:
        ctx.load(X, LAMBDA)
        assert ctx.info("score_graph") == 1
        ctx.set_option("score_narrow", 0)
        ref = _run(ctx, variables, cands, k)
        for flag in (1, 1, 0, 0, 1):  # capture, replay, the key changes, replay, and back
            ctx.set_option("score_narrow", flag)
            ctx.score_async(variables, cands, k)
            st, _ = ctx.score_finish()
            assert ctx.info("score_error_word") == 0, flag
            assert ctx.info("narrow_launches") == (want_launches if flag else 0), flag
            _same(ref, ctx.fetch(st), ("graph", flag))
    finally:
        ctx.close()
