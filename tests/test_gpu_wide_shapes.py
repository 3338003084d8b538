"""The wide cBIC layers past 19 parents (score_wide_kernel, walk_wide_kernel,
walk_wide_lds_kernel, the hikey_* tables, the host hand-over) at the shapes
where the code changes path, on inputs whose walks are short by construction
(tests/wide_shapes.py: N = 256, lambda = 2, "strong" candidates that each gain
more than one penalty in any set, "junk" candidates at the lowest indices).

Which case crosses what (m candidates, k = m, so layers 9 .. m all run):

  m20_j3_*   control, C1-like: q reaches 20 (phase 0, variable 0 in the set)
             and 21 (phase 1, q = L + 1); the LMAX = 31 instances at L = 17..20;
             q = 20 has the `hi` bitset of walk_wide_lds_kernel in HBM.
  m21_*      q = 21, 22: past kStragQMax the budget is 0 and walk_wide_kernel
             finishes every walk, its `checked` bitset 2^(q-6) words per set;
             hikey_strided_kernel's third pass covers 1 bit.
  m22_*      third pass over 2 bits.
  m24_*      the last m with hi-cover tables, third pass over a full 4 bits,
             16.7 M sets; m24_all is held to the oracle's WHOLE list.
  m25_*      no table (hoff = ~0): every surviving set walks, with `checked`
             bitsets of up to 2^20 words, so a launch chunk shrinks to
             per = wslice / wpl walks (one chunk per few walks at the top
             layers); 33.5 M sets, a 134 MB table.
  mixed      three variables with m = 12, 24 and 25 in one call: hoff entries
             with and without ~0 in one launch, three stream groups, and one
             variable (m = 12) that does not have variable 0 as a candidate.
  *_zero_junk / *_zero_absent: variable 0 among the (junk) candidates, so both
             N4 phases run with q = L, or absent from them, so q = L + 1.
  score_sets with 26 .. 31 parents on an n = 40 input.

Layers of 28 <= m <= 31 candidates need >= 2^28 table slots per variable and
are out of reach of a test of a few seconds; m = 26, 27 are not run either.

References, none of them the code under test:
  decisions   oracle.Dataset.decide(..., stop=True) against the cache the GPU
              left, for every set of the top three layers, 40 + 40 random sets
              per layer 9 .. m - 3 and 200 stored sets: none skipped.  A layer's
              decision depends only on lower layers, so the lowest failing
              layer is the wrong one.
  structure   from the input alone: all 2^m sets stored where every candidate
              is strong; with junk, exactly the junk-free sets plus the sets
              with junk whose own score ts is positive (counted per (|S|, |J|)
              class).  tests/test_wide_shapes.py proves both against the
              oracle's full list at m = 12 and 14.
  values      tests/cbic_exact.py: every stored score among the sampled sets
              within the bound of DESIGN section 6 (cbic_exact.check_value).
  full list   tests/golden/wide_shapes_oracle.json and its every-512th-score
              vector wide_shapes_oracle_m24_all_scores.npy: the oracle's whole
              score_variable list of m24_all (make_wide_shapes_fixture.py; it
              took 549 s of CPU; m22_all 109 s, m21_all 53 s; m = 25 needs
              about twice m = 24, more than the ten minutes allowed).

The literal-walk maxima over exactly the sampled sets (CPU, before any GPU
run; budget 10^5 steps, tests/test_wide_shapes.py asserts it): 26 steps on
the all-strong inputs, 20 at m21_j2, 7267 at m20_j3, 12751 at m24_j3, 14457 at
m25_j3, 27084 at m22_j4, 40527 at m25_j4 and the mixed input's m = 25 variable.
The option-off runs (wide_prune 0, wide_reduced 0, wide_lds 0 / 2,
score_streams 1) make literal walks, and use only these inputs."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import cbic_exact as ce
import wide_shapes as ws
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = dict(wide_prune=1, wide_reduced=1, wide_lds=1, score_streams=3)
OPTION_RUNS = [dict(wide_prune=0), dict(wide_reduced=0), dict(wide_lds=0), dict(wide_lds=2), dict(score_streams=1)]
OPTION_CASES = ["m21_all", "m21_j2_zero_junk", "m21_j2_zero_absent", "m24_all", "m24_j3_zero_junk", "m24_j3_zero_absent"]


def _run(ctx, c, **opts):
    """One scoring call; the error word and the scored count are checked after it."""
    ctx.load(c.X, ws.LAM)
    try:
        for name, val in opts.items():
            ctx.set_option(name, val)
        stored, scored = ctx.score(c.variables, c.cands, c.k)
    finally:
        for name in opts:
            ctx.set_option(name, OPTION_DEFAULTS[name])
    assert ctx.info("score_error_word") == 0
    assert scored == sum(sum(math.comb(m, L) for L in range(min(m, c.k) + 1)) for m in c.mv)
    offs, sets, scores = ctx.fetch(stored)
    assert offs[0] == 0 and offs[-1] == stored == len(sets)
    return np.asarray(offs), np.asarray(sets, dtype=np.uint64), np.asarray(scores, dtype=np.float32)


class _List:
    """One variable's GPU list with membership by (layer, binary search)."""

    def __init__(self, sets, scores):
        self.sets, self.scores = sets, scores
        self.pc = np.bitwise_count(sets)
        assert np.all(np.diff(self.pc.astype(np.int8)) >= 0)
        self.start = np.searchsorted(self.pc, np.arange(66))

    def find(self, P):
        L = bin(P).count("1")
        a, b = int(self.start[L]), int(self.start[L + 1])
        i = a + int(np.searchsorted(self.sets[a:b], np.uint64(P)))
        return i if i < b and int(self.sets[i]) == P else -1


def _check_shape_and_structure(c, i, lst):
    sets, scores, pc = lst.sets, lst.scores, lst.pc
    m, ms, nj = c.mv[i], len(c.strong[i]), len(c.junk[i])
    assert int(sets[0]) == 0 and scores[0].tobytes() == np.float32(-0.0).tobytes()
    assert not np.any(sets & ~np.uint64(c.cands[i])) and pc[-1] <= m
    for L in range(m + 1):  # Gosper order: strictly increasing inside a layer, so no set twice
        a, b = int(lst.start[L]), int(lst.start[L + 1])
        assert np.all(sets[a + 1:b] > sets[a:b - 1]), (c.name, i, L)
    assert np.all(np.isfinite(scores))
    jm = np.uint64(c.junk_mask(i))
    free = (sets & jm) == 0
    assert int(free.sum()) == 1 << ms, (c.name, i, int(free.sum()))  # distinct subsets of the strong columns: all of them
    assert np.all(scores[free][1:] > 0)
    if nj == 0:
        assert len(sets) == 1 << m
        return
    assert np.all(scores[~free] < 0)  # a set with junk is stored only on a positive own score
    nk = np.bitwise_count(sets[~free] & jm).astype(np.int64)
    cnt = np.bincount((pc[~free].astype(np.int64) - nk) * 8 + nk, minlength=8 * (ms + 1))
    for (k, j), (lo, hi) in c.sign_classes(i).items():
        if j >= 1:
            want = math.comb(ms, k) * math.comb(nj, j) if lo > 0 else 0
            assert cnt[k * 8 + j] == want, (c.name, i, k, j, int(cnt[k * 8 + j]), want)
    assert len(sets) == c.expected_count(i)


def _check_decisions_and_values(oracle, c, i, lst):
    v = c.variables[i]
    ds = oracle.Dataset(c.X)
    cache = oracle.Cache(lst.sets, lst.scores)
    ex = ce.Exact(c.X)
    picks = ws.sample_sets(c, i)
    wrong, bad, stored = [], [], 0
    for P in picks:
        st, val = ds.decide(ws.LAM, v, P, cache, stop=True)
        at = lst.find(P)
        if st != (at >= 0):
            wrong.append((bin(P).count("1"), hex(P), st))
            continue
        if st and P:
            stored += 1
            kind, msg = ce.check_value(lst.scores[at], ws.N_REC, bin(P).count("1"), ws.LAM, ex.cbic(v, P, ws.LAM))
            if msg is not None or kind != "resolvable":
                bad.append((hex(P), kind, msg))
    assert not wrong, f"{c.name} variable {v}: lowest wrong layer first: {sorted(wrong)[:6]} ({len(wrong)} of {len(picks)})"
    assert not bad, bad[:5]
    assert stored >= 200 and len(picks) - stored >= (100 if c.junk[i] else 0)


def _check_case(oracle, c, offs, sets, scores):
    for i in range(len(c.variables)):
        lst = _List(sets[offs[i]:offs[i + 1]], scores[offs[i]:offs[i + 1]])
        _check_shape_and_structure(c, i, lst)
        _check_decisions_and_values(oracle, c, i, lst)


_default_digests = {}


def _digest(offs, sets, scores):
    return (offs.tobytes(), len(sets), hashlib.sha256(sets.tobytes()).hexdigest(),
            hashlib.sha256(scores.tobytes()).hexdigest())


@pytest.mark.parametrize("name", ws.GPU_SINGLE + [ws.MIXED])
def test_wide_shapes_default_options(ulg_ctx, oracle_built, name):
    c = ws.case(name)
    offs, sets, scores = _run(ulg_ctx, c)
    _default_digests[name] = _digest(offs, sets, scores)
    _check_case(oracle_built, c, offs, sets, scores)
    if name == "m24_all":
        _check_full_list(sets, scores)


def _check_full_list(sets, scores):
    """The oracle's whole list: count, SHA-256 of the sorted sets, score sum,
    and every 512th pair (its set through the SHA-256 of the whole list, its
    score from wide_shapes_oracle_m24_all_scores.npy), as c45_oracle.json is checked."""
    with open(os.path.join(GOLDEN, "wide_shapes_oracle.json")) as f:
        fx = json.load(f)["m24_all"]
    want = np.load(os.path.join(GOLDEN, "wide_shapes_oracle_m24_all_scores.npy")).astype(np.float64)
    order = np.argsort(sets, kind="stable")
    s, f32 = sets[order], scores[order]
    assert len(s) == fx["stored"]
    assert hashlib.sha256(s.tobytes()).hexdigest() == fx["sets_sha256"]
    tot = float(np.sum(f32.astype(np.float64)))
    assert abs(tot - fx["score_sum"]) <= 1e-6 * abs(fx["score_sum"])
    got = f32[::fx["sample_stride"]].astype(np.float64)
    assert len(got) == len(want) == fx["samples"]
    assert np.all(np.abs(got - want) <= 1e-6 * np.maximum(np.abs(want), 1e-30))


@pytest.mark.parametrize("opts", OPTION_RUNS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", OPTION_CASES)
def test_wide_shapes_options_identical_lists(ulg_ctx, name, opts):
    """Every walk form gives the default run's lists bit for bit (those are held
    to the references above), as test_wide_hicover_prune_identical_lists
    requires at small m: the same offsets and the same SHA-256 of the sets'
    and of the scores' bytes."""
    c = ws.case(name)
    if name not in _default_digests:  # run on its own: the default run first
        _default_digests[name] = _digest(*_run(ulg_ctx, c))
    assert _digest(*_run(ulg_ctx, c, **opts)) == _default_digests[name]


@pytest.mark.parametrize("name", ["m20_j3_zero_junk", "m24_j3_zero_absent", "m25_all"])
def test_wide_shapes_paths_taken(ulg_ctx, name):
    """The launches behind the claims above, from the profile: hi-cover tables
    up to m = 24 and none at 25; LDS replays where q <= 20; at m = 25 more walk
    launches than (layer, phase) pairs, because a chunk holds only
    wslice / wpl walks (4096 at q = 21, 128 at q = 26)."""
    c = ws.case(name)
    ulg_ctx.load(c.X, ws.LAM)
    names = ["wide_hicover", "walk_wide_lds", "walk_wide_var0", "walk_wide_rest"]
    try:
        ulg_ctx.profile(True)
        ulg_ctx.profile_select(names)
        ulg_ctx.profile_reset()
        ulg_ctx.score(c.variables, c.cands, c.k)
        cnt = {nm: (ulg_ctx.profile_get(nm) or {"count": 0})["count"] for nm in names}
    finally:
        ulg_ctx.profile(False)
        ulg_ctx.profile_select(None)
    assert ulg_ctx.info("score_error_word") == 0
    print(name, cnt)
    m = c.mv[0]
    if m <= 24:
        assert cnt["wide_hicover"] >= m - 8
        assert cnt["walk_wide_lds"] >= 1
    else:
        assert cnt["wide_hicover"] == 0 and cnt["walk_wide_lds"] == 0
        assert cnt["walk_wide_var0"] > m - 8 and cnt["walk_wide_rest"] > m - 8
    if not c.z(0):
        assert cnt["walk_wide_var0"] == 0 and cnt["walk_wide_rest"] >= 1


def test_score_sets_26_to_31_parents(ulg_ctx):
    """ulg_cbic_score_sets above the 25 parents the random draws of
    test_gpu_score_sets.py stop at: 300 draws of 26 .. 31 parents on an n = 40
    input (N = 256), each within the long-double bound."""
    n = 40
    rng = np.random.default_rng(9926)
    X = rng.standard_normal((ws.N_REC, n))
    X[:, n - 1] = X[:, :n - 1] @ rng.uniform(-1.0, 1.0, size=n - 1) + rng.standard_normal(ws.N_REC)
    ex = ce.Exact(X)
    vars_, parents = [], []
    for t in range(300):
        v = n - 1 if t % 2 else int(rng.integers(n))
        L = 26 + t % 6
        vars_.append(v)
        parents.append(ws.bits(rng.choice([u for u in range(n) if u != v], size=L, replace=False)))
    ulg_ctx.load(X, ws.LAM)
    got = ulg_ctx.score_sets(vars_, parents)
    bad = []
    for v, P, g in zip(vars_, parents, got):
        L = bin(P).count("1")
        kind, msg = ce.check_value(g, ws.N_REC, L, ws.LAM, ex.cbic(v, P, ws.LAM))
        if msg is not None or kind != "resolvable":
            bad.append((v, hex(P), kind, msg))
    assert not bad, bad[:5]
    assert sorted(set(bin(P).count("1") for P in parents)) == [26, 27, 28, 29, 30, 31]
