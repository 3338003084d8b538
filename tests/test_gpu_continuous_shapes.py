"""The continuous path at the shapes the rest of the suite never reaches.

Load: colstats / normalise / gram_mfma / gram_reduce against a long-double Gram
matrix at n = 1 ... 63 around the 16-column tiles, N around the 1024-row MFMA
chunks and the 4-row MFMA step, on data with a large mean, with column scales
of 10^-100 ... 10^100, with a duplicated and with a constant column.

Scorer: ulg_cbic_score, ulg_cbic_score_sets and the .pss formatter with
variables and candidates above bit 31 (n = 63, compact candidate lists of up to
62), against the oracle.

Fisher z: ulg_mmpc_min_z -- one lane of ulg_mmpc's own query launch per query --
against the minimum of ora_partial_z over the same subsets on the very matrix
ulg_cbic_gram returns, both template instances of mmpc_query_kernel, and
ulg_mmpc on data whose hub has twelve neighbours.  ora_partial_z itself is held
to long double in test_fisher_z.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import synth
from test_fisher_z import LD, STAR_CHILDREN, STAR_HUB, ld_gram, min_z_sets, star_data
from test_gpu_cbic import REL_TOL, _compare_lists, _oracle_lists

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------
# C1: the Gram matrix against long double
# ---------------------------------------------------------------------------
GRAM_SHAPES = [(1, 2), (2, 3), (16, 3), (17, 5), (15, 1023), (16, 1024), (17, 1025), (32, 2047), (33, 2049),
               (48, 4099), (63, 4099)]
CLASS_SHAPES = {"std": GRAM_SHAPES, "offset": [(17, 1025), (63, 4099)], "scaled": [(17, 1025), (63, 4099)],
                "dup": [(17, 1025), (63, 4099)], "const": [(17, 1025), (63, 4099)]}
# A cap, not a measurement: an FP64 restatement of the four kernels on the CPU (block
# sums, 1024-row partials) stays below 3e-15 (N - 1) on every class and shape here; a
# dropped row or a swapped 16 x 16 tile moves an entry by 1e-3 (N - 1) or more.
GRAM_TOL = 1e-9


def gram_data(cls, n, N):
    """-> (X, constant column or None)."""
    rng = np.random.default_rng([9940, n, N])
    X = rng.standard_normal((N, n))
    const = None
    if cls == "offset":
        X = X + 1e8
    elif cls == "scaled":
        X = X * 10.0 ** rng.integers(-100, 101, n)
    elif cls == "dup":
        X[:, 5] = X[:, 2]
    elif cls == "const":
        const = n - 2
        X[:, const] = 3.0  # N x 3.0 sums exactly, so the centred column is exactly 0 and 0 / 0 = NaN
    return X, const


@pytest.mark.parametrize("cls,n,N", [(c, n, N) for c, shapes in CLASS_SHAPES.items() for n, N in shapes])
def test_gram_matches_long_double(ulg_ctx, cls, n, N):
    X, const = gram_data(cls, n, N)
    ulg_ctx.load(X, 2.0)
    G = ulg_ctx.gram()
    ref = ld_gram(X)
    tol = GRAM_TOL * (N - 1)
    nan = np.zeros((n, n), dtype=bool)
    if const is not None:
        nan[const, :] = nan[:, const] = True
    assert np.array_equal(np.isnan(G), nan)
    assert np.array_equal(np.isnan(np.asarray(ref, dtype=np.float64)), nan)
    ok = ~nan
    err = np.abs(G.astype(LD) - ref)[ok].astype(np.float64)
    print(f"gram {cls} n={n} N={N}: max |G - G_exact| / (N - 1) = {err.max() / (N - 1):.3g}")
    assert err.max() <= tol
    assert np.abs(G - G.T)[ok].max() <= tol
    if cls == "dup":
        assert abs(G[2, 5] - (N - 1)) <= tol and abs(G[5, 2] - (N - 1)) <= tol
    if N == 2:
        assert np.all(np.abs(np.abs(G) - 1.0) <= tol)


# ---------------------------------------------------------------------------
# C2: the scorer past bit 31
# ---------------------------------------------------------------------------
N63, ROWS63, LAM = 63, 403, 2.0  # 403 rows: one MFMA chunk with a 3-row tail
FULL63 = (1 << N63) - 1


@pytest.fixture(scope="module")
def x63():
    return synth.gaussian_sem(N63, ROWS63, 9950)[0]


@pytest.fixture(scope="module")
def oracle_k2(oracle_built, x63):
    """The oracle's k = 2 lists of all 63 variables over all 62 candidates."""
    return _oracle_lists(oracle_built, x63, LAM, list(range(N63)), [FULL63] * N63, 2)


def _binomial_count(variables, cands, k):
    return sum(math.comb(bin(int(c) & ~(1 << v)).count("1"), L) for v, c in zip(variables, cands) for L in range(k + 1))


def _score_and_compare(ctx, oracle, X, lam, variables, cands, k, what, ref=None):
    ctx.load(X, lam)
    stored, scored = ctx.score(variables, cands, k)
    assert ctx.info("score_error_word") == 0
    assert scored == _binomial_count(variables, cands, k), what
    g = ctx.fetch(stored)
    o = ref if ref is not None else _oracle_lists(oracle, X, lam, variables, cands, k)
    _compare_lists(*o, *g, variables, ctx=what)
    return g


def test_layers_k2_all_63_variables(ulg_ctx, oracle_built, x63, oracle_k2):
    _score_and_compare(ulg_ctx, oracle_built, x63, LAM, list(range(N63)), [FULL63] * N63, 2, "n=63 k=2", oracle_k2)


def test_layers_k3_low_and_high_variables(ulg_ctx, oracle_built, x63):
    v = [0, 31, 32, 62]
    _score_and_compare(ulg_ctx, oracle_built, x63, LAM, v, [FULL63] * len(v), 3, "n=63 k=3")


def test_layers_k2_without_variable_0(ulg_ctx, oracle_built, x63):
    """Candidate lists without variable 0: phase 1 alone, compact index 0 = variable 1 or 2."""
    v = list(range(1, N63))
    _score_and_compare(ulg_ctx, oracle_built, x63, LAM, v, [FULL63 & ~1] * len(v), 2, "n=63 k=2 no 0")


@pytest.mark.parametrize("with0", [False, True])
def test_sparse_candidates_above_bit_31(ulg_ctx, oracle_built, x63, with0):
    rng = np.random.default_rng(9951)
    v = [33, 47, 62]
    cands = []
    for x in v:
        c = sum(1 << int(b) for b in rng.choice(np.arange(32, N63), size=11, replace=False))
        cands.append(c | (1 if with0 else 0))
    assert all(bin(c & ~(1 << x) & ~1).count("1") >= 10 for x, c in zip(v, cands))
    _score_and_compare(ulg_ctx, oracle_built, x63, LAM, v, cands, 4, f"sparse high with0={with0}")


@pytest.mark.parametrize("with0", [False, True])
def test_wide_layers_above_bit_31(ulg_ctx, oracle_built, x63, with0):
    """Variable 62 with 11 candidates among 33 ... 61 (12 with variable 0), k = 10: layers 9 and 10 are wide."""
    rng = np.random.default_rng(9952)
    c = sum(1 << int(b) for b in rng.choice(np.arange(33, 62), size=11, replace=False)) | (1 if with0 else 0)
    _score_and_compare(ulg_ctx, oracle_built, x63, LAM, [62], [c], 10, f"wide high with0={with0}")


def test_score_sets_over_all_63_bits(ulg_ctx, oracle_built, x63):
    ulg_ctx.load(x63, LAM)
    offs, sets, scores = ulg_ctx.score_all(list(range(N63)), [FULL63] * N63, 2)
    # what the layer scorer stored comes back bit for bit, with and without the variable's own bit
    vars_ = np.repeat(np.arange(N63, dtype=np.int32), np.diff(offs))
    own = np.left_shift(np.uint64(1), vars_.astype(np.uint64))
    nonempty = sets != 0
    assert nonempty.sum() > 500 and (sets >> np.uint64(32)).any()
    for parents in (sets, sets | own):
        got = ulg_ctx.score_sets(vars_, parents)
        assert np.array_equal(got[nonempty].view(np.uint32), scores[nonempty].view(np.uint32))
        assert np.all(got[~nonempty] == 0.0) and np.all(np.signbit(got[~nonempty]))
    # 300 pairs of 0 ... 25 parents drawn from all 63 bits against the oracle's per-row OLS
    ds = oracle_built.Dataset(x63)
    rng = np.random.default_rng(9953)
    pv, pp = [], []
    for i in range(300):
        v = 62 if i < 20 else int(rng.integers(N63))
        size = int(rng.integers(0, 26))
        others = [x for x in range(N63) if x != v]
        pv.append(v)
        pp.append(sum(1 << int(b) for b in rng.choice(others, size=size, replace=False)))
    assert any(p >> 62 for p in pp) and any(p & 1 for p in pp)
    got = ulg_ctx.score_sets(pv, pp)
    got_own = ulg_ctx.score_sets(pv, [p | (1 << v) for v, p in zip(pv, pp)])
    assert np.array_equal(got.view(np.uint32), got_own.view(np.uint32))
    for v, P, g in zip(pv, pp, got):
        ref = -float(ds.cbic_raw(LAM, v, P))
        assert abs(float(g) - ref) <= REL_TOL * max(abs(ref), 1.0), (v, hex(P), float(g), ref)


@pytest.mark.parametrize("cls", ["offset", "scaled"])
def test_offset_and_scaled_data_score_like_the_oracle(ulg_ctx, oracle_built, cls):
    """A mean of 1e8 and column scales of 10^-100 ... 10^100 at (12, 1025), full skeleton, k = 4."""
    n, N = 12, 1025
    X, _ = synth.gaussian_sem(n, N, 9954)
    rng = np.random.default_rng(9955)
    X = X + 1e8 if cls == "offset" else X * 10.0 ** rng.integers(-100, 101, n)
    _score_and_compare(ulg_ctx, oracle_built, X, LAM, list(range(n)), [(1 << n) - 1] * n, 4, cls)


def _ref_pss(oracle, tmp_path, names, arity, offs, sets, scores, N, k):
    ref = tmp_path / "ref.pss"
    oracle.write_pss(str(ref), names, arity, offs, sets, scores, num_records=N, parent_limit=k)
    text = ref.read_bytes()
    return text, text[: text.index(b"VAR ")].decode()


def test_pss_text_with_63_names(ulg_ctx, oracle_built, x63, tmp_path):
    names = [f"V{i}" if i % 3 else f"variable_{i}_long" for i in range(N63)]
    arity = [ROWS63] * N63
    # host lists whose sets use bits 32 ... 62
    rng = np.random.default_rng(9956)
    offs, sets, scores = [0], [], []
    for v in range(N63):
        for _ in range(int(rng.integers(0, 6))):
            s = int(rng.integers(0, 1 << 31)) << 32 | int(rng.integers(0, 1 << 32))
            if rng.random() < 0.5:
                s &= ~((1 << 32) - 1)
            sets.append(s & FULL63 & ~(1 << v))
            scores.append(np.float32(rng.normal(0, 1e3)))
        if v == 62:
            sets.append(FULL63 & ~(1 << 62))
            scores.append(np.float32(-1.5))
        offs.append(len(sets))
    ref_text, header = _ref_pss(oracle_built, tmp_path, names, arity, offs, sets, scores, ROWS63, 62)
    assert ulg_ctx.pss_format_lists(header, names, arity, offs, sets, scores) == ref_text
    # the device lists of the k = 2 run
    ulg_ctx.load(x63, LAM)
    st, _ = ulg_ctx.score(list(range(N63)), [FULL63] * N63, 2)
    offs, sets, scores = ulg_ctx.fetch(st)
    ref_text, header = _ref_pss(oracle_built, tmp_path, names, arity, offs, sets, scores, ROWS63, 2)
    assert ulg_ctx.pss_format(header, names, arity) == ref_text


# ---------------------------------------------------------------------------
# D: Fisher-z values and both instances of mmpc_query_kernel
# ---------------------------------------------------------------------------
# ulps of the result.  Every operation of partial_z is IEEE-identical on both
# sides except the device log; measured on an MI355X: ULP_SEEN.
ULP_LIMIT = 4
ULP_SEEN = 1


def _ora_vals(oracle, G, N, X, T, sets):
    f = oracle.lib().ora_partial_z
    gp = G.ctypes.data_as(C.c_void_p)
    n = G.shape[0]
    return [f(gp, n, float(N), X, T, (C.c_int * len(S))(*S), len(S)) for S in sets]


def _min_with_stop(vals, stop):
    """min_z's loop over the values of its sets in order."""
    best = math.inf
    for z in vals:
        if z < best:
            best = z
        if best <= stop:
            break
    return best


def _mid_stop(vals):
    """A stop some set in the middle of the enumeration meets first: half way between two
    well separated neighbours of the sorted values, so that one ulp of the device log cannot
    move a value across it."""
    sv = sorted(v for v in vals if math.isfinite(v))
    for j in range(len(sv) // 2, len(sv) - 1):
        if sv[j + 1] - sv[j] > 1e-6 * sv[j + 1]:
            return 0.5 * (sv[j] + sv[j + 1])
    return 2.0 * sv[-1] + 1.0 if sv else 0.0


def _ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def _assert_close(got, want, what):
    """-> ulp distance; inf, exact 0 and NaN must match exactly."""
    if math.isnan(want) or math.isinf(want) or want == 0.0 or math.isnan(got) or math.isinf(got) or got == 0.0:
        assert (math.isnan(got) and math.isnan(want)) or got == want, (what, got, want)
        return 0
    d = _ulps(got, want)
    assert d <= ULP_LIMIT, (what, got, want, d)
    return d


@pytest.fixture(scope="module")
def star():
    return star_data()


@pytest.mark.parametrize("max_cond", [-1, 2])
def test_star_skeleton_runs_the_wide_instance(ulg_ctx, oracle_built, star, max_cond):
    """The hub keeps >= 10 neighbours, so its forward rounds had pools of >= 9: with
    max_cond = -1 those launches are mmpc_query_kernel<24>, with max_cond = 2 the <8>
    instance enumerates pools of more than 8."""
    ulg_ctx.load(star, 0.0)
    got = ulg_ctx.mmpc(0.01, max_cond)
    assert got == oracle_built.Dataset(star).mmpc(0.01, max_cond)
    assert bin(got[STAR_HUB]).count("1") >= 10
    assert all((got[STAR_HUB] >> c) & 1 for c in STAR_CHILDREN)


def _star_queries(rng, sizes_musts, pairs_of):
    """-> [(T, X, must, pool)]: must below, inside and above the pool's range or -1;
    every third pair has X and T above bit 31."""
    out = []
    for p, musts in sizes_musts:
        for j in range(pairs_of(p)):
            cols = [int(v) for v in rng.permutation(40)]
            if j % 3 == 0:
                hi = [v for v in cols if v >= 32]
                cols = hi[:2] + [v for v in cols if v not in hi[:2]]
            X, T, rest = cols[0], cols[1], cols[2:]
            if j % 2 == 0 and STAR_HUB not in (X, T):  # the hub among the conditioning variables
                rest = [STAR_HUB] + [v for v in rest if v != STAR_HUB]
            c = sorted(rest[:p + 3])
            mid = (p + 3) // 2
            named = {"below": c[0], "inside": c[mid], "above": c[-1]}
            pool = [v for i, v in enumerate(c) if i not in (0, mid, p + 2)]
            for m in musts:
                out.append((T, X, -1 if m == "none" else named[m], pool))
    return out


ALL_MUSTS = ("below", "inside", "above", "none")
# one call per list: the first keeps every conditioning set at <= 8 variables (instance <8>
# whatever max_cond), the second reaches 9 ... 13 (instance <24> once max_cond >= 9)
NARROW = [(0, ALL_MUSTS), (1, ALL_MUSTS), (7, ALL_MUSTS), (8, ("none",))]
WIDE = [(8, ("below", "inside", "above")), (9, ALL_MUSTS), (12, ALL_MUSTS)]


@pytest.mark.parametrize("max_cond", [0, 1, 3, 24])
def test_min_z_matches_oracle_on_the_same_gram(ulg_ctx, oracle_built, star, max_cond):
    ulg_ctx.load(star, 0.0)
    G = ulg_ctx.gram()
    N = star.shape[0]
    rng = np.random.default_rng(9960 + max_cond)
    worst = 0
    for name, spec in (("narrow", NARROW), ("wide", WIDE)):
        qs = _star_queries(rng, spec, lambda p: 4 if p == 12 else 12)
        ts, xs, ms, pools, stops, want = [], [], [], [], [], []
        for T, X, must, pool in qs:
            vals = _ora_vals(oracle_built, G, N, X, T, list(min_z_sets(pool, must, max_cond)))
            for stop in (-math.inf, _mid_stop(vals), math.inf):
                ts.append(T), xs.append(X), ms.append(must), stops.append(stop)
                pools.append(sum(1 << v for v in pool))
                want.append(_min_with_stop(vals, stop))
        assert len(ts) >= 300 and any(x >= 32 and t >= 32 for x, t in zip(xs, ts))
        got = ulg_ctx.mmpc_min_z(ts, xs, ms, pools, max_cond, stops)
        for i in range(len(ts)):
            worst = max(worst, _assert_close(got[i], want[i], (name, ts[i], xs[i], ms[i], hex(pools[i]), stops[i])))
        # must may also be named in the pool mask: the same query
        again = ulg_ctx.mmpc_min_z(ts, xs, ms, [p | (1 << m if m >= 0 else 0) for p, m in zip(pools, ms)], max_cond,
                                   stops)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    print(f"min_z max_cond={max_cond}: largest distance {worst} ulp")


def test_min_z_edge_data(ulg_ctx, oracle_built):
    """A constant column (NaN), a copy of X in the pool (a <= 0 or rounding noise), X a copy
    of T (the clamp) and N = 6 with |S| = 3 (dof = 0): the oracle's answer on the same G."""
    X, _ = synth.gaussian_sem(8, 403, 9961)
    X[:, 3] = 3.0
    X[:, 6] = X[:, 1]
    worst = 0
    for data in (X, X[:6]):
        N = data.shape[0]
        ulg_ctx.load(data, 0.0)
        G = ulg_ctx.gram()
        assert np.isnan(G[3]).all() and np.isnan(G[:, 3]).all() and np.isnan(G).sum() == 15
        qs = [(0, 3, -1, []), (3, 0, -1, []), (3, 0, -1, [2, 5]), (0, 3, 2, [5]),      # constant X or T
              (0, 2, -1, [3]), (0, 2, -1, [3, 5, 7]), (0, 2, 3, [5, 7]), (0, 2, 5, [3, 7]),  # constant in the pool
              (0, 1, -1, [6]), (0, 1, 6, [2, 5]), (4, 6, -1, [1, 2]), (4, 6, 1, [2]),    # a copy of X in the pool
              (1, 6, -1, []), (6, 1, -1, [0, 2]), (1, 6, 4, [0]),                      # X a copy of T
              (0, 2, -1, [4, 5, 7]), (0, 2, 4, [5, 7]), (5, 7, -1, [0, 2, 4])]          # |S| up to 3
        for max_cond in (24, 3, 2):
            for stop in (-math.inf, math.inf):
                want = [_min_with_stop(_ora_vals(oracle_built, G, N, x, t, list(min_z_sets(pool, must, max_cond))),
                                       stop) for t, x, must, pool in qs]
                got = ulg_ctx.mmpc_min_z([q[0] for q in qs], [q[1] for q in qs], [q[2] for q in qs],
                                         [sum(1 << v for v in q[3]) for q in qs], max_cond, [stop] * len(qs))
                for i, q in enumerate(qs):
                    worst = max(worst, _assert_close(got[i], want[i], (N, max_cond, stop, q)))
                if stop == -math.inf:
                    assert got[0] == math.inf and got[1] == math.inf  # nothing but NaN: the minimum stays +inf
                    assert got[4] > 0 and math.isfinite(got[4])       # the empty set survives a NaN pool member
                    r = 1 - 1e-15                                     # X a copy of T: the clamped value
                    assert _ulps(got[12], abs(0.5 * math.log((1 + r) / (1 - r))) * math.sqrt(N - 3)) <= ULP_LIMIT
        if N == 6:
            # |S| = 3 is all that max_cond = 24 adds to the last three queries: dof = 0 gives exactly 0
            z = ulg_ctx.mmpc_min_z([0, 0], [2, 2], [-1, 4], [0b10110000, 0b10100000], 24, [-math.inf] * 2)
            assert z[0] == 0.0 and z[1] == 0.0
    print(f"min_z edge data: largest distance {worst} ulp")


def test_min_z_rejects_bad_input(ulg_ctx, star):
    import ulg
    ulg_ctx.load(star, 0.0)
    inf = [-math.inf]
    bad = [([5], [5], [-1], [0]),            # x = t
           ([5], [6], [-1], [1 << 5]),       # t in the pool
           ([5], [6], [-1], [1 << 6]),       # x in the pool
           ([5], [6], [5], [0]),             # must = t
           ([5], [6], [6], [0]),             # must = x
           ([40], [6], [-1], [0]),           # t out of range
           ([5], [-1], [-1], [0]),           # x out of range
           ([5], [6], [40], [0]),            # must out of range
           ([5], [6], [-1], [1 << 40]),      # mask bit >= n
           ([38], [39], [-1], [(1 << 25) - 1]),           # a pool of 25
           ([38], [39], [30], [(1 << 24) - 1])]           # 24 and a must outside
    for t, x, m, p in bad:
        with pytest.raises(ulg.ULGError, match="status 1"):
            ulg_ctx.mmpc_min_z(t, x, m, p, -1, inf)
    assert len(ulg_ctx.mmpc_min_z([], [], [], [], -1, [])) == 0
    fresh = ulg.Context(0)
    try:
        with pytest.raises(ulg.ULGError, match="status 3"):
            fresh.mmpc_min_z([0], [1], [-1], [0], -1, inf)
    finally:
        fresh.close()
    # the lists of the context are left alone
    X, _ = synth.gaussian_sem(6, 403, 9962)
    ulg_ctx.load(X, 2.0)
    a = ulg_ctx.score_all(list(range(6)), [63] * 6, 3)
    ulg_ctx.mmpc_min_z([0, 1], [1, 2], [-1, 3], [0b111000, 0b110000], -1, [-math.inf] * 2)
    b = ulg_ctx.fetch(len(a[1]))
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("col", [0, 4, 11])
def test_mmpc_constant_column_has_no_edge(ulg_ctx, oracle_built, col):
    X, _ = synth.gaussian_sem(12, 2001, 9930)
    X[:, col] = 3.0
    ulg_ctx.load(X, 0.0)
    got = ulg_ctx.mmpc(0.01)
    assert got == oracle_built.Dataset(X).mmpc(0.01)
    assert got[col] == 0 and not any((r >> col) & 1 for r in got)
    assert sum(bin(r).count("1") for r in got) >= 10  # the other eleven keep their skeleton
