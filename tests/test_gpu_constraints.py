"""GPU tests of parent-set constraints (ulg_cbic_set_constraints, score -c):
the constrained lists of every scorer family against the Python restatement
of the reference's constrained scorer (tests/test_constraints.py), with the
rule of test_gpu_cbic.py::_compare_lists -- stored sets identical, scores
within 1e-6 relative -- and every stored violator exactly -float(n)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, read_matrix
import synth
import test_constraints as tc

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6
SCORE = os.path.join(PKG, "bin", "score")
ASTAR = os.path.join(PKG, "bin", "astar")


def _compare(want, got, c, ctx=""):
    """want = (offsets, sets, scores) of the restatement or the oracle, got = the GPU's."""
    w_offs, w_sets, w_scores = want[:3]
    g_offs, g_sets, g_scores = got
    assert len(w_offs) == len(g_offs), ctx
    nf = np.float32(-c["n"])
    for i, v in enumerate(c["variables"]):
        a = w_sets[w_offs[i]:w_offs[i + 1]]
        b = g_sets[g_offs[i]:g_offs[i + 1]]
        if not np.array_equal(a, b):
            sa, sb = set(int(x) for x in a), set(int(x) for x in b)
            raise AssertionError(f"{ctx} variable {v}: stored sets differ: only reference {sorted(sa - sb)[:8]}, "
                                 f"only gpu {sorted(sb - sa)[:8]} ({len(a)} vs {len(b)})")
        wa = w_scores[w_offs[i]:w_offs[i + 1]]
        ga = g_scores[g_offs[i]:g_offs[i + 1]]
        err = np.abs(wa.astype(np.float64) - ga.astype(np.float64)) / np.maximum(np.abs(wa.astype(np.float64)), 1.0)
        assert err.max(initial=0.0) <= REL_TOL, f"{ctx} variable {v}: max rel score error {err.max()}"
        viol = wa == nf
        assert np.array_equal(ga[viol].view(np.uint32), wa[viol].view(np.uint32)), f"{ctx} variable {v}: violators"


def _score(ctx, c):
    offs, sets, scores = ctx.score_all(c["variables"], c["cands"], c["k"])
    assert ctx.info("score_error_word") == 0
    return np.asarray(offs).copy(), np.asarray(sets).copy(), np.asarray(scores).copy()


def _constrained(ctx, name):
    c = tc.case(name)
    ctx.load(c["X"], c["lam"])
    ctx.set_constraints(c["cons"])
    assert ctx.info("constraints") == len(c["cons"])
    try:
        return c, _score(ctx, c)
    finally:
        ctx.clear_constraints()


def test_layers_1_to_6(ulg_ctx, oracle_built):
    """The fused small layers, the one-pass layer 4 and the two-pass layers
    5-6 with bucketed walks: forbidden only (variable 0), two alternatives of
    which one forbids variable 0 (5), required only -- variable 0, so the
    empty set and every set without it are stored at -12.0 (11) -- and an
    unconstrained variable (3) in the same call."""
    c, got = _constrained(ulg_ctx, "layers")
    want = tc.restated("layers")
    _compare(want, got, c, "layers")
    i = c["variables"].index(11)
    assert int(got[1][got[0][i]]) == 0 and got[2][got[0][i]] == np.float32(-12.0)
    i = c["variables"].index(3)
    assert got[2][got[0][i]].tobytes() == np.float32(-0.0).tobytes()


def test_layers_7_and_8(ulg_ctx, oracle_built):
    c, got = _constrained(ulg_ctx, "lds")
    _compare(tc.restated("lds"), got, c, "lds")


@pytest.mark.parametrize("wide_lds", [1, 2])
def test_wide_layers(ulg_ctx, oracle_built, wide_lds):
    """Layers 9-10 through the wide kernels; wide_lds 2 sends every walk
    through the LDS replay, so that path sees the violators too."""
    ulg_ctx.set_option("wide_lds", wide_lds)
    try:
        c, got = _constrained(ulg_ctx, "wide")
    finally:
        ulg_ctx.set_option("wide_lds", 1)
    _compare(tc.restated("wide"), got, c, f"wide_lds={wide_lds}")


def test_sparse_skeleton(ulg_ctx, oracle_built):
    """2-hop candidate sets: a required non-candidate makes every set of its
    variable a violator (all stored at -16.0); another variable forbids a
    candidate."""
    c, got = _constrained(ulg_ctx, "sparse")
    _compare(tc.restated("sparse"), got, c, "sparse")
    i = c["variables"].index(c["all_violate"])
    sc = got[2][got[0][i]:got[0][i + 1]]
    m = bin(c["cands"][i] & ~(1 << c["all_violate"])).count("1")
    assert len(sc) == sum(tc_binom(m, L) for L in range(c["k"] + 1)) and (sc == np.float32(-16.0)).all()


def tc_binom(m, k):
    from math import comb
    return comb(m, k) if 0 <= k <= m else 0


@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("walk_bucket", [0, 1])
def test_state_and_paths(ulg_ctx, oracle_built, streams, walk_bucket):
    """Unconstrained, constrained, cleared on one context -- the first and
    third lists are the oracle's, the second the restatement's -- through
    ulg_cbic_score and through ulg_cbic_score_async / _finish twice in a row
    (the second call replays the captured graph)."""
    c = tc.case("layers")
    unc = tc.oracle_lists(oracle_built, c)
    con = tc.restated("layers")
    ctx = ulg_ctx
    ctx.set_option("score_streams", streams)
    ctx.set_option("walk_bucket", walk_bucket)
    try:
        ctx.load(c["X"], c["lam"])
        assert ctx.info("constraints") == 0

        def both_ways(want, tag):
            _compare(want, _score(ctx, c), c, f"{tag} sync")
            for rep in range(2):
                ctx.score_async(c["variables"], c["cands"], c["k"])
                st, _ = ctx.score_finish()
                assert ctx.info("score_error_word") == 0
                offs, sets, scores = ctx.fetch(st)
                _compare(want, (offs, sets, scores), c, f"{tag} async {rep}")

        both_ways(unc, "before")
        ctx.set_constraints(c["cons"])
        both_ways(con, "constrained")
        ctx.clear_constraints()
        assert ctx.info("constraints") == 0
        both_ways(unc, "cleared")
        # the next load drops them too
        ctx.set_constraints(c["cons"])
        ctx.load(c["X"], c["lam"])
        assert ctx.info("constraints") == 0
        _compare(unc, _score(ctx, c), c, "reloaded")
    finally:
        ctx.clear_constraints()
        ctx.set_option("score_streams", 3)
        ctx.set_option("walk_bucket", 1)


def test_score_sets_under_constraints(ulg_ctx, oracle_built):
    """ulg_cbic_score_sets: -float(n) for a violator, the empty set included;
    every other value unchanged."""
    c = tc.case("layers")
    ctx = ulg_ctx
    ctx.load(c["X"], c["lam"])
    rng = np.random.default_rng(5)
    vs, ps = [], []
    for v in c["variables"]:
        vs += [v] * 41
        ps += [0] + [int(x) & ~(1 << v) for x in rng.integers(0, 1 << c["n"], 40)]
    before = ctx.score_sets(vs, ps).copy()
    ctx.set_constraints(c["cons"])
    try:
        after = ctx.score_sets(vs, ps).copy()
    finally:
        ctx.clear_constraints()
    viol = np.array([not tc.satisfies(tc.alternatives_of(c["cons"], v), p) for v, p in zip(vs, ps)])
    assert viol.any() and (~viol).any() and viol[vs.index(11)]  # variable 11's empty set violates
    assert (after[viol] == np.float32(-c["n"])).all()
    assert after[~viol].tobytes() == before[~viol].tobytes()
    assert ctx.score_sets(vs, ps).tobytes() == before.tobytes()  # cleared


def test_argument_errors(ulg_ctx):
    import ctypes as C
    import ulg
    L = ulg.lib()
    n = 6
    X, _ = synth.gaussian_sem(n, 300, 9240)
    fresh = ulg.Context(0)
    try:
        with pytest.raises(ulg.ULGError, match="status 1"):  # ULG_ERR_ARG: nothing loaded
            fresh.set_constraints([(0, 2, 0)])
    finally:
        fresh.close()
    ctx = ulg_ctx
    ctx.load(X, 2.0)
    with pytest.raises(ulg.ULGError, match="status 1"):
        ctx.set_constraints([(0, 1 << n, 0)])
    with pytest.raises(ulg.ULGError, match="status 1"):
        ctx.set_constraints([(0, 0, 1 << 40)])
    with pytest.raises(ulg.ULGError, match="status 1"):
        ctx.set_constraints([(n, 1, 0)])
    with pytest.raises(ulg.ULGError, match="status 1"):
        ctx.set_constraints([(-1, 1, 0)])
    ctx.set_constraints([(2, 1, 0)] * 64)
    assert ctx.info("constraints") == 64
    with pytest.raises(ulg.ULGError, match="status 4"):  # ULG_ERR_UNSUPPORTED
        ctx.set_constraints([(2, 1, 0)] * 65)
    assert ctx.info("constraints") == 64  # a refused call changes nothing
    ctx.clear_constraints()
    assert ctx.info("constraints") == 0
    assert L.ulg_cbic_set_constraints(None, 0, None, None, None) == 1


def test_many_alternatives_read_from_global_memory(ulg_ctx, oracle_built):
    """A table too large for the kernels' LDS copy (64 alternatives on each
    of three variables): the same lists as the restatement's."""
    c = dict(tc.case("lds"))
    rng = np.random.default_rng(11)
    cons = []
    for v in c["variables"]:
        for _ in range(64):
            r, f = (int(x) for x in rng.integers(0, 1 << c["n"], 2))
            cons.append((v, r & ~f & ~(1 << v) & int(rng.integers(0, 1 << c["n"])), f))
    c["cons"] = cons
    want = tc.restate_lists(oracle_built, c["X"], c["lam"], c["variables"], c["cands"], c["k"], cons)
    print(f"many alternatives: decision margin {want[3]:.3e}")
    assert want[3] >= tc.MARGIN_CAP
    ulg_ctx.load(c["X"], c["lam"])
    ulg_ctx.set_constraints(cons)
    try:
        got = _score(ulg_ctx, c)
    finally:
        ulg_ctx.clear_constraints()
    _compare(want, got, c, "many")


def test_end_to_end_search(ulg_ctx, oracle_built):
    """n = 8: constrained lists, search_from_scores, the exact A*: the DAG and
    cost of the oracle's A* over the restatement's lists; the forbidden edge
    absent, the required one present."""
    c = tc.e2e_case()
    offs, sets, scores, _, ref = tc.e2e_reference()
    ctx = ulg_ctx
    ctx.load(c["X"], c["lam"])
    ctx.set_constraints(c["cons"])
    try:
        got = _score(ctx, c)
        _compare((offs, sets, scores), got, c, "e2e")
        ctx.search_from_scores()
        res = ctx.astar(edges=c["cands"], mode=0, net_text=False)
    finally:
        ctx.clear_constraints()
    assert [int(x) for x in res["vpar"]] == [int(x) for x in ref["vpar"]]
    assert np.float32(res["cost"]).tobytes() == np.float32(ref["cost"]).tobytes()
    (pa, a), (u, b) = c["forbidden_edge"], c["required_edge"]
    assert not (int(res["vpar"][a]) >> pa) & 1 and (int(res["vpar"][b]) >> u) & 1


def test_cli_score_with_constraints_file(tmp_path, oracle_built):
    """bin/score -c: the .pss oracle.write_pss produces from the restatement's
    lists, byte for byte after the META header; bin/astar on it gives the
    end-to-end DAG."""
    o = oracle_built
    c = tc.e2e_case()
    offs, sets, scores, _, ref = tc.e2e_reference()
    n = c["n"]
    csv = tmp_path / "data.csv"
    synth.write_csv(str(csv), c["X"])
    names = [f"Variable_{i}" for i in range(n)]
    lines = ["# forbidden and required parents"]
    for v, r, f in c["cons"]:
        toks = [names[i] for i in range(n) if (r >> i) & 1] + ["!" + names[i] for i in range(n) if (f >> i) & 1]
        lines.append(f"{names[v]} ( {', '.join(toks)} )")
    cons = tmp_path / "cons.txt"
    cons.write_text("\n".join(lines) + "\n")
    pss, ref_pss = tmp_path / "gpu.pss", tmp_path / "ref.pss"
    r = subprocess.run([SCORE, str(csv), str(pss), "-f", "cBIC", "--lambda", "2", "-p", "4", "-c", str(cons)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert f"Constraints file: '{cons}'" in r.stdout
    cols = [ln.split(",") for ln in csv.read_text().splitlines() if ln]
    arity = [len(set(row[j] for row in cols)) for j in range(n)]
    o.write_pss(str(ref_pss), names, arity, offs, sets, scores, input_file=str(csv), num_records=len(cols),
                parent_limit=4)
    body = lambda p: p.read_text().split("\n\n", 1)[1]
    assert body(pss) == body(ref_pss)
    net = tmp_path / "net"
    r = subprocess.run([ASTAR, str(pss), "-n", str(net)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert read_matrix(str(net) + ".csv") == o.dag_matrix(ref["vpar"], n).tolist()
    # an unknown name is refused before any scoring
    cons.write_text("Variable_1 ( Variabel_2 )\n")
    r = subprocess.run([SCORE, str(csv), str(pss), "-f", "cBIC", "--lambda", "2", "-c", str(cons)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "'Variabel_2'" in r.stderr and "line 1" in r.stderr
