"""Parent-set constraints (score -c, ulg_cbic_set_constraints), the parts that
need no GPU: the Python restatement of the constrained scorer that the GPU
tests compare against, pinned to the oracle where there are no constraints;
the decision margin of every constrained case the GPU tests use; the
constraints-file parser through bin/constraints_dump, also built as a
stand-alone program under AddressSanitizer + UBSan.

The oracle has no constraints, so the checker is `restate_variable`: the
reference's calculateScores_internal (score_calculator.cpp:54-135),
calculateScore (BIC_OLS.cpp:174-276) and find_best_subset_score (:125-172)
statement for statement -- the zero-padded parent vector of length n, the XOR
toggle of VARSET_CLEAR, the `checked` set with the empty set pre-inserted,
float32 compares -- over the oracle's raw values (Dataset.cbic_raw), with
float32(n) substituted for a violating set (BIC_OLS.cpp:279-283)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG
import synth

F32 = np.float32
# five times the GPU tests' REL_TOL = 1e-6: a GPU score within tolerance cannot flip a decision
MARGIN_CAP = 5e-6


def satisfies(alts, P):
    """Constraints::satisfiesConstraints (constraints.h:123-139), `empty` pinned to 0."""
    if not alts:
        return True
    return any((r & ~P) == 0 and (P & f) == 0 for r, f in alts)


def alternatives_of(cons, v):
    return [(r, f) for (u, r, f) in cons if u == v]


class Restatement:
    """One variable's FloatMap under the reference's scoring loop."""

    def __init__(self, ds, lam, v, alts):
        self.ds, self.lam, self.v, self.alts = ds, lam, v, alts
        self.n = ds.n
        self.cache = {}
        self.margin = float("inf")  # smallest relative gap of a store decision

    def raw(self, P):
        # calculateScoreAndBeta (BIC_OLS.cpp:277-388): variableCount for a violator
        if not satisfies(self.alts, P):
            return F32(self.n)
        return F32(self.ds.cbic_raw(self.lam, self.v, P))

    def fbss(self, parents, pv, m, checked):
        best = F32(0.0)
        for idx in range(m):
            u = pv[idx]
            thin = parents ^ (1 << u)  # VARSET_CLEAR is an XOR (typedefs.h:657)
            if thin in checked:
                continue
            val = self.cache.get(thin)
            if val is not None:
                if val > best:
                    best = val
            else:
                npv = [0] * max(m - 1, 1)  # arma::uvec(num_parents - 1), zero-filled
                j = 0
                for i in range(m):
                    if u == pv[i]:
                        continue
                    npv[j] = pv[i]
                    j += 1
                    s = self.fbss(thin, npv, m - 1, checked)
                    checked.add(thin)
                    if s > best:
                        best = s
        return best

    def calculate_score(self, P):
        pv = [0] * self.n
        m = 0
        for i in range(self.n):
            if i != self.v and (P >> i) & 1:
                pv[m] = i
                m += 1
        ts = self.raw(P)
        if m > 0 and ts >= F32(0.0):
            return F32(-ts)
        checked = {0}
        best = self.fbss(P, pv, m, checked)
        if m > 0:
            gap = abs(float(best) - float(-ts)) / max(abs(float(ts)), 1.0)
            self.margin = min(self.margin, gap)
            if F32(best) >= F32(-ts):
                return F32(-ts)
        self.cache[P] = F32(-ts)
        return F32(-ts)

    def run(self, candidates, max_parents):
        score = self.calculate_score(0)
        if score < 1:
            self.cache[0] = score
        nbr = [i for i in range(self.n) if (candidates >> i) & 1]
        nn = len(nbr)
        for layer in range(1, max_parents + 1):
            compact = (1 << layer) - 1
            while compact < (1 << nn):
                P = 0
                for i in range(nn):
                    if (compact >> i) & 1:
                        P |= 1 << nbr[i]
                if not (P >> self.v) & 1:
                    score = self.calculate_score(P)
                    if score < 0:
                        self.cache[P] = score
                # nextPermutation (typedefs.h:692-697)
                t = (compact | (compact - 1)) + 1
                compact = t | ((((t & -t) // (compact & -compact)) >> 1) - 1)
        keys = sorted(self.cache, key=lambda s: (bin(s).count("1"), s))
        return (np.array(keys, dtype=np.uint64), np.array([self.cache[k] for k in keys], dtype=np.float32))


def restate_lists(oracle, X, lam, variables, cands, k, cons):
    """-> (offsets, sets, scores, margin) in ulg.Context.score_all's layout."""
    ds = oracle.Dataset(X)
    offs, sets, scores, margin = [0], [], [], float("inf")
    for v, c in zip(variables, cands):
        r = Restatement(ds, lam, v, alternatives_of(cons, v))
        s, sc = r.run(int(c), k)
        sets.append(s)
        scores.append(sc)
        offs.append(offs[-1] + len(s))
        margin = min(margin, r.margin)
    return np.array(offs, dtype=np.int64), np.concatenate(sets), np.concatenate(scores), margin


def bits(*vs):
    m = 0
    for v in vs:
        m |= 1 << v
    return m


def _sparse_case():
    import ulg
    n = 16
    X, W = synth.gaussian_sem(n, 2500, 9210)
    rows = synth.true_skeleton_edges(W, extra_frac=0.1, seed=3)
    cands_all = ulg.candidates_from_edges(rows, n)
    variables = [7, 0, 13, 2, 9]
    cands = [int(cands_all[v]) for v in variables]
    full = (1 << n) - 1
    # the first variable with a non-candidate requires it: every set of that variable violates
    va = next(v for v, c in zip(variables, cands) if (full & ~c & ~(1 << v)))
    ca = cands[variables.index(va)]
    outsider = next(u for u in range(n) if u != va and not (ca >> u) & 1)
    # variable 13 forbids its lowest candidate (unconstrained, its closest store
    # decision at this seed is 4.0e-6 apart, under MARGIN_CAP; with the
    # candidate forbidden that decision is gone: 1.1e-4)
    vb = 13
    cb = cands[variables.index(vb)] & ~(1 << vb)
    lowest = (cb & -cb).bit_length() - 1
    cons = [(va, bits(outsider), 0), (vb, 0, bits(lowest))]
    return dict(X=X, n=n, lam=1.0, k=4, variables=variables, cands=cands, cons=cons, all_violate=va,
                forbidden=(vb, lowest))


def _full_case(n, N, seed, k, variables, cons):
    X, _ = synth.gaussian_sem(n, N, seed)
    return dict(X=X, n=n, lam=2.0, k=k, variables=variables, cands=[(1 << n) - 1] * len(variables), cons=cons)


@functools.lru_cache(maxsize=None)
def case(name):
    """The constrained cases of the GPU tests (shape, variables, constraints)."""
    if name == "layers":  # layers 1-6: fused small layers, one-pass layer 4, two-pass 5-6
        return _full_case(12, 2000, 9201, 6, [0, 5, 11, 3], [
            (0, 0, bits(3, 8)),                                # forbidden only
            (5, bits(2), bits(7)), (5, 0, bits(0, 4, 9)),      # two alternatives; the second forbids variable 0
            (11, bits(0), 0),                                  # required only, and variable 0: the empty set violates
        ])                                                     # variable 3: no constraints, same call
    if name == "lds":  # layers 7-8: LDS bitsets
        return _full_case(9, 1500, 9202, 8, [0, 3, 8], [
            (0, 0, bits(2)),
            (3, bits(0), 0), (3, 0, bits(0, 5)),
            (8, bits(1, 6), 0),
        ])
    if name == "wide":  # layers 9-10: the wide kernels
        return _full_case(11, 800, 9204, 10, [0, 7], [
            (0, bits(3), bits(5)), (0, 0, bits(1, 2, 8)),
            (7, bits(0), bits(9)), (7, 0, bits(0, 4)),
        ])
    if name == "sparse":
        return _sparse_case()
    raise KeyError(name)


CASES = ["layers", "lds", "wide", "sparse"]


@functools.lru_cache(maxsize=None)
def e2e_case():
    """n = 8 end to end (every variable, k = 4): the variable with the most
    true parents is forbidden its strongest one, and another variable with a
    true parent is required one more, outside its true neighbourhood."""
    n, k = 8, 4
    X, W = synth.gaussian_sem(n, 2000, 9230)
    a = int(np.argmax((W != 0).sum(axis=0)))
    pa = int(np.argmax(np.abs(W[:, a])))
    adj = (W != 0) | (W.T != 0)
    reach = (W != 0)
    for _ in range(n):  # reach[i, j]: j is a descendant of i
        reach = reach | ((reach.astype(int) @ reach.astype(int)) > 0)
    # b: another variable with a true parent; u: neither adjacent to b nor its descendant
    b, u = next((v, x) for v in range(n) for x in range(n)
                if v != a and (W[:, v] != 0).any() and x != v and not adj[x, v] and not reach[v, x])
    cons = [(a, 0, bits(pa)), (b, bits(u), 0)]
    return dict(X=X, n=n, lam=2.0, k=k, variables=list(range(n)), cands=[(1 << n) - 1] * n, cons=cons,
                forbidden_edge=(pa, a), required_edge=(u, b))


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """The restatement's lists of e2e_case and the oracle's exact A* over them."""
    import oracle
    c = e2e_case()
    offs, sets, scores, margin = restate_lists(oracle, c["X"], c["lam"], c["variables"], c["cands"], c["k"], c["cons"])
    costs = np.array([oracle.quantize(float(s)) for s in scores], dtype=np.float32)
    ref = oracle.Search(c["n"], offs, sets, costs).astar(edges=c["cands"])
    return offs, sets, scores, margin, ref


@functools.lru_cache(maxsize=None)
def restated(name, constrained=True):
    """The restatement's lists of a case, computed once per session."""
    import oracle
    c = case(name)
    return restate_lists(oracle, c["X"], c["lam"], c["variables"], c["cands"], c["k"], c["cons"] if constrained else [])


def oracle_lists(oracle, c):
    ds = oracle.Dataset(c["X"])
    offs, sets, scores = [0], [], []
    for v, cand in zip(c["variables"], c["cands"]):
        s, sc = ds.score_variable(c["lam"], v, cand, c["k"])
        sets.append(s)
        scores.append(sc)
        offs.append(offs[-1] + len(s))
    return np.array(offs, dtype=np.int64), np.concatenate(sets), np.concatenate(scores)


@pytest.mark.parametrize("name", CASES)
def test_restatement_without_constraints_is_the_oracle(oracle_built, name):
    """Sets equal and scores equal as bit patterns: the checker is the oracle's scorer."""
    c = case(name)
    offs, sets, scores, _ = restated(name, False)
    o_offs, o_sets, o_scores = oracle_lists(oracle_built, c)
    assert np.array_equal(offs, o_offs)
    assert np.array_equal(sets, o_sets)
    assert np.array_equal(scores.view(np.uint32), o_scores.view(np.uint32))


@pytest.mark.parametrize("name", CASES)
def test_decision_margin_of_the_constrained_cases(oracle_built, name):
    """The smallest relative gap between best_subset_score and -the_score over
    every store decision (BIC_OLS.cpp:234) stays five times above the GPU
    tests' score tolerance, and the constraints change the lists."""
    c = case(name)
    offs, sets, scores, margin = restated(name, True)
    print(f"{name}: decision margin {margin:.3e}, {len(sets)} stored sets, "
          f"{int((scores == F32(-c['n'])).sum())} at -{c['n']}")
    assert margin >= MARGIN_CAP
    _, u_sets, _, _ = restated(name, False)
    assert not np.array_equal(sets, u_sets)
    # every stored violator holds -float(n), and nothing else does
    for i, v in enumerate(c["variables"]):
        alts = alternatives_of(c["cons"], v)
        for s, sc in zip(sets[offs[i]:offs[i + 1]], scores[offs[i]:offs[i + 1]]):
            assert (sc == F32(-c["n"])) == (not satisfies(alts, int(s)))


def test_restatement_reproduces_the_recorded_example(oracle_built):
    """n = 12, k = 6, seed 9201, variable 5 with (require a, forbid b) or
    (forbid three): the lists differ from the unconstrained ones in both
    directions."""
    c = case("layers")
    i = c["variables"].index(5)
    offs, sets, scores, _ = restated("layers", True)
    u_offs, u_sets, _, _ = restated("layers", False)
    a = set(int(x) for x in sets[offs[i]:offs[i + 1]])
    b = set(int(x) for x in u_sets[u_offs[i]:u_offs[i + 1]])
    assert a - b and b - a


def test_end_to_end_reference_respects_the_constraints(oracle_built):
    """The oracle's exact A* over the restatement's constrained lists (what the
    GPU end-to-end tests must reproduce): the forbidden edge is absent, the
    required one present, and the case's decisions clear the margin."""
    c = e2e_case()
    _, _, _, margin, ref = e2e_reference()
    print(f"e2e: decision margin {margin:.3e}, cost {ref['cost']}")
    assert margin >= MARGIN_CAP
    assert ref["rc"] == 0
    (pa, a), (u, b) = c["forbidden_edge"], c["required_edge"]
    assert not (int(ref["vpar"][a]) >> pa) & 1
    assert (int(ref["vpar"][b]) >> u) & 1


# ---- the constraints-file parser (host/io.cpp read_constraints) -----------------
DUMP = os.path.join(PKG, "bin", "constraints_dump")
SAN_DUMP = os.path.join(PKG, "bin", "san", "constraints_dump")

HEADER_CSV = "alpha,beta,gamma,delta,eps\n1,2,3,4,5\n2,3,4,5,6\n3,1,2,2,1\n"
PLAIN_CSV = "1,2,3,4,5\n2,3,4,5,6\n3,1,2,2,1\n"

# (name, constraints text, header?, expected lines or (exit status, token in the message))
PARSER_CASES = [
    ("comments_and_blanks",
     "# a comment line\n\n   \nalpha ( beta )   # trailing comment\n#gamma ( delta )\n", True, ["0 2 0"]),
    ("comma_and_space",
     "alpha,(,beta,gamma,),\nbeta ( ,, !alpha , delta )\n", True, ["0 6 0", "1 8 1"]),
    ("leading_tab_is_trimmed", "\talpha ( beta )\t\n", True, ["0 2 0"]),
    ("tab_is_no_separator", "alpha ( beta\tgamma )\n", True, (1, "beta\tgamma")),
    ("alternatives_on_one_line_and_two",
     "gamma ( alpha !beta ) ( !delta !eps )\ngamma ( eps )\n", True, ["2 1 2", "2 0 24", "2 16 0"]),
    ("nested_open_paren", "delta ( ( alpha ( beta )\n", True, ["3 3 0"]),
    ("tokens_after_last_close_dropped", "eps ( alpha ) beta !gamma\nalpha beta\n", True, ["4 1 0"]),
    ("empty_alternative", "alpha ( )\n", True, ["0 0 0"]),
    ("variable_i_names", "Variable_2 ( Variable_0 !Variable_4 )\n", False, ["2 1 16"]),
    ("header_names_unknown_without_header", "alpha ( beta )\n", False, (1, "alpha")),
    ("variable_i_unknown_with_header", "alpha ( Variable_1 )\n", True, (1, "Variable_1")),
    ("unknown_required", "alpha ( betta )\n", True, (1, "betta")),
    ("unknown_forbidden", "alpha ( beta )\nbeta ( !gama )\n", True, (1, "!gama")),
]


@functools.lru_cache(maxsize=None)
def _tools():
    subprocess.run(["make", "-C", PKG, "bin/constraints_dump", "bin/san/constraints_dump"], check=True,
                   stdout=subprocess.DEVNULL)
    return DUMP, SAN_DUMP


@pytest.mark.parametrize("tool", ["plain", "sanitized"])
@pytest.mark.parametrize("name,text,header,want", PARSER_CASES, ids=[c[0] for c in PARSER_CASES])
def test_constraints_parser(tmp_path, tool, name, text, header, want):
    """The stand-alone constraints_dump, and the same program under
    -fsanitize=address,undefined (any report aborts it)."""
    exe = _tools()[0 if tool == "plain" else 1]
    csv = tmp_path / "data.csv"
    csv.write_text(HEADER_CSV if header else PLAIN_CSV)
    cons = tmp_path / "cons.txt"
    cons.write_text(text)
    r = subprocess.run([exe, str(cons), str(csv)] + (["-s"] if header else []), capture_output=True, text=True)
    if isinstance(want, tuple):
        status, token = want
        assert r.returncode == status, r.stderr
        assert f"'{token}'" in r.stderr
        if name == "unknown_forbidden":
            assert "line 2" in r.stderr
    else:
        assert r.returncode == 0, r.stderr
        assert r.stdout.split("\n")[:-1] == want


def test_constraints_file_missing(tmp_path):
    csv = tmp_path / "data.csv"
    csv.write_text(PLAIN_CSV)
    r = subprocess.run([_tools()[0], str(tmp_path / "none.txt"), str(csv)], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr


def test_library_exports_set_constraints():
    import ulg
    assert "ulg_cbic_set_constraints" in ulg.header_symbols()
    assert hasattr(ulg.lib(), "ulg_cbic_set_constraints")
