"""The contract of the order MCMC's log-sum tables (include/ulg.h, "Order MCMC over log-sum tables"; the
kernels are csrc/order_sumtables.hip) restated in numpy.  No GPU, no project binding.

  table    L_v over the subsets of C_v = the OR of v's stored sets: slot idx_v(P_i) = float64(s_i), the
           rest -inf, then for j = 0 .. K_v - 1 ascending every slot with bit j becomes
           logaddexp(L[x], L[x ^ 2^j]) = max + log1p(exp(-gap)), the maximum itself when the smaller is
           -inf or the gap exceeds 38.  butterfly() does that in float64, direct() sums exp in long double.
  chain    order_mcmc_ref's draws, accept rule and picks, with the term of position p read from a GIVEN
           table, L_v[idx_v(pre_p)], and every sum a float64 add in ascending order (run()).

SLOT CAP.  logaddexp(a, b) has partial derivatives e^a / (e^a + e^b) and e^b / (e^a + e^b): positive, sum 1.
A round therefore passes its inputs' errors on as a weighted mean -- at most the larger of the two -- and
adds its own:
    d = hi - lo             rounded: 2^-53 d, which moves log1p(exp(-d)) by d e^-d 2^-53 <= 0.37 2^-53 < 2^-54
    exp(-d) <= 1            4 ulp allowed to OCML (as posterior_sample_ref allows), an ulp at most 2^-52 of
                            the value, and log1p's derivative is at most 1:        4 2^-52
    log1p(y) <= ln 2        4 ulp of a value below 1:                              4 2^-53
    hi + ..                 the add's rounding:                                    ulp(L) / 2
    the cut                 log1p(exp(-d)) left out for d > 38:                    e^-38
A slot is the root of a tree of depth at most K_v, so
    |L_dev - L_true| <= K_v (6.25 2^-52 + ulp(L) / 2 + e^-38) =: slot_cap,
ulp(L) taken at the largest magnitude on the way: every intermediate value is a log-sum of some of the
compatible scores, so it lies between their least and the slot's own value (big below).  A slot with one
compatible entry is that score's bits, one with none is -inf: the tests ask for equality there.

DELTA.  The GPU tests run run() on the device's own read-back tables: delta is then IEEE adds of the same
doubles in the same order and must be equal bit for bit, and a decision is re-derived from it with exp's
8-unit margin alone.  Whether a seed's steps keep that margin for ANY table within slot_cap is what
tests/test_order_sumtables_ref.py asserts on butterfly()'s tables with caps passed to run(): delta_cap = the
sum of the 2 cnt slot caps + cnt ulp(sum |a'_p|) + cnt ulp(sum |a_p|) + ulp(delta), as order_mcmc_ref's."""
import functools
import math

import numpy as np

import order_mcmc_ref as om

LD, U64 = np.longdouble, np.uint64
CUT = 38.0
ROUND_CAP = 6.25 * 2.0 ** -52 + math.exp(-38.0)


def members(C):
    return [u for u in range(64) if (int(C) >> u) & 1]


def index(mem, U):
    """idx_v(U): the bits of U at the candidates `mem`, squeezed together."""
    return sum(1 << r for r, u in enumerate(mem) if (int(U) >> u) & 1)


def logaddexp(a, b):
    """post_logaddexp on float64 arrays."""
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore"):
        d = hi - lo
    plain = ~(lo > -np.inf) | ~(d <= CUT)
    return np.where(plain, hi, hi + np.log1p(np.exp(-np.where(plain, 0.0, d))))


def butterfly(L, v):
    """-> (C_v, float64 table of 2^K_v slots) by the contract's rounds."""
    C = int(np.bitwise_or.reduce(L.sets[v])) if len(L.sets[v]) else 0
    mem = members(C)
    T = np.full(1 << len(mem), -np.inf)
    T[[index(mem, S) for S in L.sets[v]]] = L.sc[v]
    for j in range(len(mem)):
        W = T.reshape(-1, 2, 1 << j)
        W[:, 1, :] = logaddexp(W[:, 1, :], W[:, 0, :])
    return C, T


def direct(L, v):
    """-> (value longdouble: ln sum exp(s_i) over the entries inside each slot's subset, count of those
    entries, cap float64: slot_cap), by slot."""
    S, sc = L.sets[v], L.sc[v]
    mem = members(int(np.bitwise_or.reduce(S)) if len(S) else 0)
    x = np.arange(1 << len(mem), dtype=np.uint64)
    U = np.zeros(len(x), dtype=np.uint64)
    for r, u in enumerate(mem):
        U |= ((x >> U64(r)) & U64(1)) << U64(u)
    top = sc.max() if len(sc) else 0.0
    w = np.exp(sc.astype(LD) - LD(top))  # scores span far less than long double's range
    tot, count, mag = np.zeros(len(x), dtype=LD), np.zeros(len(x), dtype=np.int64), np.zeros(len(x))
    for i in range(len(S)):  # entry by entry: a few hundred passes over the slots
        inside = (S[i] & ~U) == U64(0)
        tot[inside] += w[i]
        count += inside
        mag = np.where(inside, np.maximum(mag, abs(sc[i])), mag)
    with np.errstate(divide="ignore"):
        val = LD(top) + np.log(tot)
    big = np.maximum(np.abs(np.where(count > 0, val, 0).astype(np.float64)), mag)
    cap = len(mem) * (ROUND_CAP + np.spacing(np.where(count > 0, big, 1.0)) / 2)
    return np.where(count > 0, val, LD(-np.inf)), count, cap


def run(L, tables, seed, chains, steps, thin, order=None, t0=0, caps=None):
    """`chains` chains for `steps` steps after step t0 with the terms taken from tables[v] = (C_v, float64
    slots); order: where to continue from, else the shuffle.  caps[v]: slot caps, for a delta cap (else the
    decisions allow exp's 8 units alone).  -> dict as order_mcmc_ref.run's, float64 throughout, with
    min_excess = the least margin - slack over the decisions and picks."""
    n, cs = L.n, np.arange(chains, dtype=np.int64)
    order = om.shuffle(seed, cs, n) if order is None else np.array(order, dtype=np.int64)
    mem = [members(C) for C, _ in tables]

    def look(v, U):
        x = index(mem[v], U)
        return tables[v][1][x], (caps[v][x] if caps is not None else 0.0)

    pre = om.prefixes(order)
    term = np.array([[look(v, U)[0] for v, U in zip(o, p)] for o, p in zip(order, pre)])
    tcap = np.array([[look(v, U)[1] for v, U in zip(o, p)] for o, p in zip(order, pre)])
    assert np.all(term > -np.inf)
    out = {k: [] for k in ("order", "log_score", "parents", "log_weight")}
    tr_delta, tr_acc = np.full((steps, chains), -np.inf), np.zeros((steps, chains), dtype=np.uint8)
    accepted, min_excess = np.zeros(chains, dtype=np.int64), 1 << 62
    for s in range(steps):
        t = t0 + s + 1
        i, j, u_acc = om.moves(seed, t, cs, n) if n > 1 else ([], [], [])
        for c in range(chains if n > 1 else 0):
            lo, hi = int(min(i[c], j[c])), int(max(i[c], j[c]))
            o, p = order[c].copy(), pre[c].copy()
            flip = (U64(1) << U64(o[lo])) ^ (U64(1) << U64(o[hi]))
            o[lo], o[hi] = o[hi], o[lo]
            p[lo + 1:hi + 1] ^= flip
            fresh = [look(o[q], p[q]) for q in range(lo, hi + 1)]
            now = was = 0.0
            for (x, _), q in zip(fresh, range(lo, hi + 1)):
                now, was = now + x, was + term[c, q]
            dead = not now > -np.inf
            delta = -np.inf if dead else now - was
            dcap = None
            if caps is not None and not dead:
                cnt = hi - lo + 1
                dcap = (sum(e for _, e in fresh) + tcap[c, lo:hi + 1].sum() + np.spacing(abs(delta))
                        + cnt * (np.spacing(sum(abs(x) for x, _ in fresh)) + np.spacing(np.abs(term[c, lo:hi + 1]).sum())))
            acc, margin, slack = om.decide(np.array([delta]), None if dcap is None else np.array([dcap]), u_acc[c:c + 1])
            min_excess = min(min_excess, int(margin[0] - slack[0]))
            tr_delta[s, c], tr_acc[s, c] = delta, acc[0]
            if acc[0]:
                order[c], pre[c] = o, p
                term[c, lo:hi + 1], tcap[c, lo:hi + 1] = [x for x, _ in fresh], [e for _, e in fresh]
                accepted[c] += 1
        if t % thin == 0:
            out["order"].append(order.astype(np.uint8))
            out["log_score"].append(np.array([functools.reduce(lambda a, b: a + b, row, 0.0) for row in term]))
            ci, pi = np.nonzero(np.ones((chains, n), dtype=bool))
            w = om._draw(seed, t, cs[ci], 1 + pi)
            e, margin, slack = om.picks(L, order[ci, pi], pre[ci, pi], term[ci, pi].astype(LD), tcap[ci, pi], w[0] | (w[1] << U64(32)))
            min_excess = min(min_excess, int((margin - slack).min()))
            par, chosen = np.zeros((chains, n), dtype=np.uint64), np.zeros((chains, n))
            par[ci, order[ci, pi]], chosen[ci, order[ci, pi]] = L.sets_all[e], L.scores_all[e].astype(np.float64)
            out["parents"].append(par)
            out["log_weight"].append(np.array([functools.reduce(lambda a, b: a + b, row, 0.0) for row in chosen]))
    out = {k: np.stack(x) for k, x in out.items() if x}
    out.update(trace_delta=tr_delta, trace_accept=tr_acc, accepted=accepted, final_order=order.astype(np.uint8), final_terms=term,
               min_excess=min_excess)
    return out


STEPS, THIN, CHAINS = 150, 10, 4


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """n -> (Lists, seed) of the GPU chain tests: order_mcmc_ref's where every K_v fits a table (n = 5: K = 4,
    n = 8: K = 7), the order-table tests' pooled lists beyond (n = 33: K = 5; n = 63: K = 13, 14, 15 and 4)."""
    from test_gpu_order_tables import inputs
    return {5: om.chain_inputs()["full-5"], 8: om.chain_inputs()["k3-8"], 33: (inputs()["n33"][0], 7), 63: (inputs()["n63"][0], 9)}
