"""The order MCMC's contract (include/ulg.h, "Order MCMC"; the kernels are
csrc/order_mcmc.hip) restated in Python integers and numpy.longdouble.  No GPU,
no project binding.  It reuses posterior_sample_ref's Philox and its margin
idea.

  term     a_v(U): m = the maximum of float64(s_i) over the entries with
           P_i subset of U; q_i = floor(exp(s_i - m) 2^52), exp in long double
           here; T = sum q_i, an exact integer; a = m + log(T 2^-52) in long
           double.  -inf without a compatible entry.
  draws    Philox4x32-10, key (lo32(seed), hi32(seed)), counter (lo32(t),
           hi32(t), c, d).  Shuffle: t = 0, d = p for p = n-1 .. 1,
           r = mulhi32(w0, p+1).  Move: d = 0, i = mulhi32(w0, n), j' =
           mulhi32(w1, n-1), j = j' + (j' >= i), U_acc = w2 | w3 << 32.
           Parent set of position p of a record: d = 1 + p, U_set = w0 | w1 << 32.
  accept   delta = (sum of the new terms of lo..hi) - (sum of the old ones);
           -inf when a new term is; accepted iff (U_acc >> 12) < q_eff,
           q_eff = 2^52 for delta >= 0 (always), floor(exp(delta) 2^52) below.
  record   at t mod thin = 0: the order, the sum of the terms, and per position
           the sampler's pick over x_i = s_i - a_p.

What the device may differ by, and the caps the GPU tests hold it to.  None is
measured on the device.

TERM CAP.  OCML documents at most 1 ulp for its FP64 exp and log (the library's
claim); 4 are allowed, as posterior_sample_ref allows.  A product exp(x) 2^52 is
at most 2^52, where an ulp is at most one unit: a q moves by at most 4 units,
one more for the floor, 8 are taken, for each of the k entries that count
(exp(x) 2^52 >= 1/2 here: one floored to 0 from just below 1 may be 1 there).
T >= 2^52 because the maximum's own weight is exactly 2^52.  So
    |a_dev - a_ref| <= 8 k / T                 the weights, relative to T, on a logarithm
                     + 2^-52                   y: the conversion of T_lo and the add, 2^-53 each, relative
                     + 4 ulp(log y)            the device's log
                     + ulp(a)                  the last add's rounding, and this module's own to FP64
                   =: term_cap (cap_of below; ulp(x) = numpy.spacing(|x|)).
A term with one compatible entry has T = 2^52, y = 1, log y = 0: the device's
value is the score itself and the test asks for equality, not for the cap.

DELTA CAP.  delta adds cnt = hi - lo + 1 new terms and as many old ones in FP64
and subtracts: the terms' own caps, half an ulp of the partial sum per add
(bounded by ulp of the sum of the |a_p|), and the subtraction's:
    delta_cap = sum of the 2 cnt term caps + cnt ulp(sum |a'_p|) + cnt ulp(sum |a_p|) + ulp(delta).
log_score's cap is the same with n old terms alone.

UNDECIDED.  A step is decided by u = U_acc >> 12 against q_eff.  With the
device's own delta bits exp moves q by at most 8 units (above): the GPU test
re-derives every decision from the trace's delta and asserts that margin.  This
module's delta differs from the device's by up to delta_cap, which moves q by
q delta_cap more: a step of run() whose distance from u to the threshold is
below 8 + ceil(q_eff delta_cap) + 1 is UNDECIDED (the device may decide either
way and meet the contract).  A set pick is the sampler's: 8 (m + 1) units for
its m candidates' weights, and the term a_p under them is the device's within
term_cap, which moves every running sum and the threshold by at most
T term_cap each: slack = 8 (m + 1) + 2 ceil(T term_cap) + 2.
tests/test_order_mcmc_ref.py asserts that no input and seed of the GPU tests
has an undecided step (about 1e-11 per step), so those tests demand equality.
"""
import itertools
import math

import numpy as np

import posterior_sample_ref as ps

LD = np.longdouble
M32 = 0xFFFFFFFF
WEIGHT_BITS = 52
ONE = 1 << WEIGHT_BITS
ULP_ALLOWANCE = 8
U64 = np.uint64


# ---- lists -------------------------------------------------------------------------
class Lists:
    """Per-variable views of (offsets, sets, scores): sets uint64, scores float64 of the float32 values."""

    def __init__(self, n, offsets, sets, scores):
        self.n = n
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.sets_all = np.asarray(sets, dtype=np.uint64)
        self.scores_all = np.asarray(scores, dtype=np.float32)
        self.sets = [self.sets_all[self.offsets[v]:self.offsets[v + 1]] for v in range(n)]
        self.sc = [self.scores_all[self.offsets[v]:self.offsets[v + 1]].astype(np.float64) for v in range(n)]

    def triple(self):
        return self.offsets, self.sets_all, self.scores_all


def cap_of(a, logy, k, T):
    """term_cap (module docstring) of terms a = m + logy with k counted entries and sum T; arrays."""
    a64 = np.abs(np.asarray(a, dtype=np.float64))
    return (ULP_ALLOWANCE * np.asarray(k, dtype=np.float64) / np.asarray(T, dtype=np.float64) + 2.0 ** -52
            + 4 * np.spacing(np.abs(np.asarray(logy, dtype=np.float64))) + np.spacing(a64))


def terms(L, vs, Us, sums=None):
    """The terms of the pairs (variable vs[r], predecessor set Us[r]).  -> (a longdouble, cap float64,
    single bool: one compatible entry, the value is then the score exactly); a = -inf, cap = 0 where no
    entry is compatible.  sums: a list of len(vs) that receives each pair's T as a Python integer (0 without
    a compatible entry), so that T_hi = T >> 64 can be asked for."""
    vs = np.asarray(vs, dtype=np.int64)
    Us = np.asarray(Us, dtype=np.uint64)
    a = np.full(len(vs), -np.inf, dtype=LD)
    cap = np.zeros(len(vs), dtype=np.float64)
    single = np.zeros(len(vs), dtype=bool)
    if sums is not None:
        sums[:] = [0] * len(vs)
    for v in np.unique(vs):
        rows = np.flatnonzero(vs == v)
        S, sc = L.sets[v], L.sc[v]
        if len(S) == 0:
            continue
        compat = (S[None, :] & ~Us[rows][:, None]) == U64(0)
        some = compat.any(axis=1)
        m = np.where(compat, sc[None, :], -np.inf).max(axis=1)
        m0 = np.where(some, m, 0.0)
        with np.errstate(under="ignore"):
            val = np.exp(sc.astype(LD)[None, :] - m0.astype(LD)[:, None]) * LD(ONE)
        val = np.where(compat, val, LD(0))
        q = np.floor(val).astype(np.uint64)
        # exact: the high and low halves summed apart (a list of more than 4096 maximal entries passes 2^64)
        hi = (q >> U64(32)).sum(axis=1, dtype=np.uint64)
        lo = (q & U64(M32)).sum(axis=1, dtype=np.uint64)
        if sums is not None:
            for r, h, l, ok in zip(rows, hi, lo, some):
                sums[r] = ((int(h) << 32) + int(l)) if ok else 0
        y = hi.astype(LD) * LD(2.0 ** (32 - WEIGHT_BITS)) + lo.astype(LD) * LD(2.0 ** -WEIGHT_BITS)
        y = np.where(some, y, LD(1))
        logy = np.log(y)
        k = (val >= 0.5).sum(axis=1)
        av = m0.astype(LD) + logy
        a[rows] = np.where(some, av, LD(-np.inf))
        cap[rows] = np.where(some, cap_of(av, logy, k, y.astype(np.float64) * ONE), 0.0)
        single[rows] = compat.sum(axis=1) == 1
    return a, cap, single


def prefixes(order):
    """pre[c, p] = the mask of the variables before position p of order[c]; order int (C, n) -> uint64 (C, n)."""
    order = np.asarray(order, dtype=np.int64)
    bits = U64(1) << order.astype(np.uint64)
    pre = np.zeros(order.shape, dtype=np.uint64)
    if order.shape[1] > 1:
        pre[:, 1:] = np.bitwise_or.accumulate(bits[:, :-1], axis=1)
    return pre


def order_terms(L, orders, sums=None):
    """terms of every position of every order: orders int (K, n) -> (a longdouble (K, n), cap, single);
    sums as in terms(), in (order, position) order."""
    orders = np.asarray(orders, dtype=np.int64)
    a, cap, single = terms(L, orders.ravel(), prefixes(orders).ravel(), sums)
    return a.reshape(orders.shape), cap.reshape(orders.shape), single.reshape(orders.shape)


# ---- draws -------------------------------------------------------------------------
def _draw(seed, t, cs, d):
    """Philox words (w0..w3) as uint64 arrays for chains cs at step t, domain d (scalar or array)."""
    cs = np.asarray(cs, dtype=np.uint64)
    d = np.broadcast_to(np.asarray(d, dtype=np.uint64), cs.shape)
    t0 = np.full(cs.shape, t & M32, dtype=np.uint64)
    t1 = np.full(cs.shape, (t >> 32) & M32, dtype=np.uint64)
    return ps._philox_np(t0, t1, cs, d, seed & M32, (seed >> 32) & M32)


def mulhi32(w, m):
    return ((np.asarray(w, dtype=np.uint64) * U64(m)) >> U64(32)).astype(np.int64)


def shuffle(seed, cs, n):
    """The initial orders of chains cs: int64 (C, n)."""
    cs = np.asarray(cs, dtype=np.int64)
    order = np.tile(np.arange(n, dtype=np.int64), (len(cs), 1))
    rows = np.arange(len(cs))
    for p in range(n - 1, 0, -1):
        r = mulhi32(_draw(seed, 0, cs, p)[0], p + 1)
        x = order[rows, p].copy()
        order[rows, p] = order[rows, r]
        order[rows, r] = x
    return order


def moves(seed, t, cs, n):
    """-> (i, j int64, u_acc uint64) of step t for chains cs, n >= 2."""
    w = _draw(seed, t, cs, 0)
    i = mulhi32(w[0], n)
    jp = mulhi32(w[1], n - 1)
    return i, jp + (jp >= i), w[2] | (w[3] << U64(32))


def weight_q(x):
    """floor(exp(x) 2^52) of a longdouble / float64 array as int64 (0 for -inf), and the values before the floor."""
    x = np.asarray(x, dtype=LD)
    with np.errstate(under="ignore"):
        val = np.where(x > -np.inf, np.exp(x) * LD(ONE), LD(0))
    return np.floor(val).astype(np.uint64).astype(np.int64), val


def mulhi64(U, T):
    """(U T) >> 64 elementwise for uint64 arrays (T < 2^63), as int64."""
    m, s = U64(M32), U64(32)
    U, T = np.asarray(U, dtype=np.uint64), np.asarray(T, dtype=np.uint64)
    u0, u1, t0, t1 = U & m, U >> s, T & m, T >> s
    p00, p01, p10, p11 = u0 * t0, u0 * t1, u1 * t0, u1 * t1
    mid = (p00 >> s) + (p01 & m) + (p10 & m)
    return (p11 + (p01 >> s) + (p10 >> s) + (mid >> s)).astype(np.int64)


def decide(delta, delta_cap, u_acc, allowance=ULP_ALLOWANCE):
    """The accept rule on deltas (longdouble or float64 array; -inf: a new term of -inf).
    -> (accept bool, margin int64: the distance of u = U_acc >> 12 to the value that decides otherwise,
    slack int64: allowance + ceil(q_eff delta_cap) + 1, or just `allowance` for delta_cap None).  A
    delta of -inf is decided by integers alone: margin 2^52, slack 0."""
    delta = np.asarray(delta, dtype=LD)
    u = (np.asarray(u_acc, dtype=np.uint64) >> U64(12)).astype(np.int64)
    dead = ~(delta > -np.inf)
    q, _ = weight_q(np.where((delta < 0) & ~dead, delta, LD(0)))  # delta >= 0: q_eff = 2^52
    q = np.where(dead, 0, q)
    accept = (u < q) & ~dead
    margin = np.where(dead, ONE, np.where(accept, q - u, u - q + 1))
    if delta_cap is None:
        slack = np.where(dead, 0, allowance)
    else:
        slack = np.where(dead, 0, allowance + np.ceil(q.astype(np.float64) * np.asarray(delta_cap)).astype(np.int64) + 1)
    return accept, margin, slack


def picks(L, vs, Us, a, a_cap, u_set):
    """The parent-set pick of each row: variable vs[r] with predecessors Us[r], term a[r] (longdouble),
    draw u_set[r].  -> (entry int64: the index into the lists, margin, slack int64)."""
    vs = np.asarray(vs, dtype=np.int64)
    entry = np.zeros(len(vs), dtype=np.int64)
    margin = np.zeros(len(vs), dtype=np.int64)
    slack = np.zeros(len(vs), dtype=np.int64)
    for v in np.unique(vs):
        rows = np.flatnonzero(vs == v)
        S, sc = L.sets[v], L.sc[v]
        compat = (S[None, :] & ~Us[rows][:, None]) == U64(0)
        with np.errstate(under="ignore"):
            val = np.exp(sc.astype(LD)[None, :] - np.asarray(a, dtype=LD)[rows][:, None]) * LD(ONE)
        val = np.where(compat, val, LD(0))
        q = np.floor(val).astype(np.uint64).astype(np.int64)
        Cs = np.cumsum(q, axis=1)
        T = Cs[:, -1]
        assert np.all(T > 0), "a set step without a candidate"
        t = mulhi64(u_set[rows], T.astype(np.uint64))
        j = (Cs > t[:, None]).argmax(axis=1)
        r = np.arange(len(rows))
        low = np.where(j > 0, Cs[r, np.maximum(j - 1, 0)], 0)
        entry[rows] = L.offsets[v] + j
        margin[rows] = np.minimum(t - low, Cs[r, j] - t)
        m = (val >= 0.5).sum(axis=1)
        slack[rows] = ULP_ALLOWANCE * (m + 1) + 2 * np.ceil(T.astype(np.float64) * a_cap[rows]).astype(np.int64) + 2
    return entry, margin, slack


# ---- the chains --------------------------------------------------------------------
def run(L, seed, chains, steps, thin=1, init_order=None, want_parents=True, t0=0, state=None):
    """`chains` chains (indices 0 .. chains-1, or the array given) for `steps` steps after step t0.
    state: (order, ) of an earlier run to continue from; else init_order int (C, n) or the shuffle.
    -> dict: order (R, C, n) uint8, log_score (R, C) longdouble, score_cap (R, C), parents (R, C, n)
    uint64, log_weight (R, C) float64, entry (R, C, n), accepted (C) int64 (of these steps), trace_delta
    (steps, C) longdouble, trace_cap, trace_accept (steps, C) bool, final_order (C, n), final_terms,
    final_cap, undecided: the steps and picks whose margin is below their slack, min_excess: the least
    margin - slack."""
    n = L.n
    cs = np.arange(chains, dtype=np.int64) if np.isscalar(chains) else np.asarray(chains, dtype=np.int64)
    C = len(cs)
    if state is not None:
        order = np.array(state, dtype=np.int64)
    elif init_order is not None:
        order = np.array(init_order, dtype=np.int64)
    else:
        order = shuffle(seed, cs, n)
    pre = prefixes(order)
    term, tcap, _ = order_terms(L, order)
    assert np.all(term > -np.inf), "an initial order with a -inf term"
    P = np.arange(n)[None, :]
    rows = np.arange(C)
    rec = {k: [] for k in ("order", "log_score", "score_cap", "parents", "log_weight", "entry")}
    tr_delta = np.full((steps, C), -np.inf, dtype=LD)
    tr_cap = np.zeros((steps, C), dtype=np.float64)
    tr_acc = np.zeros((steps, C), dtype=bool)
    accepted = np.zeros(C, dtype=np.int64)
    undecided, min_excess = 0, 1 << 62
    for s in range(steps):
        t = t0 + s + 1
        if n > 1:
            i, j, u_acc = moves(seed, t, cs, n)
            lo, hi = np.minimum(i, j), np.maximum(i, j)
            va, vb = order[rows, lo], order[rows, hi]
            flip = (U64(1) << va.astype(np.uint64)) ^ (U64(1) << vb.astype(np.uint64))
            new_order = order.copy()
            new_order[rows, lo], new_order[rows, hi] = vb, va
            inner = (P > lo[:, None]) & (P <= hi[:, None])
            new_pre = np.where(inner, pre ^ flip[:, None], pre)
            touched = (P >= lo[:, None]) & (P <= hi[:, None])
            ci, pi = np.nonzero(touched)
            fa, fc, _ = terms(L, new_order[ci, pi], new_pre[ci, pi])
            fresh = np.zeros((C, n), dtype=LD)
            fcap = np.zeros((C, n), dtype=np.float64)
            fresh[ci, pi], fcap[ci, pi] = fa, fc
            now, was = np.zeros(C, dtype=LD), np.zeros(C, dtype=LD)
            mag_now, mag_was, caps = np.zeros(C), np.zeros(C), np.zeros(C)
            with np.errstate(invalid="ignore"):
                for p in range(n):
                    on = touched[:, p]
                    now = np.where(on, now + fresh[:, p], now)
                    was = np.where(on, was + term[:, p], was)
                    finite = on & (fresh[:, p] > -np.inf)
                    mag_now += np.where(finite, np.abs(fresh[:, p].astype(np.float64)), 0.0)
                    mag_was += np.where(on, np.abs(term[:, p].astype(np.float64)), 0.0)
                    caps += np.where(on, fcap[:, p] + tcap[:, p], 0.0)
                dead = ~(now > -np.inf)
                delta = np.where(dead, LD(-np.inf), now - was)
            cnt = (hi - lo + 1).astype(np.float64)
            dcap = np.where(dead, 0.0, caps + cnt * (np.spacing(mag_now) + np.spacing(mag_was))
                            + np.spacing(np.abs(np.where(dead, 0.0, delta.astype(np.float64)))))
            acc, margin, slack = decide(delta, dcap, u_acc)
            undecided += int((margin < slack).sum())
            min_excess = min(min_excess, int((margin - slack).min()))
            tr_delta[s], tr_cap[s], tr_acc[s] = delta, dcap, acc
            take = acc[:, None]
            order = np.where(take, new_order, order)
            pre = np.where(take, new_pre, pre)
            term = np.where(take & touched, fresh, term)
            tcap = np.where(take & touched, fcap, tcap)
            accepted += acc
        if t % thin == 0:
            rec["order"].append(order.astype(np.uint8))
            tot, mag = np.zeros(C, dtype=LD), np.zeros(C)
            for p in range(n):
                tot = tot + term[:, p]
                mag += np.abs(term[:, p].astype(np.float64))
            rec["log_score"].append(tot)
            rec["score_cap"].append(tcap.sum(axis=1) + n * np.spacing(mag))
            if want_parents:
                ci, pi = np.nonzero(np.ones((C, n), dtype=bool))
                w = _draw(seed, t, cs[ci], 1 + pi)
                u_set = w[0] | (w[1] << U64(32))
                e, margin, slack = picks(L, order[ci, pi], pre[ci, pi], term[ci, pi], tcap[ci, pi], u_set)
                undecided += int((margin < slack).sum())
                min_excess = min(min_excess, int((margin - slack).min()))
                par = np.zeros((C, n), dtype=np.uint64)
                chosen = np.zeros((C, n), dtype=np.float64)
                ent = np.zeros((C, n), dtype=np.int64)
                par[ci, order[ci, pi]] = L.sets_all[e]
                chosen[ci, order[ci, pi]] = L.scores_all[e].astype(np.float64)
                ent[ci, pi] = e
                lw = np.zeros(C, dtype=np.float64)
                for v in range(n):
                    lw = lw + chosen[:, v]
                rec["parents"].append(par)
                rec["log_weight"].append(lw)
                rec["entry"].append(ent)
    out = {}
    shapes = {"order": ((0, C, n), np.uint8), "log_score": ((0, C), LD), "score_cap": ((0, C), np.float64),
              "parents": ((0, C, n), np.uint64), "log_weight": ((0, C), np.float64), "entry": ((0, C, n), np.int64)}
    for k, v in rec.items():
        out[k] = np.stack(v) if v else np.zeros(*shapes[k])
    out.update(accepted=accepted, trace_delta=tr_delta, trace_cap=tr_cap, trace_accept=tr_acc, final_order=order,
               final_terms=term, final_cap=tcap, undecided=undecided, min_excess=min_excess, records=len(rec["order"]))
    return out


# ---- exact laws, by enumeration ----------------------------------------------------
def order_law(L):
    """(perms: list of tuples, pi longdouble: the order posterior over all n! orders, log terms summed in
    long double and normalised)."""
    n = L.n
    perms = list(itertools.permutations(range(n)))
    a, _, _ = order_terms(L, np.array(perms, dtype=np.int64))
    with np.errstate(invalid="ignore"):
        ls = a.sum(axis=1)
    w = np.exp(ls - ls.max())
    return perms, w / w.sum()


def mulhi_counts(m):
    """How many of the 2^32 words w give mulhi32(w, m) = k, k = 0 .. m-1: Python ints that sum to 2^32."""
    edge = [-((-k << 32) // m) for k in range(m + 1)]  # ceil(k 2^32 / m): the first w with mulhi32 >= k
    return [edge[k + 1] - edge[k] for k in range(m)]


def transition_matrix(L):
    """The chain's one-step matrix over all n! orders from the rule's integers: the numerators over
    2^116 (Python ints; 2^32 words for i, 2^32 for j', 2^52 values of U_acc >> 12), the diagonal taking
    the rest.  -> (perms, num: list of lists of ints, den = 2^116)."""
    n = L.n
    perms = list(itertools.permutations(range(n)))
    index = {p: k for k, p in enumerate(perms)}
    a, _, _ = order_terms(L, np.array(perms, dtype=np.int64))
    ci, cj = mulhi_counts(n), mulhi_counts(n - 1)
    den = 1 << (64 + WEIGHT_BITS)
    num = [[0] * len(perms) for _ in perms]
    for k, p in enumerate(perms):
        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                q = list(p)
                q[i], q[j] = q[j], q[i]
                k2 = index[tuple(q)]
                lo, hi = min(i, j), max(i, j)
                now, was = LD(0), LD(0)
                for pos in range(lo, hi + 1):
                    now, was = now + a[k2, pos], was + a[k, pos]
                if not now > -np.inf:
                    acc = 0
                elif now - was >= 0:
                    acc = ONE
                else:
                    acc = int(weight_q(np.array([now - was]))[0][0])
                num[k][k2] += ci[i] * cj[j - (j > i)] * acc
        num[k][k] = den - sum(num[k])
    return perms, num, den


def pair_law(L):
    """{(order, parents): probability} over every order and every compatible choice of stored sets."""
    n = L.n
    law = {}
    w = [[(int(S), np.exp(LD(x) - LD(L.sc[v].max()))) for S, x in zip(L.sets[v], L.sc[v])] for v in range(n)]
    for perm in itertools.permutations(range(n)):
        pred, preds = 0, [0] * n
        for v in perm:
            preds[v] = pred
            pred |= 1 << v
        choices = [[(S, x) for S, x in w[v] if S & ~preds[v] == 0] for v in range(n)]
        for combo in itertools.product(*choices):
            p = LD(1)
            for _, x in combo:
                p = p * x
            law[(perm, tuple(S for S, _ in combo))] = p
    Z = sum(law.values(), LD(0))
    return {k: float(p / Z) for k, p in law.items()}


def chi_square(name, counts, law, K, log_sf):
    """Pearson's statistic of {cell: count} against {cell: probability}, cells that expect fewer than 5
    pooled into one; log_sf(x, dof) = ln of the chi-square tail.  Asserts the 1 - 1e-6 quantile."""
    assert set(counts) <= set(law), (name, "a sample outside the support")
    assert abs(sum(law.values()) - 1) < 1e-12
    stat, cells, pool_e, pool_o = 0.0, 0, 0.0, 0
    for cell, p in law.items():
        e, o = K * p, counts.get(cell, 0)
        if e < 5:
            pool_e, pool_o = pool_e + e, pool_o + o
        else:
            stat, cells = stat + (o - e) ** 2 / e, cells + 1
    if pool_e > 0:
        stat, cells = stat + (pool_o - pool_e) ** 2 / pool_e, cells + 1
    dof = cells - 1
    tail = log_sf(stat, dof) if dof > 0 else 0.0
    print(f"{name}: {len(law)} cells in the support, {cells} compared (pooled probability {pool_e / K:.3g}), "
          f"chi-square {stat:.2f} on {dof}, ln tail {tail:.3f}")
    assert dof >= 1 and tail >= math.log(1e-6), (name, stat, dof, tail)


# ---- inputs ------------------------------------------------------------------------
def make_lists(n, seed, max_parents=None, per_var=None, sd=1.0):
    """Lists with mild scores (normal, sd `sd`, minus 0.5 per parent), so that chains mix.  per_var None:
    every subset of the others up to max_parents; else the empty set and per_var - 1 distinct random sets
    of 1 .. max_parents parents drawn from all the others (bits above 31 and bit 62 at n = 63)."""
    rng = np.random.default_rng(seed)
    k = n - 1 if max_parents is None else min(max_parents, n - 1)
    offs, sets, scores = [0], [], []
    for v in range(n):
        others = [u for u in range(n) if u != v]
        if per_var is None:
            mine = [sum(1 << u for u in c) for r in range(k + 1) for c in itertools.combinations(others, r)]
        else:
            seen = {0}
            while len(seen) < per_var and k >= 1:
                r = int(rng.integers(1, k + 1))
                seen.add(sum(1 << int(u) for u in rng.choice(others, size=r, replace=False)))
            mine = sorted(seen)
        val = rng.normal(0.0, sd, size=len(mine)) - 0.5 * np.array([bin(S).count("1") for S in mine])
        sets += mine
        scores += list(val)
        offs.append(len(sets))
    return Lists(n, np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))


CHAIN_STEPS, CHAIN_THIN, CHAIN_MAX = 200, 7, 64
CHAIN_COUNTS = (1, 3, 64)
_CHAIN_INPUTS = None


def chain_inputs():
    """name -> (Lists, seed): the inputs of the GPU tests that compare chains with run()."""
    global _CHAIN_INPUTS
    if _CHAIN_INPUTS is None:
        _CHAIN_INPUTS = {
            "full-5": (make_lists(5, 505), 11),
            "k3-8": (make_lists(8, 808, max_parents=3), 12),
            "sparse-33": (make_lists(33, 3333, max_parents=3, per_var=24), 13),
            "sparse-63": (make_lists(63, 6363, max_parents=3, per_var=24), 14),
        }
    return _CHAIN_INPUTS


_CHAIN_REF = {}


def chain_reference(name):
    """run() of CHAIN_MAX chains for CHAIN_STEPS steps at CHAIN_THIN, once per input: chain c is the same
    in a run of fewer chains."""
    if name not in _CHAIN_REF:
        L, seed = chain_inputs()[name]
        _CHAIN_REF[name] = run(L, seed, CHAIN_MAX, CHAIN_STEPS, CHAIN_THIN)
    return _CHAIN_REF[name]


# the statistical tests: n -> (Lists, seed, T: the step of the one record, chains)
STAT_T = {3: 40, 4: 50, 6: 80}  # tests/test_order_mcmc_ref.py: the total variation from pi is below 1e-4 there
_STAT = None


def stat_inputs():
    global _STAT
    if _STAT is None:
        _STAT = {3: (make_lists(3, 303), 31, STAT_T[3], 20000), 4: (make_lists(4, 404), 41, STAT_T[4], 4096),
                 6: (make_lists(6, 606, max_parents=3), 61, STAT_T[6], 4096)}
    return _STAT


LONG_VARS = (7, 15)  # the variables of "lengths-63" whose list has 5000 entries, 4200 of them at the maximum


def term_orders(name):
    """The orders the GPU term test scores on term_cases()[name], uint8 (K, n), distinct rows: the identity,
    its reverse and 30 random ones; for "dynamic-6" one that puts variable 1 (no empty set) first; for
    "lengths-63" two that put a long list's variable last, after all 62 others, where every one of its
    entries is compatible and the sum of its weights passes 2^64 (the random orders do not: a sum above
    2^64 needs more than 4096 of the 4200 maximal entries, nearly every other variable before it)."""
    L = term_cases()[name]
    n = L.n
    rng = np.random.default_rng(len(name) + n)
    orders = [np.arange(n), np.arange(n)[::-1]] + [rng.permutation(n) for _ in range(30)]
    if name == "dynamic-6":
        orders.append(np.array([1, 0, 2, 3, 4, 5]))
    if name == "lengths-63":
        for v in LONG_VARS:
            orders.append(np.array([u for u in range(n) if u != v] + [v]))
            orders.append(np.array([u for u in range(n - 1, -1, -1) if u != v] + [v]))
    return np.unique(np.array(orders, dtype=np.uint8), axis=0)


_TERM_CASES = None


def term_cases():
    """name -> Lists, built once (see _term_cases)."""
    global _TERM_CASES
    if _TERM_CASES is None:
        _TERM_CASES = _term_cases()
    return _TERM_CASES


def _term_cases():
    """name -> Lists: the shapes of the GPU term test beyond the chain inputs (module docstring of
    tests/test_gpu_order_mcmc.py lists what each is for)."""
    out = {}
    rng = np.random.default_rng(4242)
    for n in (1, 2, 5):
        out[f"full-{n}"] = make_lists(n, 100 + n)
    out["sparse-33"] = chain_inputs()["sparse-33"][0]
    out["sparse-63"] = chain_inputs()["sparse-63"][0]
    # list lengths 1, 63, 64, 65, 255, 256, 257 (and 5000 with 4200 at the maximum) at n = 63: variable v's
    # list has lengths[v % 8] entries, random sets of up to 4 parents among all 62 others
    lengths = (1, 63, 64, 65, 255, 256, 257, 5000)
    n = 63
    offs, sets, scores = [0], [], []
    for v in range(n):
        others = [u for u in range(n) if u != v]
        want = lengths[v % 8] if v < 16 else lengths[v % 7]  # two long lists are enough
        seen = {0}
        while len(seen) < want:
            r = int(rng.integers(1, 5))
            seen.add(sum(1 << int(u) for u in rng.choice(others, size=r, replace=False)))
        mine = sorted(seen)
        if want == 5000:
            val = np.where(np.arange(want) % 25 < 21, 3.5, np.minimum(rng.normal(0.0, 1.0, size=want), 3.0))  # 4200 equal the maximum
        else:
            val = rng.normal(0.0, 1.0, size=want)
        sets += mine
        scores += list(val)
        offs.append(len(sets))
    out["lengths-63"] = Lists(n, np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))
    # scores of +-2e4, gaps beyond 745 nats, a variable whose only entry is the empty set, a list without it
    n = 6
    offs, sets, scores = [0], [], []
    for v in range(n):
        others = [u for u in range(n) if u != v]
        mine = [sum(1 << u for u in c) for r in range(n) for c in itertools.combinations(others, r)]
        if v == 0:
            mine = [0]
        elif v == 1:
            mine = [S for S in mine if S != 0]
        anchor = (2e4, -2e4, 1.5e4, -30.0, 0.0, 700.0)[v]
        gaps = rng.choice([0.0, 1.0, 40.0, 746.0, 900.0, 2000.0], size=len(mine))
        val = anchor - gaps + rng.uniform(-0.25, 0.25, size=len(mine))
        sets += mine
        scores += list(val)
        offs.append(len(sets))
    out["dynamic-6"] = Lists(n, np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))
    return out
