"""The tempered ladders' contract (include/ulg.h, "Metropolis-coupled order MCMC"; the kernel is
mc3_run_kernel in csrc/order_mcmc.hip) restated on top of order_mcmc_ref: its terms, draws, decide and
picks, Python integers and numpy.longdouble, vectorised over every replica of every ladder.  No GPU.

What differs from the chains: replica k = l R + r0 keeps its index (the Philox chain word of its shuffle,
moves and parent sets) while perm[l, r] says which of ladder l's replicas stands on rung r; rung r accepts
a move on floor(exp(beta_r delta) 2^52); after the moves of a step t with t mod E = 0 round x = t / E
decides the pairs (r, r + 1), r = x (mod 2), on d = (beta_r - beta_{r+1}) (S_{r+1} - S_r) with the draw
(t, c = l R + r, domain 64); rung 0 is recorded.

CAPS, derived from order_mcmc_ref's (none is measured on the device).
  tempered exponent  the device forms beta delta in one FP64 multiply of its own delta, which lies within
      delta_cap of this module's: |e_dev - e_ref| <= beta delta_cap + ulp(beta delta).
  exchange           S_r is a record's log_score: score_cap_r = the sum of its terms' caps + n ulp(sum |a_p|).
      The difference S_{r+1} - S_r moves by both caps and its own rounding, the product by the factor
      |beta_r - beta_{r+1}| (the betas' difference is one FP64 subtraction here as there) and its rounding:
      d_cap = |beta_r - beta_{r+1}| (score_cap_r + score_cap_{r+1} + ulp(S_{r+1} - S_r)) + ulp(d).
Both go through om.decide's slack: a move or an exchange whose margin is below 8 + ceil(q cap) + 1 is
UNDECIDED, as a pick is by om.picks' slack; tests/test_order_mc3_ref.py asserts that the GPU tests' inputs
have none, so those tests demand equality.
"""
import itertools

import numpy as np

import order_mcmc_ref as om

LD = om.LD
U64 = np.uint64
SWAP_DOMAIN = 64


def geometric(rungs, beta_min=0.1):
    b = np.array([beta_min ** (r / max(rungs - 1, 1)) for r in range(rungs)], dtype=np.float64)
    b[0] = 1.0
    return b


def _sums(term, tcap):
    """The full sums of rows of terms, p ascending -> (S longdouble, score_cap)."""
    tot, mag = np.zeros(len(term), dtype=LD), np.zeros(len(term))
    for p in range(term.shape[1]):
        tot = tot + term[:, p]
        mag += np.abs(term[:, p].astype(np.float64))
    return tot, tcap.sum(axis=1) + term.shape[1] * np.spacing(mag)


def run(L, seed, ladders, betas, E, steps, thin=1, init_order=None, want_parents=True):
    """`ladders` ladders (0 .. ladders-1, or the indices given) of len(betas) rungs for `steps` steps from
    begin.  init_order: int (ladders * R, n), row l R + r0.  -> dict: the cold records order (recs, Ln, n),
    log_score, score_cap, parents, log_weight; accepted (Ln, R) by rung, swaps (Ln, R-1); trace_delta
    (steps, Ln, R) the untempered delta by rung, trace_cap, trace_accept; swap_d (rounds, Ln, R-1) (-inf where
    the round does not consider the pair), swap_cap, swap_accept; replica (Ln, R), final_order, final_terms,
    final_cap by rung; undecided, min_excess as om.run."""
    n, R = L.n, len(betas)
    betas = np.asarray(betas, dtype=np.float64)
    lad = np.arange(ladders, dtype=np.int64) if np.isscalar(ladders) else np.asarray(ladders, dtype=np.int64)
    Ln = len(lad)
    ks = (lad[:, None] * R + np.arange(R)[None, :]).ravel()  # row l' R + slot of every array below
    order = np.array(init_order, dtype=np.int64) if init_order is not None else om.shuffle(seed, ks, n)
    pre = om.prefixes(order)
    term, tcap, _ = om.order_terms(L, order)
    assert np.all(term > -np.inf), "an initial order with a -inf term"
    perm = np.tile(np.arange(R), (Ln, 1))  # perm[l', r] = the slot on rung r
    P, rows, lrow = np.arange(n)[None, :], np.arange(Ln * R), np.arange(Ln)
    rec = {k: [] for k in ("order", "log_score", "score_cap", "parents", "log_weight")}
    tr_delta = np.full((steps, Ln, R), -np.inf, dtype=LD)
    tr_cap, tr_acc = np.zeros((steps, Ln, R)), np.zeros((steps, Ln, R), dtype=bool)
    sw_d, sw_cap, sw_acc = [], [], []
    accepted, swaps = np.zeros((Ln, R), dtype=np.int64), np.zeros((Ln, max(R - 1, 0)), dtype=np.int64)
    undecided, min_excess = 0, 1 << 62

    def note(margin, slack):
        nonlocal undecided, min_excess
        undecided += int((margin < slack).sum())
        min_excess = min(min_excess, int((margin - slack).min()))

    for t in range(1, steps + 1):
        at = (lrow[:, None] * R + perm).ravel()  # the row standing on (l', r), rung-major within a ladder
        if n > 1:
            rung_of = np.empty(Ln * R, dtype=np.int64)
            rung_of[at] = np.tile(np.arange(R), Ln)
            beta = betas[rung_of]
            i, j, u_acc = om.moves(seed, t, ks, n)
            lo, hi = np.minimum(i, j), np.maximum(i, j)
            va, vb = order[rows, lo], order[rows, hi]
            flip = (U64(1) << va.astype(U64)) ^ (U64(1) << vb.astype(U64))
            new_order = order.copy()
            new_order[rows, lo], new_order[rows, hi] = vb, va
            new_pre = np.where((P > lo[:, None]) & (P <= hi[:, None]), pre ^ flip[:, None], pre)
            touched = (P >= lo[:, None]) & (P <= hi[:, None])
            ci, pi = np.nonzero(touched)
            fresh, fcap = np.zeros((Ln * R, n), dtype=LD), np.zeros((Ln * R, n))
            fresh[ci, pi], fcap[ci, pi], _ = om.terms(L, new_order[ci, pi], new_pre[ci, pi])
            now, was = np.zeros(Ln * R, dtype=LD), np.zeros(Ln * R, dtype=LD)
            mag_now, mag_was, caps = np.zeros(Ln * R), np.zeros(Ln * R), np.zeros(Ln * R)
            with np.errstate(invalid="ignore"):
                for p in range(n):
                    on = touched[:, p]
                    now, was = np.where(on, now + fresh[:, p], now), np.where(on, was + term[:, p], was)
                    mag_now += np.where(on & (fresh[:, p] > -np.inf), np.abs(fresh[:, p].astype(np.float64)), 0.0)
                    mag_was += np.where(on, np.abs(term[:, p].astype(np.float64)), 0.0)
                    caps += np.where(on, fcap[:, p] + tcap[:, p], 0.0)
                dead = ~(now > -np.inf)
                delta = np.where(dead, LD(-np.inf), now - was)
            cnt = (hi - lo + 1).astype(np.float64)
            d64 = np.abs(np.where(dead, 0.0, delta.astype(np.float64)))
            dcap = np.where(dead, 0.0, caps + cnt * (np.spacing(mag_now) + np.spacing(mag_was)) + np.spacing(d64))
            acc, margin, slack = om.decide(beta.astype(LD) * delta, beta * dcap + np.spacing(beta * d64), u_acc)
            note(margin, slack)
            tr_delta[t - 1], tr_cap[t - 1], tr_acc[t - 1] = (x[at].reshape(Ln, R) for x in (delta, dcap, acc))
            take = acc[:, None]
            order, pre = np.where(take, new_order, order), np.where(take, new_pre, pre)
            term, tcap = np.where(take & touched, fresh, term), np.where(take & touched, fcap, tcap)
            accepted += acc[at].reshape(Ln, R)
        if R > 1 and t % E == 0:
            x = t // E
            S, scap = _sums(term[at], tcap[at])
            S, scap = S.reshape(Ln, R), scap.reshape(Ln, R)
            on = np.array([(r - x) % 2 == 0 for r in range(R - 1)])
            db = betas[:-1] - betas[1:]  # FP64, one subtraction each
            ds = S[:, 1:] - S[:, :-1]
            d = np.where(on[None, :], db[None, :].astype(LD) * ds, LD(-np.inf))
            ds64, d64 = np.abs(ds.astype(np.float64)), np.abs(np.where(on[None, :], d, LD(0)).astype(np.float64))
            dcap = np.abs(db)[None, :] * (scap[:, :-1] + scap[:, 1:] + np.spacing(ds64)) + np.spacing(d64)
            w = om._draw(seed, t, (lad[:, None] * R + np.arange(R - 1)[None, :]).ravel(), SWAP_DOMAIN)
            acc, margin, slack = om.decide(d.ravel(), dcap.ravel(), w[0] | (w[1] << U64(32)))
            note(margin, slack)
            acc = acc.reshape(Ln, R - 1)
            sw_d.append(d), sw_cap.append(np.where(on[None, :], dcap, 0.0)), sw_acc.append(acc)
            for r in np.flatnonzero(on):  # disjoint pairs: any order
                a, b = perm[:, r].copy(), perm[:, r + 1].copy()
                perm[:, r], perm[:, r + 1] = np.where(acc[:, r], b, a), np.where(acc[:, r], a, b)
            swaps += acc
        if t % thin == 0:
            cold = lrow * R + perm[:, 0]
            rec["order"].append(order[cold].astype(np.uint8))
            S, scap = _sums(term[cold], tcap[cold])
            rec["log_score"].append(S), rec["score_cap"].append(scap)
            if want_parents:
                ci, pi = np.nonzero(np.ones((Ln, n), dtype=bool))
                w = om._draw(seed, t, ks[cold][ci], 1 + pi)
                e, margin, slack = om.picks(L, order[cold][ci, pi], pre[cold][ci, pi], term[cold][ci, pi], tcap[cold][ci, pi],
                                            w[0] | (w[1] << U64(32)))
                note(margin, slack)
                par, chosen = np.zeros((Ln, n), dtype=np.uint64), np.zeros((Ln, n))
                par[ci, order[cold][ci, pi]] = L.sets_all[e]
                chosen[ci, order[cold][ci, pi]] = L.scores_all[e].astype(np.float64)
                lw = np.zeros(Ln)
                for v in range(n):
                    lw = lw + chosen[:, v]
                rec["parents"].append(par), rec["log_weight"].append(lw)
    at = (lrow[:, None] * R + perm).ravel()
    out = {k: np.stack(v) for k, v in rec.items() if v}
    out.update(accepted=accepted, swaps=swaps, trace_delta=tr_delta, trace_cap=tr_cap, trace_accept=tr_acc,
               swap_d=np.stack(sw_d) if sw_d else np.zeros((0, Ln, max(R - 1, 0)), dtype=LD),
               swap_cap=np.stack(sw_cap) if sw_cap else np.zeros((0, Ln, max(R - 1, 0))),
               swap_accept=np.stack(sw_acc) if sw_acc else np.zeros((0, Ln, max(R - 1, 0)), dtype=bool),
               replica=lad[:, None] * R + perm, final_order=order[at].reshape(Ln, R, n), final_terms=term[at].reshape(Ln, R, n),
               final_cap=tcap[at].reshape(Ln, R, n), undecided=undecided, min_excess=min_excess, records=len(rec["order"]))
    return out


# ---- exact laws at R = 2 -----------------------------------------------------------
def move_matrix(L, beta):
    """om.transition_matrix with the tempered rule: numerators over 2^116 of rung beta's one-step matrix."""
    n = L.n
    perms = list(itertools.permutations(range(n)))
    index = {p: k for k, p in enumerate(perms)}
    a, _, _ = om.order_terms(L, np.array(perms, dtype=np.int64))
    ci, cj = om.mulhi_counts(n), om.mulhi_counts(n - 1)
    den = 1 << (64 + om.WEIGHT_BITS)
    num = [[0] * len(perms) for _ in perms]
    for k, p in enumerate(perms):
        for i, j in itertools.permutations(range(n), 2):
            q = list(p)
            q[i], q[j] = q[j], q[i]
            k2 = index[tuple(q)]
            now = sum((a[k2, pos] for pos in range(min(i, j), max(i, j) + 1)), LD(0))
            was = sum((a[k, pos] for pos in range(min(i, j), max(i, j) + 1)), LD(0))
            if not now > -np.inf:
                acc = 0
            elif now - was >= 0:
                acc = om.ONE
            else:
                acc = int(om.weight_q(np.array([LD(beta) * (now - was)]))[0][0])
            num[k][k2] += ci[i] * cj[j - (j > i)] * acc
        num[k][k] = den - sum(num[k])
    return perms, num, den


def joint_step(L, betas):
    """One (move, exchange) step of a ladder of two rungs over the (n!)^2 pairs (cold order k, hot order h),
    state k n! + h, from the rule's integers: J = (P_cold x P_hot) X as longdouble, where X sends (k, h) to
    (h, k) on q_kh of the 2^52 values of U >> 12 (q = 2^52 for d >= 0, floor(exp(d) 2^52) below) and keeps
    it otherwise.  -> (perms, M: the moves alone, J: the moves and the exchange)."""
    perms, pc, den = move_matrix(L, betas[0])
    _, ph, _ = move_matrix(L, betas[1])
    a, _, _ = om.order_terms(L, np.array(perms, dtype=np.int64))
    S = a.sum(axis=1)
    m = len(perms)
    Pc = np.array([[LD(x) / LD(den) for x in row] for row in pc], dtype=LD)
    Ph = np.array([[LD(x) / LD(den) for x in row] for row in ph], dtype=LD)
    M = np.kron(Pc, Ph)
    d = LD(np.float64(betas[0]) - np.float64(betas[1])) * (S[None, :] - S[:, None])  # [k, h]: S_hot - S_cold
    q = np.where(d >= 0, om.ONE, om.weight_q(np.where(d < 0, d, LD(0)))[0]).astype(LD) / LD(om.ONE)
    X = np.zeros((m * m, m * m), dtype=LD)
    for k in range(m):
        for h in range(m):
            X[k * m + h, h * m + k] += q[k, h]
            X[k * m + h, k * m + h] += 1 - q[k, h]
    return perms, M, M @ X


def ladder_law(L, betas):
    """(perms, pi: the order posterior, hot: pi^betas[1] normalised), longdouble."""
    perms, pi = om.order_law(L)
    hot = pi ** LD(betas[1])
    return perms, pi, hot / hot.sum()


# ---- the GPU tests' inputs -----------------------------------------------------------
LADDER_STEPS, LADDER_MAX = 70, 3
LADDER_CASES = ((2, 1), (3, 7), (8, 3))  # (R, E)
_LADDER_REF = {}


def ladder_reference(name, R, E):
    """run() of LADDER_MAX ladders on om.chain_inputs()[name], once: ladder l is the same among fewer."""
    if (name, R, E) not in _LADDER_REF:
        L, seed = om.chain_inputs()[name]
        _LADDER_REF[(name, R, E)] = run(L, seed, LADDER_MAX, geometric(R), E, LADDER_STEPS, om.CHAIN_THIN)
    return _LADDER_REF[(name, R, E)]


STAT_BETAS = np.array([1.0, 0.3])
STAT_T = {3: 40, 4: 50}  # tests/test_order_mc3_ref.py: the joint law is within 1e-4 of pi x pi^0.3 there
STAT_SEED = 4141
