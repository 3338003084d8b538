"""The partition MCMC's contract (include/ulg.h, "Partition MCMC"; the kernels are
csrc/partition_mcmc.hip) restated in Python integers and numpy.longdouble, in
the manner of order_mcmc_ref, whose Philox draws, weights, decision margins and
caps it reuses.  No GPU, no project binding.  A state is a list of part masks
(Python ints); a move is made on that list as the contract's text says it,
not by the header's index arithmetic.

Caps beyond order_mcmc_ref's TERM CAP (none measured on the device):
LN RHO.  The device's ln rho is one FP64 division (2^-53 relative: 2^-52 is
taken, absolute on the logarithm), its log (4 ulp), for a split or join the
product k ln 2 and the add (an ulp each):
    rho_cap = 2^-52 + 4 ulp(log part) + ulp(k ln 2) + ulp(ln rho).
DELTA CAP.  order_mcmc_ref's with cnt = |D|, plus rho_cap and the last add's ulp.
"""
import numpy as np

import order_mcmc_ref as om

LD = np.longdouble
U64 = np.uint64
ONE = om.ONE
AUX = 65
LN2 = np.log(LD(2))


def eligible(S, A, R):
    ok = (S & ~U64(A)) == U64(0)
    return ok & ((S & U64(R)) != U64(0)) if R else ok


def term(L, v, A, R):
    """-> (a longdouble, cap, T int) of variable v under (A, R); (-inf, 0, 0) without an eligible entry.  Memoised on L."""
    memo = L.__dict__.setdefault("_part_terms", {})
    if (v, A, R) not in memo:
        el = eligible(L.sets[v], A, R)
        if not el.any():
            memo[(v, A, R)] = (LD(-np.inf), 0.0, 0)
        else:
            sc = L.sc[v][el]
            m = sc.max()
            with np.errstate(under="ignore"):
                val = np.exp(sc.astype(LD) - LD(m)) * LD(ONE)
            q = np.floor(val).astype(np.uint64)
            T = (int((q >> U64(32)).sum(dtype=np.uint64)) << 32) + int((q & U64(om.M32)).sum(dtype=np.uint64))
            logy = np.log(LD(T >> 32) * LD(2.0 ** (32 - 52)) + LD(T & om.M32) * LD(2.0 ** -52))
            a = LD(m) + logy
            memo[(v, A, R)] = (a, float(om.cap_of(a, logy, int((val >= 0.5).sum()), float(T))), T)
    return memo[(v, A, R)]


def pairs(parts, n):
    """[(A_v, R_v)] by variable of the partition `parts` (a list of masks)."""
    out, before, prev = [None] * n, 0, 0
    for B in parts:
        for v in range(n):
            if (B >> v) & 1:
                out[v] = (before, prev)
        before, prev = before | B, B
    return out


def part_of(parts, n):
    return [next(j for j, B in enumerate(parts) if (B >> v) & 1) for v in range(n)]


def from_part_of(row):
    return [sum(1 << v for v, p in enumerate(row) if p == j) for j in range(max(row) + 1)]


def propose(w, r, parts, n):
    """The move of the d = 0 words w and split mask r on `parts` -> (label, new parts or None for a no-op, ln rho, rho_cap)."""
    m = len(parts)
    if n < 2:
        return "none", None, LD(0), 0.0
    kind = int(w[0]) >> 30
    where = part_of(parts, n)
    mh = lambda x, k: (int(x) * k) >> 32  # noqa: E731

    def ratio(num, den, k=0):
        part = np.log(LD(num) / LD(den))
        lr = part + k * LN2
        cap = 2.0 ** -52 + 4 * np.spacing(abs(float(part))) + (np.spacing(abs(k) * 0.6931471805599453) if k else 0.0) + np.spacing(abs(float(lr)))
        return lr, float(cap)

    if kind == 0:
        v, wp = mh(w[1], n), mh(w[2], n - 1)
        u = wp + (wp >= v)
        if where[v] == where[u]:
            return "swap-noop", None, LD(0), 0.0
        new = list(parts)
        flip = (1 << v) | (1 << u)
        new[where[v]] ^= flip
        new[where[u]] ^= flip
        return "swap", new, LD(0), 0.0
    if kind < 3:
        v, tau = mh(w[1], n), mh(w[2], 2 * m + 1)
        j, single = where[v], parts[where[v]] == 1 << v
        rest = [B & ~(1 << v) for B in parts]
        if tau & 1:
            k = (tau - 1) // 2
            if k == j:
                return "topart-noop", None, LD(0), 0.0
            rest[k] |= 1 << v
            label = "topart"
        else:
            g = tau // 2
            if single and g in (j, j + 1):
                return "togap-noop", None, LD(0), 0.0
            rest = rest[:g] + [1 << v] + rest[g:]
            label = "togap"
        new = [B for B in rest if B]
        return (label,) + (new,) + ratio(2 * m + 1, 2 * len(new) + 1)
    j = mh(w[1], m)
    if (int(w[0]) >> 29) & 1:
        low, up = parts[j] & r, parts[j] & ~r
        if not low or not up:
            return "split-noop", None, LD(0), 0.0
        return ("split", parts[:j] + [low, up] + parts[j + 1:]) + ratio(m, m + 1, bin(parts[j]).count("1"))
    if j == m - 1:
        return "join-noop", None, LD(0), 0.0
    both = parts[j] | parts[j + 1]
    return ("join", parts[:j] + [both] + parts[j + 2:]) + ratio(m, m - 1, -bin(both).count("1"))


def evaluate(L, parts, new):
    """-> (D, delta of the terms longdouble or -inf, its cap, new terms [(v, a, cap, T)])."""
    n = L.n
    old_pairs, new_pairs = pairs(parts, n), pairs(new, n)
    D = [v for v in range(n) if old_pairs[v] != new_pairs[v]]
    now = was = LD(0)
    mag_now = mag_was = caps = 0.0
    fresh = []
    for v in D:
        a2, c2, T2 = term(L, v, *new_pairs[v])
        a1, c1, _ = term(L, v, *old_pairs[v])
        fresh.append((v, a2, c2, T2))
        now, was = now + a2, was + a1
        if a2 > -np.inf:
            mag_now += abs(float(a2))
        mag_was += abs(float(a1))
        caps += c1 + c2
    if not now > -np.inf:
        return D, LD(-np.inf), 0.0, fresh
    diff = now - was
    return D, diff, caps + len(D) * (np.spacing(mag_now) + np.spacing(mag_was)) + np.spacing(abs(float(diff))), fresh


def pick(L, v, A, R, a, a_cap, u_set):
    """A record's parent-set pick -> (entry index into the lists, margin, slack), as order_mcmc_ref.picks."""
    el = eligible(L.sets[v], A, R)
    with np.errstate(under="ignore"):
        val = np.where(el, np.exp(L.sc[v].astype(LD) - a) * LD(ONE), LD(0))
    Cs = np.cumsum(np.floor(val).astype(np.uint64).astype(np.int64))
    T = int(Cs[-1])
    assert T > 0
    t = int(om.mulhi64(np.array([u_set], dtype=np.uint64), np.array([T], dtype=np.uint64))[0])
    j = int((Cs > t).argmax())
    low = int(Cs[j - 1]) if j else 0
    slack = om.ULP_ALLOWANCE * (int((val >= 0.5).sum()) + 1) + 2 * int(np.ceil(T * a_cap)) + 2
    return int(L.offsets[v]) + j, min(t - low, int(Cs[j]) - t), slack


def run(L, seed, init, steps, thin=1):
    """Chain c = 0 .. len(init)-1 from init[c] (a row of part indices) for `steps` steps -> dict of arrays in the
    device's layout (part, parts, log_score, score_cap, parents, log_weight, trace_delta, trace_cap, trace_accept,
    accepted, final_part, final_terms, final_cap), labels: the moves met (with "-inf" for a rejection by a -inf
    term), sizes: |D| of every evaluated move, max_T: the largest sum of weights, undecided / min_excess as
    order_mcmc_ref.run."""
    n, C = L.n, len(init)
    R = steps // thin
    out = dict(part=np.zeros((R, C, n), np.uint8), parts=np.zeros((R, C), np.int32), log_score=np.zeros((R, C), LD),
               score_cap=np.zeros((R, C)), parents=np.zeros((R, C, n), np.uint64), log_weight=np.zeros((R, C)),
               trace_delta=np.full((steps, C), -np.inf, LD), trace_cap=np.zeros((steps, C)), trace_accept=np.zeros((steps, C), bool),
               accepted=np.zeros(C, np.int64), final_part=np.zeros((C, n), np.uint8), final_terms=np.zeros((C, n), LD),
               final_cap=np.zeros((C, n)), labels=set(), sizes=[], max_T=0, undecided=0, min_excess=1 << 62)

    def margin_seen(margin, slack):
        out["undecided"] += int(margin < slack)
        out["min_excess"] = min(out["min_excess"], int(margin - slack))

    for c in range(C):
        parts = from_part_of([int(p) for p in init[c]])
        tm = [term(L, v, *pr) for v, pr in enumerate(pairs(parts, n))]
        assert all(a > -np.inf for a, _, _ in tm), "an initial partition with a -inf term"
        out["max_T"] = max([out["max_T"]] + [T for _, _, T in tm])
        for s in range(steps):
            t = s + 1
            w = [int(x[0]) for x in om._draw(seed, t, [c], 0)]
            x = [int(y[0]) for y in om._draw(seed, t, [c], AUX)]
            label, new, lr, rcap = propose(w, x[2] | (x[3] << 32), parts, n)
            out["labels"].add(label)
            if new is not None:
                D, diff, dcap, fresh = evaluate(L, parts, new)
                out["sizes"].append(len(D))
                out["max_T"] = max([out["max_T"]] + [T for _, _, _, T in fresh])
                if diff > -np.inf:
                    delta = diff + lr
                    cap = dcap + rcap + np.spacing(abs(float(delta)))
                else:
                    delta, cap = LD(-np.inf), 0.0
                    out["labels"].add("-inf")
                acc, margin, slack = om.decide(np.array([delta]), np.array([cap]), np.array([x[0] | (x[1] << 32)], dtype=np.uint64))
                margin_seen(margin[0], slack[0])
                out["trace_delta"][s, c], out["trace_cap"][s, c], out["trace_accept"][s, c] = delta, cap, acc[0]
                if acc[0]:
                    parts = new
                    for v, a, tc, T in fresh:
                        tm[v] = (a, tc, T)
                    out["accepted"][c] += 1
            if t % thin == 0:
                r = t // thin - 1
                out["part"][r, c], out["parts"][r, c] = part_of(parts, n), len(parts)
                tot, mag = LD(0), 0.0
                for a, _, _ in tm:
                    tot, mag = tot + a, mag + abs(float(a))
                out["log_score"][r, c], out["score_cap"][r, c] = tot, sum(tc for _, tc, _ in tm) + n * np.spacing(mag)
                lw = 0.0
                for v, (A, Rq) in enumerate(pairs(parts, n)):
                    u = om._draw(seed, t, [c], 1 + v)
                    e, margin, slack = pick(L, v, A, Rq, tm[v][0], tm[v][1], int(u[0][0]) | (int(u[1][0]) << 32))
                    margin_seen(margin, slack)
                    out["parents"][r, c, v] = L.sets_all[e]
                    lw = lw + float(L.scores_all[e])
                out["log_weight"][r, c] = lw
        out["final_part"][c] = part_of(parts, n)
        out["final_terms"][c], out["final_cap"][c] = [a for a, _, _ in tm], [tc for _, tc, _ in tm]
    return out


# ---- exact laws, by enumeration ----------------------------------------------------
def dag_table(L):
    """Every DAG of the stored families: (par int64 (K, n), w longdouble (K): prod_v w_v(Pa_v) unnormalised, part
    int64 (K, n): its partition by peeling sources, ext int64 (K): its linear extensions)."""
    n = L.n
    grids = np.meshgrid(*[np.arange(len(L.sets[v])) for v in range(n)], indexing="ij")
    par = np.stack([L.sets[v].astype(np.int64)[g.ravel()] for v, g in enumerate(grids)], axis=1)
    lw = sum(L.sc[v].astype(LD)[g.ravel()] for v, g in enumerate(grids))
    alive = np.full(len(par), (1 << n) - 1, dtype=np.int64)
    part = np.zeros(par.shape, dtype=np.int64)
    for j in range(n):
        src = np.zeros(len(par), dtype=np.int64)
        for v in range(n):
            is_src = ((alive >> v) & 1 == 1) & ((par[:, v] & alive) == 0)
            src |= is_src.astype(np.int64) << v
            part[is_src, v] = j
        alive &= ~src
    keep = alive == 0
    par, lw, part = par[keep], lw[keep], part[keep]
    f = np.zeros((1 << n, len(par)), dtype=np.int64)
    f[0] = 1
    for S in range(1, 1 << n):
        for v in range(n):
            if (S >> v) & 1:
                f[S] += np.where((par[:, v] & ~(S ^ (1 << v))) == 0, f[S ^ (1 << v)], 0)
    return par, np.exp(lw - lw.max()), part, f[-1]


def edge_matrix(par, w, n):
    """sum_k w_k [u in Pa_v^k] / sum_k w_k as float64 (n, n), row u column v."""
    return np.array([[float((w * ((par[:, v] >> u) & 1)).sum() / w.sum()) for v in range(n)] for u in range(n)])


def word(k, m):
    """A 32-bit word w with mulhi32(w, m) = k."""
    return -((-k << 32) // m)


def transition_matrix(L):
    """The restated step's matrix over all ordered partitions, the draws taken as uniform (kind 1/4 each, v 1/n,
    tau 1/(2m+1), a split's subset 2^-k, ...) and the accept probability min(1, exp(delta)) in long double: every
    move goes through propose() by words made for it.  -> (states: list of tuples of masks, K float64 matrix whose
    diagonal collects the no-ops and rejections, log_pi: ln prod_v T_v by state)."""
    n = L.n
    states, frontier = [], [((1 << n) - 1,)]
    moves = lambda m: ([(word(0, 4) | 0, word(v, n), word(u, n - 1), LD(1) / (4 * n * (n - 1)), 0) for v in range(n) for u in range(n - 1)] +  # noqa: E731
                       [(1 << 30, word(v, n), word(tau, 2 * m + 1), LD(1) / (2 * n * (2 * m + 1)), 0) for v in range(n) for tau in range(2 * m + 1)] +
                       [(3 << 30, word(j, m), 0, LD(1) / (8 * m), 0) for j in range(m)])
    index, rows = {}, []
    while frontier:  # every state reachable from the flat one: irreducibility is then the reverse reachability
        S = frontier.pop()
        if S in index:
            continue
        index[S] = len(states)
        states.append(S)
        row = {}
        cand = moves(len(S))
        for j, B in enumerate(S):  # splits: every subset of B_j as the mask r
            k = bin(B).count("1")
            bits = [v for v in range(n) if (B >> v) & 1]
            cand += [((3 << 30) | (1 << 29), word(j, len(S)), 0, LD(1) / (8 * len(S) * 2 ** k), sum(1 << bits[i] for i in range(k) if (sub >> i) & 1))
                     for sub in range(1 << k)]
        for w0, w1, w2, p, r in cand:
            _, new, lr, _ = propose((w0, w1, w2, 0), r, list(S), n)
            if new is None:
                continue
            _, diff, _, _ = evaluate(L, list(S), new)
            acc = LD(0) if not diff > -np.inf else min(LD(1), np.exp(diff + lr))
            row[tuple(new)] = row.get(tuple(new), LD(0)) + p * acc
            frontier.append(tuple(new))
        rows.append(row)
    K = np.zeros((len(states), len(states)))
    for i, row in enumerate(rows):
        for S2, p in row.items():
            K[i, index[S2]] = float(p)
        K[i, i] += 1.0 - K[i].sum()
    log_pi = np.array([float(sum(term(L, v, *pr)[0] for v, pr in enumerate(pairs(list(S), n)))) for S in states])
    return states, K, log_pi


# ---- inputs ------------------------------------------------------------------------
LONG = 5000  # the long list: 4200 entries at the maximum


def with_chain_and_long_list(L, long_var=None):
    """L with {v-1} added to every variable v >= 1 that lacks it (so the singletons 0, 1, .., n-1 are a valid state)
    and, for long_var, LONG more sets, all holding variable 0, 21 of 25 at the score 3.5."""
    rng = np.random.default_rng(L.n)
    offs, sets, scores = [0], [], []
    for v in range(L.n):
        mine, val = [int(S) for S in L.sets[v]], list(L.sc[v])
        if v and (1 << (v - 1)) not in mine:
            mine.append(1 << (v - 1))
            val.append(-0.25)
        if v == long_var:
            others = [u for u in range(1, L.n) if u != v]
            seen = set(mine)
            while len(seen) < len(mine) + LONG:
                seen.add(1 | sum(1 << int(u) for u in rng.choice(others, size=int(rng.integers(1, 5)), replace=False)))
            extra = sorted(seen - set(mine))
            mine += extra
            val += [3.5 if i % 25 < 21 else float(min(rng.normal(), 3.0)) for i in range(LONG)]
        sets += mine
        scores += val
        offs.append(len(sets))
    return om.Lists(L.n, np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))


CHAIN_STEPS, CHAIN_THIN = 150, 7
_INPUTS, _REF = None, {}


def chain_inputs():
    """name -> (Lists, seed, init uint8 (4, n)): chain 0 and 3 from the empty DAG, 1 from the singletons 0, 1, ..,
    2 from (all but n-1 | n-1), where at n = 33 and 63 the long list of n-1 is eligible whole: its sum passes 2^64."""
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = {}
        for name, L, seed, long_var in (("full-5", om.make_lists(5, 505), 21, None), ("k3-8", om.make_lists(8, 808, max_parents=3), 22, None),
                                        ("sparse-33", om.make_lists(33, 3333, max_parents=3, per_var=24), 23, 32),
                                        ("sparse-63", om.make_lists(63, 6363, max_parents=3, per_var=24), 25, 62)):
            n = L.n
            init = np.zeros((4, n), dtype=np.uint8)
            init[1] = np.arange(n)
            init[2, n - 1] = 1
            _INPUTS[name] = (with_chain_and_long_list(L, long_var), seed, init)
    return _INPUTS


def chain_reference(name):
    if name not in _REF:
        L, seed, init = chain_inputs()[name]
        _REF[name] = run(L, seed, init, CHAIN_STEPS, CHAIN_THIN)
    return _REF[name]


# the statistical tests: n -> (Lists, seed, T: the step of the one record, chains); tests/test_partition_mcmc_ref.py
# shows the total variation of the flat state's T-step law from pi to be below 1e-4
STAT = {4: (om.make_lists(4, 404, sd=2.0), 41, 200, 4096), 5: (om.make_lists(5, 515, sd=1.0), 51, 300, 4096)}
