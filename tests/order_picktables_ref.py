"""The contract of a record's DAG drawn from the order MCMC's tables (include/ulg.h, "Order MCMC: a record's
DAG from the tables"; the kernels are csrc/order_picktables.hip) restated in numpy and Python integers.  No
GPU, no project binding.

  stages   build(): order_sumtables_ref.butterfly's float64 rounds with a copy of the table before rounds 6,
           12, 18, 24 (S_c, c = 1 .. nch - 1, nch = max(1, ceil(K / 6))) and the entry map E.  direct():
           the long-double sum a stage slot stands for -- the stored sets whose index bits >= 6c equal the
           slot's and whose bits < 6c lie inside it.
  pick     levels(): per level c = nch - 1 .. 0 the 64 lanes' values and weights floor(exp(value - a_cur)
           2^52) (exp in long double, as order_mcmc_ref's picks); pick(): the descent with the draws of
           domain 1 + p + 64 c.

LAW BOUND.  Level c's lanes split the sets under the slot chosen above by their bits 6c .. 6c + 5, and with
exact tables the lanes' weights sum to that slot's: the ratios telescope to p(P) = w(P) / A(U).  What the
restated pick differs by:
    values   a stage slot made in 6c rounds is within cap_c = 6c (ROUND_CAP + ulp / 2) of its sum
             (order_sumtables_ref's SLOT CAP with 6c for K; level 0 reads the scores: exact), the ulp at
             that slot's own magnitude.  A ratio exp(v_j) / sum exp(v_l) has every weighing lane's error in
             it: it moves by at most e^(2 cap_c), relative, cap_c the LARGEST cap among the level's lanes of
             finite value (law() takes that maximum); a_cur cancels in it.
    floors   q_l = rho_l W - f_l with f_l in [0, 1), T = W - F with F in [0, 64), so
             q_j / T - rho_j = (rho_j F - f_j) / T lies in (-1 / T, 64 / T): 64 2^-52 per chunk, T_c being
             2^52 sum exp(v_l - a_cur) - F, within 2^52 (2 cap_c + 2^-46) of 2^52 (what 64 / T_c has above
             64 2^-52 is below 2^-88, far under the comparison's own long-double arithmetic).
A product of ratios each at most 1 moves by at most the sum of its factors' absolute errors, so
    |p_pick(P) - p(P)| <= p(P) expm1(2 sum_c cap_c) + nch 64 2^-52 =: law_bound.
"""
import math

import numpy as np

import order_mcmc_ref as om
import order_sumtables_ref as st

LD, U64 = np.longdouble, np.uint64
BITS, LANES = 6, 64


def chunks(K):
    return max(1, -(-K // BITS))


def build(L, v):
    """-> (C_v, L_v float64, [S_1 .. S_{nch-1}], E int32) by the contract's rounds and copies."""
    C = int(np.bitwise_or.reduce(L.sets[v])) if len(L.sets[v]) else 0
    mem = st.members(C)
    T, E = np.full(1 << len(mem), -np.inf), np.full(1 << len(mem), -1, dtype=np.int32)
    idx = [st.index(mem, S) for S in L.sets[v]]
    T[idx], E[idx] = L.sc[v], np.arange(len(idx), dtype=np.int32)
    stages = []
    for j in range(len(mem)):
        if j and j % BITS == 0:
            stages.append(T.copy())
        W = T.reshape(-1, 2, 1 << j)
        W[:, 1, :] = st.logaddexp(W[:, 1, :], W[:, 0, :])
    return C, T, stages, E


def direct(L, v, c):
    """-> (value longdouble, count, cap float64) by slot of stage c (c = nch: the table itself): the sum over
    the stored sets with index bits >= 6c exact and bits < 6c inside the slot's; cap = cap_c above."""
    S, sc = L.sets[v], L.sc[v]
    mem = st.members(int(np.bitwise_or.reduce(S)) if len(S) else 0)
    K = len(mem)
    low = (1 << min(BITS * c, K)) - 1
    y = np.arange(1 << K, dtype=np.int64)
    top = sc.max() if len(sc) else 0.0
    tot, count, mag = np.zeros(len(y), dtype=LD), np.zeros(len(y), dtype=np.int64), np.zeros(len(y))
    for s, x in zip(sc, (st.index(mem, P) for P in S)):
        inside = ((y & ~low) == (x & ~low)) & ((x & low & ~y) == 0)
        tot[inside] += np.exp(LD(s) - LD(top))
        count += inside
        mag = np.where(inside, np.maximum(mag, abs(s)), mag)
    with np.errstate(divide="ignore"):
        val = LD(top) + np.log(tot)
    big = np.maximum(np.abs(np.where(count > 0, val, 0).astype(np.float64)), mag)
    cap = min(BITS * c, K) * (st.ROUND_CAP + np.spacing(np.where(count > 0, big, 1.0)) / 2)
    return np.where(count > 0, val, LD(-np.inf)), count, cap


def levels(K, stages, E, sc, x, a, path):
    """The levels of a pick at index x with term a, c = nch - 1 .. 0.  path(c, q int list, values) -> the
    lane taken at level c.  Yields (c, q: 64 Python ints, values float64 (64), slots, j)."""
    fixed, a_cur = 0, a
    for c in range(chunks(K) - 1, -1, -1):
        lanes = np.arange(LANES)
        on = ((lanes & ~((x >> (BITS * c)) & 63)) == 0) & (lanes < (1 << max(K - BITS * c, 0)))
        slots = fixed | (lanes << (BITS * c)) | (x & ((1 << (BITS * c)) - 1))
        safe = np.where(on, slots, 0)
        if c >= 1:
            val = np.where(on, stages[c - 1][safe], -np.inf)
        else:
            e = E[safe]
            val = np.where(on & (e >= 0), sc[np.maximum(e, 0)], -np.inf)
        q = [int(t) for t in om.weight_q(val.astype(LD) - LD(a_cur))[0]]
        j = path(c, q, val)
        yield c, q, val, slots, j
        if j is None:
            return
        fixed, a_cur = fixed | (j << (BITS * c)), val[j]


def drawn(seed, t, chain, p):
    """path() of the contract's draws: the first lane whose running sum passes mulhi64(U, T); None at T = 0."""
    def path(c, q, val):
        w = om._draw(seed, t, np.array([chain]), 1 + p + 64 * c)
        U, T = int(w[0][0]) | (int(w[1][0]) << 32), sum(q)
        thr, run = (U * T) >> 64, 0
        for j, x in enumerate(q):
            run += x
            if run > thr:
                return j
        return None
    return path


def pick(K, stages, E, sc, x, a, seed, t, chain, p):
    """-> the picked entry i - offsets[v], or -1."""
    last = None
    for last in levels(K, stages, E, sc, x, a, drawn(seed, t, chain, p)):
        pass
    return -1 if last[4] is None else int(E[last[3][last[4]]])


def law(K, stages, E, sc, x, a, px, caps):
    """The probability the restated pick gives the stored set at index px (inside x) as an exact fraction
    (numerator, denominator: Python ints), and law_bound's two parts: the relative e^(2 sum cap) - 1 with
    cap_c the largest of caps[c] over the level's lanes of finite value (c >= 1), and the floors' 64 2^-52
    per chunk."""
    num, den, rel, floors = 1, 1, 0.0, 0.0
    for c, q, val, slots, j in levels(K, stages, E, sc, x, a, lambda c, q, val: (px >> (BITS * c)) & 63):
        T = sum(q)
        assert T > 0
        num, den = num * q[j], den * T
        rel += 2 * float(caps[c][slots[val > -np.inf]].max()) if c >= 1 else 0.0
        floors += 64 * 2.0 ** -52
    return num, den, math.expm1(rel), floors


def run_records(L, tables, staged, seed, chains, records):
    """The records' DAGs restated on GIVEN tables: tables[v] = (C_v, L_v), staged[v] = ([S_1 ..], E_v);
    records: iterable of (t, order (chains, n)).  -> (parents uint64 (R, chains, n), log_weight float64)."""
    n, mem = L.n, [st.members(C) for C, _ in tables]
    pars, lws = [], []
    for t, order in records:
        pre = om.prefixes(order)
        par, chosen = np.zeros((chains, n), dtype=np.uint64), np.zeros((chains, n))
        for c in range(chains):
            for p in range(n):
                v = int(order[c, p])
                x = st.index(mem[v], pre[c, p])
                e = pick(len(mem[v]), staged[v][0], staged[v][1], L.sc[v], x, tables[v][1][x], seed, t, c, p)
                assert e >= 0
                par[c, v], chosen[c, v] = L.sets[v][e], L.sc[v][e]
        pars.append(par)
        lw = np.zeros(chains)
        for v in range(n):
            lw = lw + chosen[:, v]
        lws.append(lw)
    return np.stack(pars), np.stack(lws)
