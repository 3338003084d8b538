"""Plain numpy references of the exact model averaging (csrc/posterior.hip,
ulg_posterior; contract: include/ulg.h).  No GPU, no project binding.

Input: per-variable lists (offsets[n+1], sets, scores): variable v owns the
entries offsets[v] .. offsets[v+1]; a stored set P of v has weight
exp(score), an absent set weight 0.  The model is the order-modular prior: the
pair (linear order, DAG compatible with it) weighs prod_v w_v(Pa_v), so a DAG
counts once per linear extension.

(a) brute(): a sum over all n! orderings in np.longdouble, linear space (each
    variable's scores shifted by their maximum, which cancels in every
    posterior and is added back to ln Z), n <= 7.  It knows nothing of the
    lattice recursions.

(b) lattice(): the recursion of the header in log space, parametrised by
    dtype, in the kernels' operation order, returning every table:
      alpha_v(S) subset sums, bit 0 upward, entry i | bit takes in entry i
      f(S), b(S) layer by layer, the sum over v in S ascending from -inf
      g_v(S) = f(S) + b(V \\ S \\ v), superset sums, bit 0 upward
      t_i = score_i + gamma_v(P_i); L_v = logsumexp of v's t in block order;
      set_logpost = t - L_v; edge[u, v] = exp(logsumexp in block order of v's
      set_logpost with u in the set)
    "block order" is block_logsumexp's: the maximum, then entry k of the
    variable (taken or not) belongs to lane k mod 256, lanes add exp(x - max)
    over their entries ascending, and the 256 lane sums meet in the binary tree
    red[l] += red[l + s], s = 128, 64, .. 1.
    logaddexp(a, b) = max + log1p(exp(-|a - b|)), the maximum itself when the
    other operand is -inf or the gap exceeds `cut` (38 nats in the kernels;
    None = no cut, the longdouble reference's).
"""
import itertools

import numpy as np

CUT = 38.0       # csrc/posterior_dev.h kPostLogAddCut
LANES = 256      # posterior.hip kB
TILE_BITS = 10   # posterior.hip kTileBits: the tile kernel's bit count
COL_BITS = 4     # ... and the bits one strided launch takes
# [within, beyond]: when a list, logaddexp counts its finite operand pairs whose gap lies within 1.5 nats
# of the cut on either side (tests/test_posterior_ref.py: lattice() meets both)
NEAR_CUT = None


def logaddexp(a, b, cut):
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        d = hi - lo
        s = hi + np.log1p(np.exp(-d))
    both = np.isfinite(lo) & np.isfinite(hi)
    if cut is not None:
        if NEAR_CUT is not None:
            NEAR_CUT[0] += int((both & (d > cut - 1.5) & (d <= cut)).sum())
            NEAR_CUT[1] += int((both & (d > cut) & (d < cut + 1.5)).sum())
        both &= ~(d > cut)
    return np.where(both, s, hi)


def squeeze(S, v):
    S = np.asarray(S, dtype=np.int64)
    low = (1 << v) - 1
    return (S & low) | ((S >> 1) & ~low)


def expand(i, v):
    i = np.asarray(i, dtype=np.int64)
    low = (1 << v) - 1
    return (i & low) | ((i & ~low) << 1)


def popcounts(n):
    pc = np.zeros(1 << n, dtype=np.int64)
    for b in range(n):
        pc[1 << b:2 << b] = pc[:1 << b] + 1
    return pc


def block_logsumexp(x, take, dtype):
    """logsumexp of x[take] in the workgroup's order (module docstring)."""
    ninf = dtype(-np.inf)
    if not take.any():
        return ninf
    mx = x[take].max()
    if not mx > ninf:
        return ninf
    with np.errstate(invalid="ignore", over="ignore"):  # entries not taken may lie above the maximum
        e = np.where(take, np.exp(x - mx), dtype(0))
    e = np.where(np.isnan(e), dtype(0), e)
    rows = -(-len(e) // LANES)
    pad = np.zeros(rows * LANES, dtype=dtype)
    pad[:len(e)] = e
    red = np.zeros(LANES, dtype=dtype)
    for r in pad.reshape(rows, LANES):
        red = red + r
    s = LANES // 2
    while s:
        red[:s] = red[:s] + red[s:2 * s]
        s //= 2
    return mx + np.log(red[0])


def lattice(n, offsets, sets, scores, dtype=np.float64, cut=CUT, tables=True):
    """-> dict(log_z, set_logpost, edge, L, alpha, f, b, gamma); gamma is [n, 2^(n-1)]."""
    offsets = np.asarray(offsets, dtype=np.int64)
    sets = np.asarray(sets, dtype=np.uint64).astype(np.int64)
    sc = np.asarray(scores, dtype=np.float32).astype(dtype)
    m, half, full = n - 1, 1 << (n - 1), 1 << n
    ninf = dtype(-np.inf)
    alpha = np.full((n, half), ninf, dtype=dtype)
    for v in range(n):
        sl = slice(offsets[v], offsets[v + 1])
        alpha[v, squeeze(sets[sl], v)] = sc[sl]
    for bit in range(m):
        t = alpha.reshape(n, -1, 2, 1 << bit)
        t[:, :, 1, :] = logaddexp(t[:, :, 1, :], t[:, :, 0, :], cut)
    pc = popcounts(n)
    order = np.argsort(pc, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(pc, minlength=n + 1))])
    f = np.full(full, ninf, dtype=dtype)
    b = np.full(full, ninf, dtype=dtype)
    f[0] = b[0] = 0
    allv = full - 1
    for layer in range(1, n + 1):
        S = order[bounds[layer]:bounds[layer + 1]]
        fa = np.full(len(S), ninf, dtype=dtype)
        ba = np.full(len(S), ninf, dtype=dtype)
        for v in range(n):
            has = ((S >> v) & 1) == 1
            Sv = S[has]
            P = Sv ^ (1 << v)
            with np.errstate(invalid="ignore"):
                fa[has] = logaddexp(fa[has], f[P] + alpha[v, squeeze(P, v)], cut)
                ba[has] = logaddexp(ba[has], alpha[v, squeeze(allv & ~Sv, v)] + b[P], cut)
        f[S], b[S] = fa, ba
    idx = np.arange(half, dtype=np.int64)
    comp = ~idx & (half - 1)
    gamma = np.empty((n, half), dtype=dtype)
    t_all = np.empty(len(sets), dtype=dtype)
    for v in range(n):
        g = f[expand(idx, v)] + b[expand(comp, v)]
        for bit in range(m):
            t = g.reshape(-1, 2, 1 << bit)
            t[:, 0, :] = logaddexp(t[:, 0, :], t[:, 1, :], cut)
        gamma[v] = g
        sl = slice(offsets[v], offsets[v + 1])
        t_all[sl] = sc[sl] + g[squeeze(sets[sl], v)]
    log_z = f[allv]
    lp = np.full(len(sets), ninf, dtype=dtype)
    L = np.full(n, ninf, dtype=dtype)
    edge = np.zeros((n, n), dtype=dtype)
    for v in range(n):
        sl = slice(offsets[v], offsets[v + 1])
        x = t_all[sl]
        L[v] = block_logsumexp(x, np.ones(len(x), dtype=bool), dtype)
        if log_z > ninf and L[v] > ninf:
            with np.errstate(invalid="ignore"):
                lp[sl] = np.where(x > ninf, x - L[v], ninf)
        for u in range(n):
            if u != v:
                l = block_logsumexp(lp[sl], ((sets[sl] >> u) & 1) == 1, dtype)
                edge[u, v] = np.exp(l) if l > ninf else 0
    out = {"log_z": log_z, "set_logpost": lp, "edge": edge, "L": L}
    if tables:
        out.update(alpha=alpha, f=f, b=b, gamma=gamma)
    return out


def brute(n, offsets, sets, scores):
    """All n! orderings in longdouble -> dict(log_z, set_logpost, edge).  n <= 7."""
    assert 1 <= n <= 7
    ld = np.longdouble
    offsets = np.asarray(offsets, dtype=np.int64)
    sets = [int(x) for x in np.asarray(sets, dtype=np.uint64)]
    sc = np.asarray(scores, dtype=np.float32).astype(ld)
    shift = [sc[offsets[v]:offsets[v + 1]].max() if offsets[v + 1] > offsets[v] else ld(0) for v in range(n)]
    w = [np.exp(sc[i] - shift[v]) for v in range(n) for i in range(offsets[v], offsets[v + 1])]
    # A[v][S] = sum of w over v's stored subsets of S, by the definition
    A = [[sum((w[i] for i in range(offsets[v], offsets[v + 1]) if sets[i] & ~S == 0), ld(0)) for S in range(1 << n)]
         for v in range(n)]
    Z = ld(0)
    num = [[ld(0)] * (1 << n) for _ in range(n)]  # per (v, predecessor set): the others' product, summed over orders
    for perm in itertools.permutations(range(n)):
        pred, preds = 0, [0] * n
        for v in perm:
            preds[v] = pred
            pred |= 1 << v
        a = [A[v][preds[v]] for v in range(n)]
        tot = ld(1)
        for x in a:
            tot = tot * x
        Z += tot
        for v in range(n):
            o = ld(1)
            for u in range(n):
                if u != v:
                    o = o * a[u]
            num[v][preds[v]] += o
    with np.errstate(divide="ignore"):
        log_z = np.log(Z) + sum(shift, ld(0))
        lp = np.full(len(sets), ld(-np.inf), dtype=ld)
        edge = np.zeros((n, n), dtype=ld)
        if Z > 0:
            for v in range(n):
                for i in range(offsets[v], offsets[v + 1]):
                    p = w[i] * sum((num[v][S] for S in range(1 << n) if sets[i] & ~S == 0), ld(0)) / Z
                    lp[i] = np.log(p)
                    for u in range(n):
                        if (sets[i] >> u) & 1:
                            edge[u, v] += p
    return {"log_z": log_z, "set_logpost": lp, "edge": edge}


# ---- inputs ------------------------------------------------------------------------
def make_lists(n, kind, seed, max_parents=None, keep=0.3):
    """Lists of one family: (offsets int64, sets uint64, scores float32).
    dense     every subset of V \\ v (up to max_parents)
    sparse    each of them with probability `keep`, the empty set always
    noempty   dense, but the odd variables lack the empty set
    solo      dense, but the last variable's only set is the empty one
    nolist    dense, but the last variable's list is empty (Z = 0)
    dynamic   sparse, scores over +-2e4 nats: a variable's scores lie around
              its anchor (2e3 .. 2e4 in magnitude, either sign) at gaps of 0, 1, 37.5, 38, 38.5 and 500 nats either
              way, so that logaddexp meets gaps on both sides of its cut
    Scores are float32 of either sign."""
    rng = np.random.default_rng(seed)
    k = n - 1 if max_parents is None else min(max_parents, n - 1)
    offs, sets, scores = [0], [], []
    for v in range(n):
        others = [u for u in range(n) if u != v]
        mine = [sum(1 << u for u in c) for r in range(k + 1) for c in itertools.combinations(others, r)]
        if kind in ("sparse", "dynamic"):
            mine = [S for S in mine if S == 0 or rng.random() < keep]
        elif kind == "noempty" and v % 2 == 1:
            mine = [S for S in mine if S != 0]
        elif kind == "solo" and v == n - 1:
            mine = [0]
        elif kind == "nolist" and v == n - 1:
            mine = []
        if kind == "dynamic":
            anchor = rng.uniform(2e3, 2e4) * rng.choice([-1.0, 1.0])
            gaps = rng.choice([0.0, 1.0, 37.5, 38.0, 38.5, 500.0], size=len(mine)) * rng.choice([-1.0, 1.0], size=len(mine))
            val = anchor + gaps + rng.uniform(-0.25, 0.25, size=len(mine))
        else:
            val = rng.uniform(-30.0, 10.0, size=len(mine)) - 2.0 * np.array([bin(S).count("1") for S in mine])
        sets += mine
        scores += list(val)
        offs.append(len(sets))
    return (np.array(offs, dtype=np.int64), np.array(sets, dtype=np.uint64), np.array(scores, dtype=np.float32))


BRUTE_KINDS = ("dense", "sparse", "noempty", "solo", "nolist")
# n - 1 one below, at and one above the tile kernel's bit count, and the first n
# at which a second strided launch occurs (n - 1 = TILE_BITS + COL_BITS + 1)
TABLE_NS = (TILE_BITS, TILE_BITS + 1, TILE_BITS + 2, TILE_BITS + COL_BITS + 2)


def gpu_inputs():
    """name -> (n, offsets, sets, scores): every synthetic input of tests/test_gpu_posterior.py."""
    out = {}
    for n in range(1, 8):
        for kind in BRUTE_KINDS:
            out[f"brute-{kind}-{n}"] = (n,) + make_lists(n, kind, 100 * n + len(kind))
    for n in TABLE_NS:
        out[f"tables-{n}"] = (n,) + make_lists(n, "sparse", 7000 + n, max_parents=3, keep=0.5)
    for n in (6, 9):
        out[f"dynamic-{n}"] = (n,) + make_lists(n, "dynamic", 9000 + n, keep=0.6)
    return out


_REF = {}


def reference(name, n, offsets, sets, scores):
    """The longdouble recursion (the reference), the float64 recursion with the kernels'
    cut, e64 = their largest log-domain deviation over ln Z and every finite set_logpost,
    M = the largest finite |value| of the reference's tables, and the cap
    8 max(e64, 2^-52 (1 + M)).  Computed once per name."""
    if name not in _REF:
        ld = lattice(n, offsets, sets, scores, dtype=np.longdouble, cut=None)
        f64 = lattice(n, offsets, sets, scores, dtype=np.float64, cut=CUT, tables=False)
        e64 = 0.0
        if np.isfinite(ld["log_z"]):
            e64 = float(abs(f64["log_z"] - ld["log_z"]))
        fin = np.isfinite(ld["set_logpost"])
        if fin.any():
            e64 = max(e64, float(np.abs(f64["set_logpost"][fin].astype(np.longdouble) - ld["set_logpost"][fin]).max()))
        M = 0.0
        for key in ("alpha", "f", "b", "gamma"):
            t = ld[key][np.isfinite(ld[key])]
            if t.size:
                M = max(M, float(np.abs(t).max()))
        _REF[name] = {"ld": ld, "f64": f64, "e64": e64, "M": M, "cap": 8.0 * max(e64, 2.0 ** -52 * (1.0 + M))}
    return _REF[name]
