"""The posterior sampler's contract (include/ulg.h, "Sampling"; the kernel is
csrc/posterior_sample.hip) restated in Python integers.  No GPU, no project
binding.

Given the lists, the tables ln alpha_v and ln f (float64: the GPU tests pass the
device's own, read back with ulg_posterior_table, so every x below is the
device's to the bit) and the draws, sample() walks every sample from S = V down
to the empty set and returns every step's choice and its margin.

  draws    Philox4x32-10, key (lo32(seed), hi32(seed)), counter (lo32(k),
           hi32(k), i, 0) -> (w0 .. w3); U_sink = w0 | w1 << 32,
           U_set = w2 | w3 << 32; k the global sample index, i the position.
  weights  sink: v in S ascending, x = (f[S\\v] + alpha_v[S\\v]) - f[S];
           set: v's entries in list order with P subset of S\\v,
           x = float64(s) - alpha_v[S\\v].  q = 0 for x = -inf, else
           floor(exp(x) 2^52) -- exp taken in long double here.
  pick     T = sum q, t = (U T) >> 64, the first j with C_j > t.

The device's FP64 exp is not the long double one.  OCML documents at most 1 ulp
for it (the library's claim, not a measurement); the reference allows 4.  A
product exp(x) 2^52 is at most about 2^52, where an ulp is at most one unit, so
a q moves by at most 4 units and one more for the floor: 8 is taken.  With m
candidates of q > 0 that moves a running sum, and with it t, by at most
slack = 8 (m + 1) units.  (A candidate counts towards m from exp(x) 2^52 >= 1/2
on: one the reference floors to 0 from just below 1 may be 1 on the device.)
A step's margin is the distance in q units from t to the nearer end of the
chosen interval, min(t - C_{j-1}, C_j - t).  A step whose margin is below its
slack is UNDECIDED: the device may differ there and still meet the contract.
tests/test_posterior_sample_ref.py asserts that no input and seed of the GPU
tests has an undecided step (the chance is about 1e-11 per step), so those
tests demand equality everywhere.
"""
import numpy as np

import posterior_ref as pr

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
WEIGHT_BITS = 52
ULP_ALLOWANCE = 8  # q units per candidate (module docstring)


def philox(ctr, key):
    """Philox4x32-10 on Python integers: ctr (c0, c1, c2, c3), key (k0, k1) -> (w0, w1, w2, w3)."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def _philox_np(c0, c1, c2, c3, k0, k1):
    """The same on uint64 arrays that hold 32-bit words."""
    m = np.uint64(M32)
    s = np.uint64(32)
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & m, (p0 >> s) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m, (k1 + np.uint64(PHILOX_W1)) & m
    return c0, c1, c2, c3


def draws(seed, first, count, n):
    """u uint64 (count, n, 2): u[k, i] = (U_sink, U_set) of position i of sample first + k."""
    k = np.repeat(np.arange(first, first + count, dtype=np.uint64), n)
    i = np.tile(np.arange(n, dtype=np.uint64), count)
    w = _philox_np(k & np.uint64(M32), k >> np.uint64(32), i, np.zeros_like(i), seed & M32, (seed >> 32) & M32)
    u = np.empty((count, n, 2), dtype=np.uint64)
    u[:, :, 0] = (w[0] | (w[1] << np.uint64(32))).reshape(count, n)
    u[:, :, 1] = (w[2] | (w[3] << np.uint64(32))).reshape(count, n)
    return u


def weight_q(x):
    """x float64 array -> (q int64 array, m = the candidates that count towards the slack)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(under="ignore"):
        val = np.exp(x.astype(np.longdouble)) * np.longdouble(2.0 ** WEIGHT_BITS)
    val = np.where(x > -np.inf, val, np.longdouble(0))
    q = np.floor(val).astype(np.uint64).astype(np.int64)
    return q, int((val >= 0.5).sum())


def mulhi64(U, T):
    """(U T) >> 64 for a uint64 array U and a Python integer 0 <= T < 2^64, as int64 (T < 2^63 here)."""
    m, s = np.uint64(M32), np.uint64(32)
    u0, u1 = U & m, U >> s
    t0, t1 = np.uint64(T & M32), np.uint64(T >> 32)
    p00, p01, p10, p11 = u0 * t0, u0 * t1, u1 * t0, u1 * t1
    mid = (p00 >> s) + (p01 & m) + (p10 & m)
    return (p11 + (p01 >> s) + (p10 >> s) + (mid >> s)).astype(np.int64)


def pick(q, U):
    """q int64 weights of the candidates, U uint64 array of draws -> (j, margin) per draw; j = len(q)
    and margin -1 where every weight is 0."""
    C = np.cumsum(q)
    T = int(C[-1]) if len(C) else 0
    t = mulhi64(U, T)
    if T == 0:
        return np.full(len(U), len(q), dtype=np.int64), np.full(len(U), -1, dtype=np.int64)
    j = np.searchsorted(C, t, side="right")
    low = np.where(j > 0, C[np.maximum(j - 1, 0)], 0)
    return j, np.minimum(t - low, C[j] - t)


def sample(n, offsets, sets, scores, alpha, f, u):
    """u uint64 (K, n, 2).  -> dict:
    parents uint64 (K, n), order uint8 (K, n), log_weight float64 (K): what the call returns;
    entry int64 (K, n): the list entry chosen at each position;
    sink_margin, set_margin, sink_slack, set_slack int64 (K, n): per position;
    undecided: the steps (either kind) whose margin is below their slack."""
    offsets = np.asarray(offsets, dtype=np.int64)
    sets = np.asarray(sets, dtype=np.uint64).astype(np.int64)
    sc64 = np.asarray(scores, dtype=np.float32).astype(np.float64)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(n, -1)
    f = np.asarray(f, dtype=np.float64)
    u = np.asarray(u, dtype=np.uint64)
    K = u.shape[0]
    assert u.shape == (K, n, 2)
    S = np.full(K, (1 << n) - 1, dtype=np.int64)
    order = np.zeros((K, n), dtype=np.uint8)
    entry = np.zeros((K, n), dtype=np.int64)
    parents = np.zeros((K, n), dtype=np.uint64)
    chosen_score = np.zeros((K, n), dtype=np.float64)
    marg = {key: np.zeros((K, n), dtype=np.int64) for key in ("sink_margin", "set_margin", "sink_slack", "set_slack")}
    for i in range(n - 1, -1, -1):
        for Sg in np.unique(S):
            Sg = int(Sg)
            rows = np.flatnonzero(S == Sg)
            members = [v for v in range(n) if (Sg >> v) & 1]
            with np.errstate(invalid="ignore"):
                x = np.array([(f[Sg ^ (1 << v)] + alpha[v, int(pr.squeeze(Sg ^ (1 << v), v))]) - f[Sg] for v in members])
            q, m = weight_q(x)
            j, margin = pick(q, u[rows, i, 0])
            assert np.all(j < len(members)), "a sink step without a candidate"
            vs = np.array(members, dtype=np.int64)[j]
            order[rows, i] = vs
            marg["sink_margin"][rows, i], marg["sink_slack"][rows, i] = margin, ULP_ALLOWANCE * (m + 1)
            for v in np.unique(vs):
                v = int(v)
                sub = rows[vs == v]
                rest = Sg ^ (1 << v)
                lo, hi = offsets[v], offsets[v + 1]
                idx = lo + np.flatnonzero((sets[lo:hi] & ~rest) == 0)
                q, m = weight_q(sc64[idx] - alpha[v, int(pr.squeeze(rest, v))])
                j, margin = pick(q, u[sub, i, 1])
                assert np.all(j < len(idx)), "a set step without a candidate"
                entry[sub, i] = idx[j]
                parents[sub, v] = sets[idx[j]].astype(np.uint64)
                chosen_score[sub, v] = sc64[idx[j]]
                marg["set_margin"][sub, i], marg["set_slack"][sub, i] = margin, ULP_ALLOWANCE * (m + 1)
                S[sub] = rest
    w = np.zeros(K, dtype=np.float64)
    for v in range(n):
        w = w + chosen_score[:, v]
    out = {"parents": parents, "order": order, "log_weight": w, "entry": entry}
    out.update(marg)
    out["undecided"] = int((marg["sink_margin"] < marg["sink_slack"]).sum() + (marg["set_margin"] < marg["set_slack"]).sum())
    return out


# ---- inputs ------------------------------------------------------------------------
KINDS = ("dense", "sparse", "noempty", "solo")  # posterior_ref.BRUTE_KINDS but "nolist" (Z = 0: nothing to sample)
SMALL_NS = (1, 2, 6, 7)
K_SMALL = 257  # not a multiple of the 4 waves of a workgroup
CUT_VAR = 5    # the variable of the n = 12 lists whose list is cut


def cut_list(offsets, sets, scores, v, keep):
    """Variable v's list cut to its first `keep` entries."""
    lo, hi = int(offsets[v]), int(offsets[v + 1])
    drop = np.arange(lo + keep, hi)
    offs = offsets.copy()
    offs[v + 1:] -= len(drop)
    return offs, np.delete(sets, drop), np.delete(scores, drop)


_INPUTS = None


def gpu_inputs():
    """name -> (n, offsets, sets, scores, K, seed): every input of tests/test_gpu_posterior_sample.py that
    is compared with sample()."""
    global _INPUTS
    if _INPUTS is None:
        out = {}
        base = pr.gpu_inputs()
        for n in SMALL_NS:
            for kind in KINDS:
                out[f"{kind}-{n}"] = base[f"brute-{kind}-{n}"] + (K_SMALL, 1000 + n)
            out[f"dynamic-{n}"] = (n,) + pr.make_lists(n, "dynamic", 9000 + n, keep=0.6) + (K_SMALL, 2000 + n)
        n12 = pr.make_lists(12, "dense", 1212, max_parents=4)  # 562 entries per list: 8 full chunks of 64 and 50
        out["wide-12"] = (12,) + n12 + (K_SMALL, 12)
        for keep in (1, 64, 65):  # one chunk's single pass: the shortest list, the longest, and one past it
            out[f"cut{keep}-12"] = (12,) + cut_list(*n12, CUT_VAR, keep) + (K_SMALL, 1200 + keep)
        out["wide-16"] = (16,) + pr.make_lists(16, "dense", 1616, max_parents=3) + (64, 16)
        _INPUTS = out
    return _INPUTS


_TABLES = {}


def host_tables(name):
    """(alpha, f) of a gpu_inputs() entry by the float64 numpy recursion, once per name."""
    if name not in _TABLES:
        n, offs, sets, scores = gpu_inputs()[name][:4]
        r = pr.lattice(n, offs, sets, scores, dtype=np.float64)
        _TABLES[name] = (r["alpha"], r["f"])
    return _TABLES[name]
