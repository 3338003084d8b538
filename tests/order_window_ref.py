"""ulg_order_window's contract (include/ulg.h, "Order search"; the kernel is
csrc/order_window.hip) restated directly: numpy float64 adds, Python integer masks,
the DP layer by layer over arrays indexed by the local mask.  No GPU, no project
binding, and deliberately not the kernel's scatter and subset-max: a beta table is
raised entry by entry over every mask that contains the entry's window part, and
the final terms and parents are order_search_ref.order_best's, which run() holds
equal to the terms the windows wrote.

Every value is a maximum of float32 scores or a fixed FP64 sum of such: the device
must give the same bits, and the GPU tests ask for equality.

`events` collects what a call has met: "accepted", "rejected" (a window left as it
was), "repaired" (a present sum of -inf replaced), "clamped" (a last start that is
not a multiple of the stride), "converged" (stopped by a sweep that accepted
nothing), "capped" (stopped by max_sweeps after a sweep that accepted one).
"""
import numpy as np

import order_mcmc_ref as om
import order_search_ref as osr

F64 = np.float64

# the GPU tests' cases: (input, width, stride, max_sweeps)
CASES = [("n5", 5, 1, 4), ("n5", 2, 1, 8), ("n5", 3, 2, 1), ("n5", 12, 0, 2), ("n8", 8, 4, 4), ("n8", 3, 2, 8),
         ("n33", 6, 3, 3), ("n33", 7, 7, 2), ("n63", 6, 6, 2), ("n63", 12, 6, 2)]


def starts(n, w, stride):
    a, out = 0, [0]
    while a != n - w:
        a = min(a + stride, n - w)
        out.append(a)
    return out


def betas(L, xs, U):
    """beta[j][M] = b_{x_j}(U + V(M)) for every local mask M (read where j is not in M): each stored set
    inside U + V(full) raises the masks that contain its window part."""
    w, Ms = len(xs), np.arange(1 << len(xs))
    full = sum(1 << x for x in xs)
    out = []
    for x in xs:
        b = np.full(1 << w, -np.inf)
        for S, s in zip(L.sets[x].tolist(), L.sc[x].tolist()):
            if S & ~(U | full) or (S >> x) & 1:
                continue
            part = sum(1 << i for i in range(w) if (S >> xs[i]) & 1)
            b = np.where((part & ~Ms) == 0, np.maximum(b, s), b)
        out.append(b + 0.0)  # -0 reads +0
    return out


def window(L, order, terms, a, w):
    """One window at start a; order and terms are rewritten when it is accepted (-> True)."""
    U = sum(1 << v for v in order[:a])
    xs = order[a:a + w]
    beta, Ms = betas(L, xs, U), np.arange(1 << w)
    size = np.array([bin(M).count("1") for M in Ms])
    Fm = np.full(1 << w, -np.inf)
    Fm[0] = 0.0
    c = np.array([0] + [(M & -M).bit_length() - 1 for M in range(1, 1 << w)])  # the least j of M
    for k in range(1, w + 1):
        for j in range(w):  # ascending: a later j must be strictly better
            sel = Ms[(size == k) & ((Ms >> j) & 1 == 1)]
            cand = Fm[sel & ~(1 << j)] + beta[j][sel & ~(1 << j)]
            better = cand > Fm[sel]
            Fm[sel[better]], c[sel[better]] = cand[better], j
    present = F64(0.0)
    for t in terms[a:a + w]:
        present = present + t
    full = (1 << w) - 1
    assert Fm[full] >= present
    if not Fm[full] > present:
        return False
    M = full
    while M:
        j, p = int(c[M]), a + bin(M).count("1") - 1
        M &= ~(1 << j)
        order[p], terms[p] = xs[j], F64(beta[j][M])
    return True


def run(L, order, width, stride, max_sweeps, events=None, trace=None):
    """ulg_order_window for one order -> (order list, terms, S, parents list, accepted, sweeps); trace
    receives S after every window."""
    events = set() if events is None else events
    n, order = L.n, [int(v) for v in order]
    w = min(width, n)
    stride = min(stride or max(1, width // 2), w)
    terms, accepted, sweeps = list(osr.order_best(L, order)[0]), 0, 0
    while sweeps < max_sweeps:
        sweeps, any_ = sweeps + 1, False
        for a in starts(n, w, stride):
            repaired = not np.isfinite(sum(terms[a:a + w]))
            took = window(L, order, terms, a, w)
            accepted, any_ = accepted + took, any_ or took
            events.add("accepted" if took else "rejected")
            events |= ({"repaired"} if took and repaired else set()) | ({"clamped"} if a % stride else set())
            if trace is not None:
                trace.append(sum(terms))
        if not any_:
            break
    events.add("capped" if any_ else "converged")
    terms_final, parents = osr.order_best(L, order)
    assert np.array_equal(terms_final, terms)
    S = F64(0.0)
    for t in terms:
        S = S + t
    return order, terms_final, S, parents, accepted, sweeps


def run_many(L, orders, width, stride, max_sweeps, events=None):
    """... for several orders -> the binding's dict."""
    rows = [run(L, o, width, stride, max_sweeps, events) for o in orders]
    n = L.n
    return {"orders": np.array([r[0] for r in rows], dtype=np.uint8).reshape(-1, n), "terms": np.array([r[1] for r in rows]).reshape(-1, n),
            "score": np.array([r[2] for r in rows]), "parents": np.array([r[3] for r in rows], dtype=np.uint64).reshape(-1, n),
            "accepted": np.array([r[4] for r in rows], dtype=np.int64), "sweeps": np.array([r[5] for r in rows], dtype=np.int64)}


def case_orders(name, count=4):
    """The GPU tests' orders of an input: the first shuffled orders of its seed, and for n5 the order whose
    first variable has no empty set (a -inf term)."""
    L, seed = osr.inputs()[name][:2]
    orders = [[int(v) for v in om.shuffle(seed, [c], L.n)[0]] for c in range(count)]
    return orders + ([[0, 1, 2, 3, 4]] if name == "n5" else [])
