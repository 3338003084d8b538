"""A step-counting literal walk of find_best_subset_score (BIC_OLS.cpp:125-172,
SURVEY N3) in plain Python, in the manner of tests/golden/walk_sim.py, with a
step budget.

decide_walk(P, lookup, thr, z, budget) replays the recursion for one parent
set P (a variable mask) whose own score ts is negative (thr = -ts > 0):

  * the parent vector is P's members in ascending order; a child list handed
    down is the first j appended entries followed by zeros, and a zero reads as
    variable 0 (the XOR toggle of VARSET_CLEAR can therefore add variable 0);
  * `checked` starts with the empty set; a node enters it after each call of
    its expansion returns;
  * lookup(T) gives the stored score of T in the finished lists, or None.  The
    cache is seen as it stood when P was scored under the two-phase layer order
    (SURVEY N4): the layers below |P|, plus, when P lacks variable 0, the sets
    of |P| members that contain it.  z says whether variable 0 is a candidate
    at all (a set with variable 0 is never a key when it is not);
  * the walk stops at the first visited key >= thr: the set is dominated.  A
    walk that returns from the root without one means the set is stored.  That
    is the store rule (BIC_OLS.cpp:234 with best starting at 0 < thr).

One step is one turn of the explicit-stack loop, as walk_wide_kernel counts
them with its re-test skipping off.  -> (dominated, steps).  A walk that would
exceed `budget` steps raises BudgetExceeded: a test input that does this is
redesigned, not run."""


class BudgetExceeded(RuntimeError):
    pass


def members(P):
    return [i for i in range(64) if (int(P) >> i) & 1]


def decide_walk(P, lookup, thr, z, budget=10 ** 5):
    P = int(P)
    pv0 = members(P)
    L = len(pv0)
    has0 = bool(P & 1)

    def cached(T):
        pc = bin(T).count("1")
        if pc > L or (pc == L and (has0 or not (T & 1))):
            return None
        if (T & 1) and not z:
            return None
        return lookup(T)

    pv = [[0] * L for _ in range(L + 1)]
    pv[0] = list(pv0)
    Ts = [0] * (L + 1)
    idxs = [0] * (L + 1)
    inner = [0] * (L + 1)
    is_ = [0] * (L + 1)
    js = [0] * (L + 1)
    us = [0] * (L + 1)
    Ts[0] = P
    chk = {0}
    d = 0
    steps = 0
    while True:
        steps += 1
        if steps > budget:
            raise BudgetExceeded(f"set {P:#x}: more than {budget} steps")
        mm = L - d
        if not inner[d]:
            if idxs[d] == mm:
                if d == 0:
                    return False, steps
                d -= 1
                chk.add(Ts[d + 1])
                continue
            u = pv[d][idxs[d]]
            T2 = Ts[d] ^ (1 << u)
            if T2 in chk:
                idxs[d] += 1
                continue
            val = cached(T2)
            if val is not None:
                if val >= thr:
                    return True, steps
                idxs[d] += 1
                continue
            inner[d] = 1
            is_[d] = 0
            js[d] = 0
            us[d] = u
            for k in range(mm - 1):
                pv[d + 1][k] = 0
            continue
        if is_[d] == mm:
            inner[d] = 0
            idxs[d] += 1
            continue
        pi = pv[d][is_[d]]
        is_[d] += 1
        if pi == us[d]:
            continue
        pv[d + 1][js[d]] = pi
        js[d] += 1
        Ts[d + 1] = Ts[d] ^ (1 << us[d])
        idxs[d + 1] = 0
        inner[d + 1] = 0
        d += 1
