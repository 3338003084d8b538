"""The unrank tables' plan and the set rank out of child_ranks, on the host.

host/unrank_lut_check.cpp (urlearning-cpp_amd/bin/unrank_lut_check) runs
csrc/score_plan.h without a GPU:

  * `plan` prints which tables a scoring call puts into the context's cache
    and the offset every (layer, phase, variable) launch reads.  The rule is
    restated here: a launch (L, ph) of a variable with m candidates unranks
    with (U, l) = (m-1, L-1) in phase 0, (m-1, L) in phase 1 when variable 0
    is a candidate, (m, L) otherwise; a table exists for layers 4..8, U <= 32
    and 0 < C(U, l) <= cap; tables are appended to the cache in the order
    variables, layers, phases first need them and keep their offsets.
  * `ranks` checks, for every set with m <= 12 and L <= 6, that the sum
    child_ranks returns is the set's colex rank.
"""
import math
import os
import subprocess

import pytest

from conftest import PKG

CHECK = os.path.join(PKG, "bin", "unrank_lut_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "unrank_lut_check")


def restate(calls):
    """calls: [(cap, maxp, n, [(v, mask), ...]), ...] on one cache ->
    per call (tables [(U, l, off, count)], offsets {(L, ph, i): off})"""
    cache, total, out = {}, 0, []
    for cap, maxp, n, vm in calls:
        maxp = n - 1 if (maxp < 1 or maxp > n - 1) else maxp
        ms = []
        for v, mask in vm:
            c = mask & ((1 << n) - 1) & ~(1 << v)
            ms.append((bin(c).count("1"), bool(c & 1)))
        kmax = max(min(m, maxp) for m, _ in ms)
        offs = {}
        if cap > 0:
            for i, (m, z) in enumerate(ms):
                for L in range(4, min(kmax, 8) + 1):
                    for ph in (0, 1):
                        if ph == 0 and not z:
                            continue
                        U = m - 1 if (ph == 0 or z) else m
                        l = L - 1 if ph == 0 else L
                        if l > U or U > 32:
                            continue
                        cnt = math.comb(U, l)
                        if cnt == 0 or cnt > cap:
                            continue
                        if (U, l) not in cache:
                            if total + cnt > 2 ** 31 - 1:
                                continue
                            cache[(U, l)] = (total, cnt)
                            total += cnt
                        offs[(L, ph, i)] = cache[(U, l)][0]
        out.append(([(U, l, o, c) for (U, l), (o, c) in cache.items()], offs))
    return out


def run_plan(calls):
    args = [CHECK, "plan"]
    for j, (cap, maxp, n, vm) in enumerate(calls):
        if j:
            args.append("/")
        args += [str(cap), str(maxp), str(n)] + ["%d:%x" % (v, mask) for v, mask in vm]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "CALL":
            out.append(([], {}))
        elif f[0] == "T":
            out[-1][0].append(tuple(int(x) for x in f[1:5]))
        elif f[0] == "O":
            out[-1][1][(int(f[1]), int(f[2]), int(f[3]))] = int(f[4])
    return out


def single(m, z, cap, maxp):
    """one variable with m candidates, variable 0 among them or not"""
    if z:  # variable m scored, candidates 0 .. m-1
        return (cap, maxp, m + 1, [(m, (1 << m) - 1)])
    return (cap, maxp, m + 2, [(1, ((1 << (m + 2)) - 1) & ~1)])  # candidates 2 .. m+1


GRID = [(m, z, cap, L) for m in (3, 4, 5, 7, 8, 9, 12, 20, 31, 32, 33, 34, 40) for z in (False, True)
        for cap in (0, 1, 100, 1000, 1 << 20, 2 ** 31 - 1) for L in (3, 4, 5, 6, 8)
        if not (m >= 31 and L > 6)]


def test_plan_grid_matches_restatement():
    for m, z, cap, L in GRID:  # each on a cache of its own
        calls = [single(m, z, cap, L)]
        got, want = run_plan(calls), restate(calls)
        assert got == want, (m, z, cap, L)
        tables, offs = got[0]
        if cap == 0 or L < 4 or (m - 1 if z else m) > 32:
            assert not tables and not offs, (m, z, cap, L)
        for U, l, _, cnt in tables:
            assert U <= 32 and cnt == math.comb(U, l) <= cap


def test_plan_shares_tables_across_variables_and_calls():
    n = 12
    full = (1 << n) - 1
    call_a = (1 << 20, 6, n, [(v, full) for v in range(n)])
    call_b = (300, 6, n, [(v, full) for v in range(n)])
    call_c = (1 << 20, 5, n, [(v, full & ~1) for v in range(1, n)])   # no variable 0: (m, L) forms
    call_d = (1 << 20, 6, 35, [(v, (1 << 35) - 1) for v in (0, 17, 34)])  # U = 34, 33: no table
    calls = [call_a, call_b, call_c, call_d, call_a]
    got, want = run_plan(calls), restate(calls)
    assert got == want
    # call a: variable 0 (m = 11, no z) and the others (m = 11, z) need 3 + 6 tables
    assert sorted((U, l) for U, l, _, _ in got[0][0]) == sorted(
        [(11, 4), (11, 5), (11, 6)] + [(10, l) for l in (3, 4, 5, 6)])
    # every variable but 0 reads the same offset in a launch
    for L in (4, 5, 6):
        for ph in (0, 1):
            assert len({got[0][1][(L, ph, i)] for i in range(1, n)}) == 1
    # call b (cap 300): variable 0's tables are over the cap, the others' stay
    assert all((L, 1, 0) not in got[1][1] for L in (4, 5, 6))
    assert all((L, ph, 1) in got[1][1] for L in (4, 5, 6) for ph in (0, 1))
    assert got[1][0] == got[0][0]          # nothing added
    assert len(got[2][0]) == len(got[0][0])  # (10, 4..5) are there already
    assert got[3][0] == got[2][0] and not got[3][1]
    assert got[4] == (got[3][0], got[0][1])  # offsets never move


def test_child_ranks_sum_is_the_colex_rank():
    r = subprocess.run([CHECK, "ranks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "unrank_lut_check ok" in r.stdout, (r.stdout, r.stderr)


def test_unrank_lut_check_under_sanitizers():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/unrank_lut_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([SAN_CHECK, "ranks"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "unrank_lut_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    n = 12
    r = subprocess.run([SAN_CHECK, "plan", "300", "6", str(n)] + ["%d:%x" % (v, (1 << n) - 1) for v in range(n)] +
                       ["/", str(1 << 20), "5", "35", "0:7ffffffff", "34:7ffffffff"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "CALL 1" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
