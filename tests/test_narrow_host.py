"""The layer kernels' narrow form on the host (option score_narrow).

host/narrow_check.cpp (urlearning-cpp_amd/bin/narrow_check) runs the two
functions the narrow kernels share with the 64-bit ones, child_ranks_t and
mask_elements (csrc/score_plan.h), over 32-bit masks against the same
functions over 64-bit masks, and CbicPlan's rule for which launches take the
form.  Restated here: a launch is narrow when the option is on, the form is
built for it (variant 241, layer 5 or 6, not a small layer), it has sets,
every variable of the call has at most 32 candidates, its sets plus one block
fit 32 bits and the table has fewer than 2^30 slots (where the plan falls
back to variant 1 anyway).
"""
import math
import os
import subprocess

import pytest

from conftest import PKG

CHECK = os.path.join(PKG, "bin", "narrow_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "narrow_check")


def _full(n, nv=None):
    nv = n if nv is None else nv
    return [(v, (1 << n) - 1) for v in range(nv)]


def _low(m, skip=()):
    """a mask of m candidates from bit 0 up, skipping the given bits"""
    out, b = 0, 0
    while bin(out).count("1") < m:
        if b not in skip:
            out |= 1 << b
        b += 1
    return out


# name: (score_narrow, variant, streams, maxp, n, [(variable, candidate mask)])
SHAPES = {
    "n9_full": (1, 241, 3, 6, 9, _full(9)),
    "n9_off": (0, 241, 3, 6, 9, _full(9)),
    "n9_variant113": (1, 113, 3, 6, 9, _full(9)),              # no narrow kernel for V = 81
    "n9_onepass": (1, 1, 1, 6, 9, _full(9)),
    "n9_k4": (1, 241, 3, 4, 9, _full(9)),                      # small layers only
    "n25_full": (1, 241, 3, 6, 25, _full(25)),                 # C3
    "n33_m32": (1, 241, 3, 6, 33, _full(33, 4)),               # m = 32 everywhere: just inside
    "n34_m33": (1, 241, 3, 6, 34, _full(34, 4)),               # m = 33 everywhere: just outside
    # variables 35 and 34 with 32 candidates (with and without variable 0), the rest 7
    "n36_m32_mixed": (1, 241, 3, 6, 36, [(35, _low(32)), (34, _low(32, skip=(0,))), (1, 0xfd), (2, 0xfb), (3, 0xf7)]),
    # ... and one of them with 33: every launch of the call comes out wide,
    # also the launches of the stream groups that score the small variables
    "n36_m33_mixed": (1, 241, 3, 6, 36, [(35, _low(33)), (34, _low(32, skip=(0,))), (1, 0xfd), (2, 0xfb), (3, 0xf7)]),
    "n36_m33_one_stream": (1, 241, 1, 6, 36, [(35, _low(33)), (34, _low(32, skip=(0,))), (1, 0xfd)]),
    "n64_k6": (1, 241, 3, 6, 64, _full(64)),                   # 2^30 slots or more: variant 1
}


def run_plan(exe, shape, env=None):
    narrow, variant, streams, maxp, n, vm = shape
    args = [exe, "plan", str(narrow), str(variant), str(streams), str(maxp), str(n)] + ["%d:%x" % (v, m) for v, m in vm]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "narrow_check ok: plan" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    plan, launches = None, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "PLAN":
            plan = {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
        elif f[0] == "LAUNCH":
            g, L, ph, sets, nw = map(int, f[1:])
            launches[(g, L, ph)] = (sets, nw)
    return plan, launches


def restate(shape):
    """{(g, L, ph): (sets, narrow)} of the stream groups' unrolled launches"""
    narrow, variant, streams, maxp, n, vm = shape
    maxp = n - 1 if (maxp < 1 or maxp > n - 1) else maxp
    ms = []
    for v, mask in vm:
        c = mask & ((1 << n) - 1) & ~(1 << v)
        ms.append((bin(c).count("1"), bool(c & 1)))
    kmax = max(min(m, maxp) for m, _ in ms)
    slots = sum(math.comb(m, L) for m, _ in ms for L in range(kmax + 1))
    if slots >> 30:
        variant = 1
    two = bool(variant & 16)
    G = max(1, min(streams, len(ms))) if two else 1
    Ls = min(kmax, 8, 4) if two else 0
    fits = max(m for m, _ in ms) <= 32 and slots < (1 << 30)
    out = {}
    for L in range(Ls + 1, min(kmax, 8) + 1):
        for ph in (0, 1):
            for g in range(G):
                cnt = 0
                for i, (m, z) in enumerate(ms):
                    if i % G != g:
                        continue
                    if ph == 0:
                        cnt += math.comb(m - 1, L - 1) if z else 0
                    else:
                        cnt += math.comb(m - 1, L) if z else math.comb(m, L)
                if cnt:
                    nw = narrow and variant == 241 and L in (5, 6) and fits and cnt + 256 <= (1 << 32)
                    out[(g, L, ph)] = (cnt, int(bool(nw)))
    return out


def test_32_bit_ranks_and_elements_equal_the_64_bit_ones():
    r = subprocess.run([CHECK, "ranks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "narrow_check ok" in r.stdout, (r.stdout, r.stderr[-4000:])
    # every set of m <= 12, L <= 6 and of m = 32, L <= 3, and 2 x 2 samples of 20,002 sets
    sets = {L: sum(math.comb(m, L) for m in range(1, 13)) + (math.comb(32, L) if L <= 3 else 0) for L in range(1, 7)}
    sets[5] += 2 * 20002
    sets[6] += 2 * 20002
    assert int(r.stdout.split()[2]) == sum((4 * L + 4) * c for L, c in sets.items())


def test_rule_boundaries():
    r = subprocess.run([CHECK, "rule"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "narrow_check ok: rule" in r.stdout, (r.stdout, r.stderr[-4000:])


@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_picks_the_narrow_launches(name):
    shape = SHAPES[name]
    plan, launches = run_plan(CHECK, shape)
    want = restate(shape)
    assert launches == want, name
    count = sum(nw for _, nw in want.values())
    assert plan["narrow_launches"] == count
    inside = ("n9_full", "n25_full", "n33_m32", "n36_m32_mixed")
    assert (count > 0) == (name in inside), (name, count)
    if name in inside:  # every layer-5 and layer-6 launch with sets
        assert all(nw == 1 for (_, L, _), (_, nw) in want.items() if L in (5, 6))
    if name == "n36_m33_mixed":  # the launches themselves are those of the m = 32 call but one
        assert set(want) == set(restate(SHAPES["n36_m32_mixed"]))
    if name == "n25_full":
        assert count == 12 and want[(0, 6, 1)][0] + want[(1, 6, 1)][0] + want[(2, 6, 1)][0] == 2557324


def test_narrow_check_under_sanitizers():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/narrow_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for mode in ("ranks", "rule"):
        r = subprocess.run([SAN_CHECK, mode], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and "narrow_check ok" in r.stdout, (mode, r.stdout, r.stderr[-4000:])
    for name in ("n9_full", "n33_m32", "n34_m33", "n36_m33_mixed", "n64_k6"):
        run_plan(SAN_CHECK, SHAPES[name], env=env)
