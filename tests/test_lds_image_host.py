"""The layer launches' LDS images on the host (option score_lds_image).

host/lds_image_check.cpp (urlearning-cpp_amd/bin/lds_image_check) plans one
scoring call with csrc/score_plan.h and checks every image byte for byte
against the arrays it packs: each region at lds_layout's offset, every other
byte (alignment gaps, the aliased carve's counters) zero, the size the
layout's, a multiple of 16, the images back to back.  Restated here: which
launches exist and how many sets each has.  With the default options a
two-pass variant (bit 4) runs layers 1..3 in the fused small kernel (no
image), layer 4 as one launch over all variables, layers 5..8 as one launch
per stream group (variables striped over min(3, nv) groups); variant 1 runs
every layer 1..8 as one launch.  A launch without sets has no image.
"""
import math
import os
import subprocess

import pytest

from conftest import PKG

CHECK = os.path.join(PKG, "bin", "lds_image_check")
SAN_CHECK = os.path.join(PKG, "bin", "san", "lds_image_check")


def _full(n, nv=None):
    nv = n if nv is None else nv
    return [(v, (1 << n) - 1) for v in range(nv)]


# name: (variant, cap, maxp, n, [(variable, candidate mask)])
SHAPES = {
    "n3_nv1": (1, 1 << 20, 2, 3, _full(3, 1)),              # one-pass: layers 1 and 2 are layer launches
    "n3_nv1_fused": (241, 1 << 20, 2, 3, _full(3, 1)),      # both layers in the fused small kernel: no image
    "n9_full": (241, 1 << 20, 6, 9, _full(9)),              # n * n * 8 = 648: no multiple of 16
    "n9_plain": (113, 1 << 20, 6, 9, _full(9)),             # the plain carve at layers 5 and 6
    "n9_nolut": (241, 0, 6, 9, _full(9)),                   # no unrank offsets: their place stays zero
    "n9_onepass": (1, 1 << 20, 6, 9, _full(9)),             # every layer a layer launch
    "n12_mixed": (241, 300, 6, 12, [(3, 0xffe), (0, 0xfff), (7, 0x7fe), (11, 0x0ff)]),
    "n25_full": (241, 1 << 20, 6, 25, _full(25)),
    "n64_k5": (241, 1 << 20, 5, 64, _full(64)),
    "n64_k6": (241, 1 << 20, 6, 64, _full(64)),             # 2^30 slots or more: the plan falls back to variant 1
}


def run_check(exe, shape, env=None):
    variant, cap, maxp, n, vm = shape
    args = [exe, str(variant), str(cap), str(maxp), str(n)] + ["%d:%x" % (v, m) for v, m in vm]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "lds_image_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    plan, imgs = None, []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "PLAN":
            plan = {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
        elif f[0] == "IMG":
            imgs.append(dict(zip(("g", "L", "ph", "off", "bytes", "sets", "aliased", "zeros"), map(int, f[1:]))))
    return plan, imgs


def restate(shape):
    """{(g, L, ph): sets} of the launches that carry an image"""
    variant, cap, maxp, n, vm = shape
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
    G = max(1, min(3, len(ms))) if two else 1
    Ls = min(kmax, 8, 4) if two else 0
    Lf = min(Ls, 3) if (variant & 65) == 65 else 0
    out = {}
    for L in range(Lf + 1, min(kmax, 8) + 1):
        for ph in (0, 1):
            for g in range(1 if L <= Ls else G):
                cnt = 0
                for i, (m, z) in enumerate(ms):
                    if L > Ls and i % G != g:
                        continue
                    if ph == 0:
                        cnt += math.comb(m - 1, L - 1) if z else 0
                    else:
                        cnt += math.comb(m - 1, L) if z else math.comb(m, L)
                if cnt:
                    out[(g, L, ph)] = cnt
    return variant, out


@pytest.mark.parametrize("name", list(SHAPES))
def test_images_match_their_sources(name):
    shape = SHAPES[name]
    plan, imgs = run_check(CHECK, shape)
    variant, want = restate(shape)
    assert plan["variant"] == variant
    assert {(i["g"], i["L"], i["ph"]): i["sets"] for i in imgs} == want, name
    # tables exist for layers 4..8 and at most 32 candidates
    assert plan["lut"] == (0 if name == "n9_nolut" or name.startswith(("n3_", "n64_")) else 1)
    assert bool(imgs) == (name != "n3_nv1_fused")
    end = 0
    for i in sorted(imgs, key=lambda i: i["off"]):
        assert i["off"] == end and i["off"] % 16 == 0 and i["bytes"] % 16 == 0 and i["bytes"] > 0
        end = i["off"] + i["bytes"]
        # the aliased carve: two-pass kernels with the second compaction, bitsets in registers
        assert i["aliased"] == int((variant & 208) == 208 and i["L"] > 4 and i["L"] < 7)
    assert end == plan["bytes"]
    if name == "n25_full":   # C3: the layer-6 aliased image
        assert {i["bytes"] for i in imgs if i["L"] == 6} == {11312}
        assert all(i["aliased"] for i in imgs if i["L"] >= 5)
    if name == "n9_plain":
        assert imgs and not any(i["aliased"] for i in imgs)
    if name == "n9_nolut":   # nv * 4 bytes more are zero than with offsets
        _, with_lut = run_check(CHECK, SHAPES["n9_full"])
        assert [i["zeros"] for i in imgs] != [i["zeros"] for i in with_lut]
        assert [i["bytes"] for i in imgs] == [i["bytes"] for i in with_lut]


def test_lds_image_check_under_sanitizers():
    import fcntl
    with open(os.path.join(PKG, ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", PKG, "bin/san/lds_image_check"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name in ("n3_nv1", "n9_full", "n9_plain", "n9_nolut", "n12_mixed", "n25_full", "n64_k5"):
        _, imgs = run_check(SAN_CHECK, SHAPES[name], env=env)
        assert imgs, name
