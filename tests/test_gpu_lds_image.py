"""The layer launches' LDS images (option score_lds_image).

With the option on, every block of a layer launch copies its constants --
Gram matrix, binomials, work prefixes, unrank offsets, slab offsets, metadata,
candidate lists -- from one host-packed image in 16-byte pieces; with it off,
from the separate arrays in seven loops.  Neither touches the arithmetic of a
score: on every shape below both must give the same offsets, the same sets
and the same score BITS, with the error word 0.  What each shape can break:

  n=9  k=6 full       252 layer-6 sets in one block; the image is shorter than
                      two passes of the block (the tail piece)
  n=12 k=6 edges      mixed candidate counts, variables without variable 0;
  ... constrained     the twin kernels: the constraint table sits in LDS
                      behind the layout and must survive the padded copy
  n=35 k=5, 3 vars    an image over 12 KB: a fourth piece for some threads
  n=40 k=4, 2 vars    15.6 KB, all four unrolled passes nearly full
  n=44 k=4, 2 vars    18.3 KB: more than 4 * 256 pieces, the strided loop
  variant 113         the plain carve at layers 5 and 6
  two loads           one context, X1 then X2: a stale Gram mirror or image
  async rounds        three contexts in flight, graph replay, then the option
                      changes (a new graph key)
"""
import numpy as np
import pytest

import synth
from test_gpu_unrank_lut import CONS12, _edges12, _full, _run, _same

pytestmark = pytest.mark.gpu

LAMBDA = 2.0


def _pair(n, picks):
    return list(picks), [(1 << n) - 1] * len(picks)


# name: (n, N, k, (variables, candidates), constraints, score_variant, least bytes of a launch's image, most)
SHAPES = {
    "n9_full": (9, 300, 6, _full(9), None, None, 0, 2 * 256 * 16),
    "n12_edges": (12, 400, 6, _edges12(), None, None, 0, 1 << 20),
    "n12_edges_cons": (12, 400, 6, _edges12(), CONS12, None, 0, 1 << 20),
    "n35_k5_three": (35, 200, 5, _pair(35, (0, 17, 34)), None, None, 3 * 256 * 16 + 1, 4 * 256 * 16),
    "n40_k4_two": (40, 200, 4, _pair(40, (0, 39)), None, None, 3 * 256 * 16 + 1, 4 * 256 * 16),
    "n44_k4_two": (44, 200, 4, _pair(44, (0, 43)), None, None, 4 * 256 * 16 + 1, 1 << 20),
    "n12_variant113": (12, 300, 6, _full(12), None, 113, 0, 1 << 20),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_image_changes_nothing(name):
    import ulg
    n, N, k, (variables, cands), cons, variant, least, most = SHAPES[name]
    X, _ = synth.gaussian_sem(n, N, 9300 + n)
    ctx = ulg.Context(0)
    try:
        assert ctx.info("score_lds_image") == 1
        ctx.load(X, LAMBDA)
        if cons:
            ctx.set_constraints(cons)
        if variant is not None:
            ctx.set_option("score_variant", variant)
        ctx.set_option("score_lds_image", 0)
        off = _run(ctx, variables, cands, k)
        assert ctx.info("lds_image_bytes") == 0
        ctx.set_option("score_lds_image", 1)
        on = _run(ctx, variables, cands, k)
        _same(off, on, name)
        # the plan's own images for this call (host/lds_image_check.cpp prints
        # them): the context built exactly those, and their sizes place the
        # shape in the pass of the copy it is here for
        from test_lds_image_host import CHECK, run_check
        _, imgs = run_check(CHECK, (variant or 241, 1 << 20, k, n, list(zip(variables, cands))))
        assert imgs and ctx.info("lds_image_bytes") == sum(i["bytes"] for i in imgs)
        assert all(least <= i["bytes"] <= most for i in imgs), [i["bytes"] for i in imgs]
        again = _run(ctx, variables, cands, k)  # the same call: graph replay, nothing uploaded
        _same(on, again, (name, "again"))
    finally:
        ctx.close()


def test_second_load_replaces_gram_and_image():
    import ulg
    n, N, k = 12, 300, 6
    variables, cands = _full(n)
    X1, _ = synth.gaussian_sem(n, N, 9312)
    X2, _ = synth.gaussian_sem(n, N, 9313)
    ctx, fresh = ulg.Context(0), ulg.Context(0)
    try:
        ctx.load(X1, LAMBDA)
        first = _run(ctx, variables, cands, k)
        ctx.load(X2, LAMBDA)
        second = _run(ctx, variables, cands, k)
        fresh.load(X2, LAMBDA)
        want = _run(fresh, variables, cands, k)
        _same(want, second, "second load")
        assert not np.array_equal(first[2].view(np.uint32), second[2].view(np.uint32))
        fresh.set_option("score_lds_image", 0)
        _same(_run(fresh, variables, cands, k), second, "second load, arrays")
    finally:
        ctx.close()
        fresh.close()


def test_async_rounds_and_option_change():
    import ulg
    n, N, k = 12, 300, 6
    variables, cands = _full(n)
    ctxs = [ulg.Context(0) for _ in range(3)]
    try:
        refs = []
        for j, ctx in enumerate(ctxs):
            X, _ = synth.gaussian_sem(n, N, 9320 + j)
            ctx.load(X, LAMBDA)
            ctx.set_option("score_lds_image", 0)
            refs.append(_run(ctx, variables, cands, k))
        for flag in (1, 1, 0, 1):  # capture, replay, the key changes, and back
            for ctx in ctxs:
                ctx.set_option("score_lds_image", flag)
                ctx.score_async(variables, cands, k)
            for ctx, ref in zip(ctxs, refs):
                st, _ = ctx.score_finish()
                assert ctx.info("score_error_word") == 0, flag
                offs, sets, scores = ctx.fetch(st)
                _same(ref, (offs, sets, scores), ("async", flag))
    finally:
        for ctx in ctxs:
            ctx.close()
