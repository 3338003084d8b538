"""A destroyed context gives back every byte it allocated.

ulg_get_info's "device_bytes_live" and "pinned_bytes_live" count what the
process holds through the owning buffers (csrc/dev_buf.h), every context's
together.  Context A (the session's) reads both, context B is created, used
through finished, ordinary calls and closed, and A reads them again: the two
readings must be equal.  Each case drives B through the entry points that
allocate a different part of the state: the scorer's, the search's and the
.pss writer's buffers, the pinned words, the wide layers' tables, the
discrete scorer's slabs.  Before the buffers freed themselves the pair buffer
of score_sets (d_sets_in) was missing from the hand-kept release list, and the
continuous case below failed by 16 B per pair."""
import numpy as np
import pytest
import torch  # noqa: F401  at collection, before any test loads libulg.so: imported after it, torch reports no HIP GPU

import shard
import synth

pytestmark = pytest.mark.gpu

NAMES = ("device_bytes_live", "pinned_bytes_live")


def _live(ctx):
    return tuple(ctx.info(k) for k in NAMES)


def _use_nothing(b):
    pass


def _use_load(b):
    X, _ = synth.gaussian_sem(6, 64, 11)
    b.load(X, 2.0)


def _use_continuous(b):
    n, N, k = 6, 64, 3
    full = [(1 << n) - 1] * n
    X, _ = synth.gaussian_sem(n, N, 11)
    b.load(X, 2.0)
    stored, _ = b.score(list(range(n)), full, k)
    rng = np.random.default_rng(5)
    vs = rng.integers(0, n, 100)
    ps = [int(m) & ~(1 << int(v)) for v, m in zip(vs, rng.integers(0, 1 << n, 100))]
    assert np.isfinite(b.score_sets(vs, ps)).all()
    offs, sets, scores = b.fetch(stored)
    assert offs[-1] == stored > 0
    assert b.pss_format("META x\n", [f"v{i}" for i in range(n)], [N] * n).startswith(b"META x\n")
    b.search_from_scores()
    b.pdb_build()
    exact = b.astar(edges=full, mode=b.ASTAR_EXACT)
    swept = b.astar(edges=full, mode=b.ASTAR_GPU, net_text=False)
    assert np.float32(exact["cost"]).tobytes() == np.float32(swept["cost"]).tobytes()
    one_rank = shard.sharded_sweep(b, n, (1 << n) - 1)  # sweep_shard_begin .. sweep_shard_end
    assert np.float32(one_rank["cost"]).tobytes() == np.float32(swept["cost"]).tobytes()
    assert len(b.mmpc()) == n
    z = b.mmpc_min_z([0, 1], [1, 2], [-1, -1], [0b111000, 0b111000])
    assert np.isfinite(z).all()


def _use_wide(b):
    n, N, k = 11, 64, 9
    X, _ = synth.gaussian_sem(n, N, 12)
    b.load(X, 2.0)
    stored, scored = b.score(list(range(n)), [(1 << n) - 1] * n, k)
    assert 0 < stored <= scored
    assert b.info("score_error_word") == 0


def _use_discrete(b):
    n, N = 6, 200
    arity = [2, 3, 2, 3, 2, 3]
    rng = np.random.default_rng(7)
    codes = np.stack([rng.integers(0, a, N) for a in arity], axis=1)
    full = [(1 << n) - 1] * n
    b.load_discrete(codes, arity)
    for cells in (16384, 8):  # 8: the tables past 8 cells count in the hash slab
        b.set_option("disc_dense_cells", cells)
        stored, _ = b.score_discrete(list(range(n)), full, 3, kind=b.SCORE_BIC, prune=True)
        assert stored > 0
        stored, _ = b.score_discrete(list(range(n)), full, 3, kind=b.SCORE_BDEU, prune=False)
        assert stored > 0
    assert b.info("disc_sparse_sets") > 0
    assert np.isfinite(b.score_sets_discrete([0, 1, 2], [0b110, 0b101, 0b011000])).all()
    assert b.discrete_counts(0, 0b110).sum() == N
    g2, dof, cells = b.g2_discrete([0, 1], [1, 2], [0b100, 0b1000])
    assert np.isfinite(g2).all()
    assert len(b.mmpc_discrete()) == n


@pytest.mark.parametrize("use", [_use_nothing, _use_load, _use_continuous, _use_wide, _use_discrete],
                         ids=["unused", "load", "continuous", "wide", "discrete"])
def test_closed_context_returns_every_byte(ulg_ctx, use):
    import ulg
    before = _live(ulg_ctx)
    b = ulg.Context(0)
    try:
        use(b)
        during = _live(ulg_ctx)
    finally:
        b.close()
    after = _live(ulg_ctx)
    print(dict(zip(NAMES, before)), dict(zip(NAMES, during)), dict(zip(NAMES, after)))
    assert during[0] > before[0]  # the counts are process-wide: A sees B's bytes (at least its binomial tables)
    assert after == before


def test_options_read_back_through_the_abi():
    """ulg_get_info answers every option name with the option as it stands, a
    refused value leaves it alone and keeps the message's form, and the info
    names that are not options still answer."""
    import ulg
    b = ulg.Context(0)
    try:
        assert (b.info("walk_k6"), b.info("wide_host"), b.info("score_unrank_lut")) == (4, 1024, 1 << 20)
        b.set_option("wide_host", (1 << 32) + 1)
        b.set_option("walk_k6", 8)
        assert (b.info("walk_k6"), b.info("wide_host")) == (8, (1 << 32) + 1)
        with pytest.raises(ulg.ULGError, match=r"walk_k6 must be 1, 2, 4 or 8$"):
            b.set_option("walk_k6", 3)
        with pytest.raises(ulg.ULGError, match=r"score_streams must be 1\.\.4$"):
            b.set_option("score_streams", (1 << 32) + 1)
        with pytest.raises(ulg.ULGError, match=r"unknown option: wide_host_iters$"):
            b.set_option("wide_host_iters", 1)
        with pytest.raises(ulg.ULGError, match=r"unknown info: no_such_name$"):
            b.info("no_such_name")
        assert (b.info("walk_k6"), b.info("score_streams")) == (8, 3)
        assert b.info("out_of_time") == 0 and b.info("unrank_lut_entries") == 0
    finally:
        b.close()
