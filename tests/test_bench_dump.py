"""bench.py --dump-outputs: the files' names, dtypes and the size cap (no GPU)."""
import os
import sys

import numpy as np

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _lists(total, n=5):
    rng = np.random.default_rng(1)
    offs = np.linspace(0, total, n + 1).astype(np.int64)
    sets = rng.integers(0, 1 << 30, size=total, dtype=np.uint64)
    scores = rng.standard_normal(total).astype(np.float32)
    return offs, sets, scores


def test_dump_writes_the_lists_unchanged(tmp_path):
    offs, sets, scores = _lists(1000)
    bench.dump_outputs(str(tmp_path / "d"), offs, sets, scores)
    assert sorted(os.listdir(tmp_path / "d")) == ["offsets.npy", "scores.npy", "sets.npy"]
    o, s, c = (np.load(tmp_path / "d" / f"{nm}.npy") for nm in ("offsets", "sets", "scores"))
    assert o.dtype == np.float64 and s.dtype == np.float64 and c.dtype == np.float32
    assert np.array_equal(o, offs) and np.array_equal(s.astype(np.uint64), sets)
    assert c.tobytes() == scores.tobytes()


def test_dump_above_the_limit_is_one_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 8192)
    offs, sets, scores = _lists(5000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), offs, sets, scores)
    size = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert size <= 8192
    s, c = np.load(tmp_path / "a" / "sets.npy"), np.load(tmp_path / "a" / "scores.npy")
    assert 0 < len(s) == len(c) < 5000
    # the same positions of both arrays, in list order
    pos = {(int(a), b.tobytes()): i for i, (a, b) in enumerate(zip(sets, scores))}
    idx = [pos[(int(a), b.tobytes())] for a, b in zip(s.astype(np.uint64), c)]
    assert idx == sorted(idx)
    for f in ("offsets.npy", "sets.npy", "scores.npy"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
