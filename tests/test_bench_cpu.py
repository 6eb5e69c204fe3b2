"""bench.py's --dump-outputs writer (no GPU): file names, dtypes, and the seeded sample beyond the size budget."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _bases(n, seed):
    return np.frombuffer(np.random.default_rng(seed).choice(list(b"ACGT"), n).astype(np.uint8).tobytes(), dtype=np.uint8)


def test_dump_whole_outputs(tmp_path):
    bases = [_bases(1000, 1), _bases(2500, 2)]
    bench.dump_outputs(str(tmp_path), bases, [(3, 1002), (0, 2499)])
    assert sorted(os.listdir(tmp_path)) == ["contig_lengths.npy", "polished_bases.npy", "spans.npy"]
    pb = np.load(tmp_path / "polished_bases.npy")
    assert pb.dtype == np.float32 and np.array_equal(pb.astype(np.uint8), np.concatenate(bases))
    assert np.array_equal(np.load(tmp_path / "contig_lengths.npy"), [1000.0, 2500.0])
    sp = np.load(tmp_path / "spans.npy")
    assert sp.dtype == np.float64 and np.array_equal(sp, [[3, 1002], [0, 2499]])


def test_dump_samples_beyond_the_budget(tmp_path):
    bases = [_bases(200_000, 3), _bases(150_000, 4)]
    budget = 256 << 10
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bases, [(0, 1), (0, 1)], budget=budget)
    files = os.listdir(tmp_path / "a")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    idx = np.load(tmp_path / "a" / "polished_bases_index.npy")
    pb = np.load(tmp_path / "a" / "polished_bases.npy")
    assert idx.dtype == np.float64 and pb.dtype == np.float32 and idx.size == pb.size > 10_000
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(pb.astype(np.uint8), np.concatenate(bases)[idx.astype(np.int64)])
    for f in files:  # a fixed sample: the same files every time
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    assert bench.DUMP_BYTES == 64 << 20
