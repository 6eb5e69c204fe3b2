"""The rows form of the phasing vote without a GPU.  Under NP2_VOTE_COMPACT np2_vote_decide restates on the host what the
vote kernels hand to the plain pipeline — the finished adjacency rows of the read graph (partners below a read, then
those above it, flagged reads left out, weights already decided) — and the graph adopts them as they are.  The decision
must be the one the default form (sorted pairs, rows built by the graph itself) gives."""
import numpy as np
import pytest

from nextpolish2_amd import Opts
from nextpolish2_amd.api import Np2Error, vote_decide

from test_shard_cpu import _random_votes, _vote


def _both_forms(monkeypatch, v, n_reads, opts):
    monkeypatch.delenv("NP2_VOTE_COMPACT", raising=False)
    want = vote_decide([v], n_reads, opts)
    monkeypatch.setenv("NP2_VOTE_COMPACT", "1")
    try:
        return want, vote_decide([v], n_reads, opts)
    finally:
        monkeypatch.delenv("NP2_VOTE_COMPACT", raising=False)


def test_random_votes_are_decided_alike_in_both_forms(monkeypatch):
    rng = np.random.default_rng(17)
    n_bad = n_lost = 0
    for _ in range(300):
        n_reads = int(rng.integers(12, 61))
        m = min(n_reads - 1, 40)
        reads, pairs, first, refw, bad = _random_votes(rng, n_reads, int(rng.integers(5, max(6, m * (m - 1) // 4))))
        n_bad += len(bad)
        v = _vote(reads.tolist(), pairs, first, refw, bad, set(refw))
        for use_all in (False, True):
            want, got = _both_forms(monkeypatch, v, n_reads, Opts(use_all_reads=use_all))
            assert np.array_equal(got, want), (n_reads, use_all)
            n_lost += len(want)
    assert n_bad > 100 and n_lost > n_bad  # (flagged reads took part, and the votes removed others as well)


def _far_pair_vote(gap):
    """A small vote in which the reads 1 and 1 + gap disagree, next to a few close pairs."""
    a, b = 1, 1 + gap
    pairs = {(a, b): (0, 4), (a, 2): (3, 0), (2, 3): (2, 1), (b, b + 1): (3, 0), (b + 1, b + 2): (1, 3), (3, 4): (0, 3)}
    reads = sorted({r for ab in pairs for r in ab})
    first = {r: 1000 + 10 * i for i, r in enumerate(reads)}
    refw = {reads[0]: 2, reads[-1]: -1}
    return _vote(reads, pairs, first, refw, set(), set(refw)), b + 4


def test_a_pair_at_the_band_edge_goes_through(monkeypatch):
    v, n_reads = _far_pair_vote(256)  # b - a - 1 == 255: the last column of the kernels' band
    for use_all in (False, True):
        want, got = _both_forms(monkeypatch, v, n_reads, Opts(use_all_reads=use_all))
        assert np.array_equal(got, want)


def test_a_pair_beyond_the_band_is_refused_in_the_rows_form(monkeypatch):
    v, n_reads = _far_pair_vote(257)
    monkeypatch.delenv("NP2_VOTE_COMPACT", raising=False)
    vote_decide([v], n_reads, Opts())  # (the default form takes it)
    monkeypatch.setenv("NP2_VOTE_COMPACT", "1")
    with pytest.raises(Np2Error) as e:
        vote_decide([v], n_reads, Opts())
    assert "NP2_E_UNSUPPORTED" in str(e.value)
