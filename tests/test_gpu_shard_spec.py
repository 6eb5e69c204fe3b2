"""The early start of a shard's next pass (np2_shard_vote) and its settlement (np2_shard_apply): the pass goes out on the
reads the vote kernel flagged while the votes are merged and decided elsewhere; the decision then removes exactly those
(the pass stands), other reads as well (they go too, the pass starts again) or keeps a flagged read (it comes back, the
pass starts again).  Whatever list is applied, a run that starts early and one that does not (NP2_NO_SPECULATE) must end
with the same bytes; with the contig-wide decision itself both equal the oracle."""
import re

import numpy as np
import pytest

from nextpolish2_amd import Opts, Polisher
from nextpolish2_amd.api import ShardRun, shard_plan, vote_decide
from nextpolish2_amd.dist import stitch_shards
from oracle.np2_oracle import Oracle

pytestmark = pytest.mark.gpu
HALO, VERIFY = 12000, 1024
APPLY = re.compile(r"\[np2 shard\] apply: (\d+) removed here, (\d+) beyond the flagged ones, (\d+) flagged ones kept")


def _applied(variant, D, F, extra):
    """The list one phasing pass applies: (a) the decision, (b) without its first flagged read, (c) plus one other read,
    (d) both, (e) nothing.  No flagged read in the pass: (a) and (c) are all there is."""
    if not len(F):
        variant = {"b": "a", "d": "c", "e": "a"}.get(variant, variant)
    if variant == "e":
        return np.zeros(0, dtype=np.uint32)
    keep = np.ones(len(D), dtype=bool)
    if variant in "bd":
        keep[np.flatnonzero(np.isin(D, F))[0]] = False
    out = D[keep]
    if variant in "cd":
        out = np.sort(np.append(out, np.uint32(extra)))
    return out.astype(np.uint32)


def _sharded(pol, pileup, plans, opts, variant, capfd, monkeypatch, switch=None):
    """Both shards through the protocol with `variant` applied in every phasing pass -> stitched (bases, pos), flagged reads
    per pass, and per pass and shard that started early: ((removed, beyond, kept) expected from the votes, ... logged).
    `switch`: set while the shards' contexts are created (a context reads the switches when it is created)."""
    reads = pileup.reads
    both = np.flatnonzero((reads["aln_t_e"] >= max(pl.zone_lo for pl in plans)) & (reads["aln_t_s"] < min(pl.zone_hi for pl in plans))
                          & ((reads["flags"] & 1) == 0))
    both = both[both > 0]
    for name in ("NP2_NO_SPECULATE", "NP2_TEST_MISSPECULATE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("NP2_SHARD_SPEC_LOG", "1")
    if switch:
        monkeypatch.setenv(switch, "1")
    ctxs = [pol.clone() for _ in plans]
    if switch:
        monkeypatch.delenv(switch)
    runs = [ShardRun(c, pileup, pl, opts, VERIFY) for c, pl in zip(ctxs, plans)]
    gone, n_flagged, counts = set(), [], []
    try:
        while runs[0].passes_left() > 1:
            votes = [r.vote() for r in runs]
            D = vote_decide(votes, pileup.n_reads, opts)
            flagged = [set(v.read_id[(v.flags & 4) != 0].tolist()) for v in votes]
            F = np.array(sorted(set().union(*flagged)), dtype=np.uint32)
            assert np.all(np.isin(F, D))  # (main.rs:977: the decision removes every flagged read)
            extra = next(int(r) for r in both if r not in gone and r not in set(D.tolist()))
            lst = _applied(variant, D, F, extra)
            capfd.readouterr()
            for r in runs:
                r.apply(lst)
            logged = [tuple(int(x) for x in m) for m in APPLY.findall(capfd.readouterr().err)]
            expect = []
            for pl, fl in zip(plans, flagged):
                if not fl:
                    continue  # (no flagged read, no early start, no line)
                local = [int(x) for x in lst if pl.read_lo <= x < pl.read_hi]
                expect.append((len(local), sum(x not in fl for x in local), len(fl - set(lst.tolist()))))
            counts.append((expect, logged))
            n_flagged.append(len(F))
            gone.update(lst.tolist())
        pieces = [r.final() for r in runs]
        b, p = stitch_shards(pieces, plans, VERIFY)
        return np.array(b), np.array(p), n_flagged, counts
    finally:
        for r in runs:
            r.close()


@pytest.mark.parametrize("opts", [Opts(), Opts(iter_count=3)], ids=["two-passes", "three-passes"])
def test_early_start_of_a_shard_settles_to_the_same_bytes_whatever_is_applied(opts, small_diploid, monkeypatch, capfd):
    s, yaks = small_diploid
    ob, op = Oracle(yaks).polish(s.pileup, opts)
    plans = shard_plan(s.pileup, 2, HALO)
    pol = Polisher(yaks)
    for variant in "abcde":
        b1, p1, n_flagged, counts = _sharded(pol, s.pileup, plans, opts, variant, capfd, monkeypatch)
        b0, p0, n_flagged0, counts0 = _sharded(pol, s.pileup, plans, opts, variant, capfd, monkeypatch, "NP2_NO_SPECULATE")
        print(f"variant {variant}: flagged per pass {n_flagged}; per pass (expected, logged) (removed, beyond, kept) per shard: {counts}")
        assert np.array_equal(b1, b0) and np.array_equal(p1, p0), variant
        assert n_flagged == n_flagged0 and any(n_flagged)  # (at least one pass with flagged reads: nothing here is vacuous)
        assert all(not logged for _, logged in counts0)  # (no early start, nothing to settle)
        if variant == "a":
            assert np.array_equal(b1, ob) and np.array_equal(p1, op)
        for (expect, logged), nf in zip(counts, n_flagged):
            assert logged == expect, (variant, expect, logged)
            if not nf:
                continue
            beyond, kept = sum(x[1] for x in logged), sum(x[2] for x in logged)
            if variant in "bde":
                assert kept > 0, (variant, logged)
            if variant in "cd":
                assert beyond > 0, (variant, logged)
            if variant in "ac":
                assert kept == 0, (variant, logged)
            # ((a) is not all zeros: a read of the halo that only the neighbour's regions flag lies beyond this shard's flags —
            # 14 and 13 of the 65 and 61 reads the two shards remove here —, so `beyond` is held to the count worked out from
            # the votes above, which is 0 wherever a shard flagged every read it loses)
    b2, p2, _, _ = _sharded(pol, s.pileup, plans, opts, "a", capfd, monkeypatch, "NP2_TEST_MISSPECULATE")
    assert np.array_equal(b2, ob) and np.array_equal(p2, op)
