"""The phasing vote's adjacency rows, built on the device (csrc/np2_regions.hip: k_vote_rows_count, k_vote_rows_emit).

The plain pipeline reads the finished rows of the read graph back and the host adopts them as they are.  The sort path
(NP2_EDGE_SORT, or a pair outside the band) still builds its rows on the host from the sorted pair list: it is the
comparison.  Every case checks the polished sequence against the oracle and the graph the decision was taken on
(trace: vote.row_off / vote.rows) bit for bit between the two paths.  The inputs were chosen on the CPU with the oracle's
trace (voting reads, largest partner distance, removed reads) and are pinned by their seeds."""
import numpy as np
import pytest

from nextpolish2_amd import BatchPolisher, Opts, Polisher
from nextpolish2_amd.synth import Synth
from oracle import np2_oracle as orc

pytestmark = pytest.mark.gpu

BAND = 256  # EDGE_BAND: partners b of read a with b - a - 1 < BAND fit the banded accumulator


def _small_diploid():
    return Synth(60000, depth=30, seed=22, diploid=True, read_len_mean=9000.0, read_len_sd=1500.0)  # 195 reads


def _sparse_voters():
    # 152 reads of very uneven length over few markers: 94 of them vote, the others lie between voting reads
    return Synth(40000, depth=12, seed=461, diploid=True, snp_rate=0.0005, hap_indel_rate=0.0002, read_len_mean=3000.0,
                 read_len_sd=2500.0)


def _traced(pol, pileup, opts):
    pol.set_trace(True)
    b, p = pol.polish(pileup, opts)
    out = dict(b=b, p=p, off=pol.trace(0, "vote.row_off"), rows=pol.trace(0, "vote.rows"), lost=pol.trace(0, "invalid_ids"),
               tm=pol.timings())
    pol.set_trace(False)
    return out


def _well_formed(off, rows):
    """Row 0 is empty; every row lists its partners in ascending order (those below it, then those above it), never the
    read itself; every edge has its mirror image with the same weight."""
    assert off[0] == 0 and off[1] == 0 and off[-1] == len(rows)
    src = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off.astype(np.int64)))
    nbr = rows["nbr"].astype(np.int64)
    assert np.all(nbr != src) and np.all(nbr >= 1) and np.all(nbr < len(off) - 1)
    same_row = src[1:] == src[:-1]
    assert np.all(nbr[1:][same_row] > nbr[:-1][same_row])
    fwd = {(int(a), int(b)): float(w) for a, b, w in zip(src, nbr, rows["w"])}
    assert all(fwd.get((b, a)) == w for (a, b), w in fwd.items())


def _check(monkeypatch, s, yaks, opts=None):
    """-> the traced run of the default path, after the checks every case makes."""
    opts = opts or Opts()
    ob, op = orc.Oracle(yaks).polish(s.pileup, opts)
    pol = Polisher(yaks)
    b, p = pol.polish(s.pileup, opts)  # (as in production: the rows are adopted where the read-back left them)
    assert np.array_equal(b, ob) and np.array_equal(p, op)
    dev = _traced(pol, s.pileup, opts)
    monkeypatch.setenv("NP2_EDGE_SORT", "1")
    try:
        srt = _traced(Polisher(yaks), s.pileup, opts)
    finally:
        monkeypatch.delenv("NP2_EDGE_SORT")
    for r in (dev, srt):
        assert np.array_equal(r["b"], ob) and np.array_equal(r["p"], op)
    assert (dev["off"] is None) == (srt["off"] is None)
    if dev["off"] is not None:
        assert dev["off"].tobytes() == srt["off"].tobytes() and dev["rows"].tobytes() == srt["rows"].tobytes()
        assert len(dev["off"]) == len(s.pileup.reads) + 1
        _well_formed(dev["off"], dev["rows"])
        assert "vote_rows" not in srt["tm"] and srt["tm"].get("vote_sort") == 1
    return dev


def test_small_diploid_contig(monkeypatch):
    s = _small_diploid()  # R in the low hundreds: every window of the band is clipped at read 1
    r = _check(monkeypatch, s, [s.yak(21), s.yak(31)])
    assert 100 < len(r["off"]) - 1 < BAND and r["off"][-1] > 1000 and r["tm"].get("vote_rows") == 1


def test_read_count_that_is_no_multiple_of_four(monkeypatch):
    s = Synth(20000, depth=5, seed=402, diploid=True)
    assert len(s.pileup.reads) == 9
    r = _check(monkeypatch, s, [s.yak(21)])
    assert r["off"][-1] > 0


def test_two_or_three_voting_reads(monkeypatch):
    s = Synth(12000, depth=3, seed=433, diploid=True, snp_rate=0.001, hap_indel_rate=0.0)
    r = _check(monkeypatch, s, [s.yak(21)])
    assert len(r["off"]) - 1 == 4 and r["off"][-1] > 0
    assert np.count_nonzero(np.diff(r["off"])) in (2, 3)


def test_haploid_contig_has_no_votes_and_nobody_loses(monkeypatch, small_haploid):
    s, yaks = small_haploid
    r = _check(monkeypatch, s, yaks)
    assert r["off"] is None or r["off"][-1] == 0
    assert r["lost"] is None or len(r["lost"]) == 0


def test_rows_left_in_the_band_by_an_earlier_contig_are_not_read(monkeypatch):
    dense, sparse = _small_diploid(), _sparse_voters()
    assert len(sparse.pileup.reads) < len(dense.pileup.reads)
    yaks = [Synth.yak_assembly([dense, sparse], 21)]
    ob, op = orc.Oracle(yaks).polish(sparse.pileup, Opts())
    fresh = _traced(Polisher(yaks), sparse.pileup, Opts())
    assert np.array_equal(fresh["b"], ob) and np.array_equal(fresh["p"], op)
    for trace in (True, False):
        pol = Polisher(yaks)
        pol.set_trace(trace)
        pol.polish(dense.pileup, Opts())
        if trace:  # (every read of the dense contig votes: it wrote the band rows of all the sparse contig's reads)
            again = _traced(pol, sparse.pileup, Opts())
            off, rows = again["off"], again["rows"]
            assert off.tobytes() == fresh["off"].tobytes() and rows.tobytes() == fresh["rows"].tobytes()
            # reads without a partner that lie inside other reads' windows: their band rows are the dense contig's
            deg = np.diff(off)
            reach = np.zeros(len(deg), dtype=np.int64)  # largest partner of any read up to v
            src = np.repeat(np.arange(len(deg)), deg)
            np.maximum.at(reach, src, rows["nbr"].astype(np.int64))
            reach = np.maximum.accumulate(reach)
            inside = [v for v in range(2, len(deg)) if deg[v] == 0 and reach[v - 1] > v]
            assert len(inside) >= 10
            b, p = again["b"], again["p"]
        else:
            b, p = pol.polish(sparse.pileup, Opts())
        assert np.array_equal(b, ob) and np.array_equal(p, op)


@pytest.mark.parametrize("use_all", [False, True])
def test_reads_flagged_bad_leave_the_rows_unless_all_reads_are_used(monkeypatch, use_all):
    s = _small_diploid()
    yaks = [s.yak(21)]
    r = _check(monkeypatch, s, yaks, Opts(use_all_reads=use_all))
    # The vote kernel flags the reads that disagree with the contig at a marker; without use_all_reads they are removed
    # whatever the Louvain says and are no part of its graph.  A read the Louvain itself removes has neighbours there.
    # So: the removed reads WITHOUT a row are the flagged ones, and there have to be some for this case to test anything.
    kept_out = _traced(Polisher(yaks), s.pileup, Opts(use_all_reads=False))
    deg = np.diff(kept_out["off"])
    flagged = [int(v) for v in kept_out["lost"] if deg[v] == 0]
    assert len(flagged) >= 10
    listed = set(kept_out["rows"]["nbr"].tolist())
    assert not listed & set(flagged)
    if use_all:  # the same reads are part of the graph when every read is used
        deg_all = np.diff(r["off"])
        assert all(deg_all[v] > 0 for v in flagged)
    else:
        assert r["off"].tobytes() == kept_out["off"].tobytes()


def _largest_distance(off, rows):
    src = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off.astype(np.int64)))
    return int((rows["nbr"].astype(np.int64) - src).max()) - 1


def test_largest_partner_distance_just_inside_and_beyond_the_band(monkeypatch):
    inside = Synth(30000, depth=290, seed=790, diploid=True)   # oracle: largest b - a - 1 of a voting pair = 250
    beyond = Synth(30000, depth=310, seed=810, diploid=True)   # ... = 261
    r = _check(monkeypatch, inside, [inside.yak(21)])
    assert r["tm"].get("vote_rows") == 1 and "vote_sort" not in r["tm"]  # the rows came from the device
    assert BAND - 16 <= _largest_distance(r["off"], r["rows"]) < BAND
    r = _check(monkeypatch, beyond, [beyond.yak(21)])
    assert r["tm"].get("vote_sort") == 1 and "vote_rows" not in r["tm"]  # the whole contig took the sort
    assert _largest_distance(r["off"], r["rows"]) >= BAND


def test_batch_of_three_contigs_of_different_size():
    syn = [_small_diploid(), Synth(20000, depth=5, seed=402, diploid=True), _sparse_voters()]
    assert len({len(s.pileup.reads) for s in syn}) == 3
    yaks = [Synth.yak_assembly(syn, 21)]
    pol = Polisher(yaks)
    contigs = [pol.upload(s.pileup) for s in syn]
    single = [pol.polish_resident(c, Opts()) for c in contigs]
    o = orc.Oracle(yaks)
    for s, (b, p) in zip(syn, single):
        ob, op = o.polish(s.pileup, Opts())
        assert np.array_equal(b, ob) and np.array_equal(p, op)
    bp = BatchPolisher(pol, 3)
    for _ in range(2):
        for (b, p), (sb, sp) in zip(bp.polish(contigs, Opts(), want_pos=True), single):
            assert np.array_equal(b, sb) and np.array_equal(p, sp)
    bp.close()
