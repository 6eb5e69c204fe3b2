"""The candidate-edge cases (cand_cases.py) on the CPU: every case builds, lands on the geometry it is built for, the oracle
completes, and the oracle's candidate strings are reproduced by a plain restatement of the emission rule working on the
gapped alignment strings — so the expected strings can be re-derived by a reader, and the oracle is checked on inputs it
has never seen."""
import numpy as np
import pytest

import cand_cases as cc


def candidate(aln, start, end):
    """The candidate string of one (read, region) pair (get_lqseqs_from_align_tags, main.rs:1478-1521), from the read's gapped
    alignment (aln_t_s, target, query): every non-gap query letter whose target position lies in
    [max(start, aln_t_s), end], taken from the first non-insertion column of that position on.  An insertion column
    ('-' in the target) belongs to the position before it."""
    ts, t, q = aln
    pos, out, begun = ts - 1, [], False
    for tc, qc in zip(t, q):
        if tc != "-":
            pos += 1
        if pos > end:
            break
        if pos >= max(start, ts):
            begun = begun or tc != "-"
            if begun and qc != "-":
                out.append(qc.upper())
    return "".join(out)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_case_builds_on_its_geometry(name):
    pu, yaks, opts = cc.CASES[name]
    assert pu.L <= 6400 and pu.n_reads <= 131 and len(yaks) == 1
    assert int(pu.reads["aln_t_e"].max()) == pu.L - 1 and int(pu.reads["aln_t_s"][0]) == 0
    cc.geometry(name)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_restated_emission_rule_gives_the_oracles_strings(name):
    ref = cc.expected(name)
    if ref is None:
        pytest.fail("the reference panics on a case built to complete")
    o = ref[0]
    alns = cc.ALNS[name]
    for ps in range(cc.CASES[name][2].iter_count):
        st, en = o.trace(ps, "cand.start").tolist(), o.trace(ps, "cand.end").tolist()
        coff, order = o.trace(ps, "cand.cand_off").tolist(), o.trace(ps, "cand.order").tolist()
        soff, seq = o.trace(ps, "cand.seq_off").tolist(), o.trace(ps, "cand.seq").tobytes().decode()
        assert st == o.trace(ps, "lq.start").tolist() and en == o.trace(ps, "lq.end").tolist()
        assert len(coff) == len(st) + 1 and coff[-1] == len(order) and len(soff) == len(order) + 1 and soff[-1] == len(seq)
        for g in range(len(st)):
            reads = order[coff[g]:coff[g + 1]]
            assert reads == sorted(set(reads)) and len(reads) <= 60  # ascending read index, one candidate a read
            for i in range(coff[g], coff[g + 1]):
                want = candidate(alns[order[i]], st[g], en[g])
                assert want and seq[soff[i]:soff[i + 1]] == want, (name, ps, g, order[i], st[g], en[g])


def test_the_cases_sit_on_both_sides_of_their_edges():
    """what the builders' own assertions cannot see: counts taken from the oracle's candidate lists"""
    def ncand(name):
        return np.diff(cc.expected(name)[0].trace(0, "cand.cand_off")).tolist()
    assert ncand("kept_60") == [60] and ncand("kept_61") == [60] and ncand("kept_64") == [60] and ncand("kept_61_list_70") == [60]
    assert ncand("read_list_64") == [64 - 4 - 5] and ncand("read_list_65") == [65 - 4 - 5]
    for n in (1, 3, 4, 5, 15, 16, 17):
        assert len(ncand(f"counts_{n}")) == n
    # bucket: the records of a tile are the (column, read) pairs off the contig's own node: 12 in tile 0, 13 in tile 1
    o = cc.expected("bucket")[0]
    off, cnt = o.trace(0, "graph.off").astype(np.int64), o.trace(0, "graph.count").astype(np.int64)
    rows = cc.CASES["bucket"][0].n_reads
    assert (cnt[off[:-1]] >= rows - 4).all()  # the first node of a position is the contig's
    extra = np.add.reduceat(cnt, off[:-1]) - cnt[off[:-1]]
    assert [int(extra[t * 1024:(t + 1) * 1024].sum()) for t in range(3)] == [12, 13, 0] and max(cc.BUCKET_CAPS) > 13 > 12 > min(cc.BUCKET_CAPS)
    # read_ends: the reads ending at end - 1 and before are not paired, the one ending at end is
    o = cc.expected("read_ends")[0]
    order = o.trace(0, "cand.order").tolist()
    pu = cc.CASES["read_ends"][0]
    (s, e), = cc.REGIONS["read_ends"][0]
    te = pu.reads["aln_t_e"].tolist()
    assert [r for r in range(pu.n_reads) if te[r] >= e] == order and min(te) == e - 1
    # read_starts: paired iff the read starts at or before the region's start
    o = cc.expected("read_starts")[0]
    pu = cc.CASES["read_starts"][0]
    (s, e), = cc.REGIONS["read_starts"][0]
    ts = pu.reads["aln_t_s"].tolist()
    assert [r for r in range(pu.n_reads) if ts[r] <= s] == o.trace(0, "cand.order").tolist()
    assert ts[1] == e + 2 and ts[2] == s + 4 and max(ts) == e + 30 and {s - 1, s, s + 1, s + 2, e, e + 1} <= set(ts)
