"""The trio scan on the device (np2_trio_strings, np2_trio_device, python -m nextpolish2_amd.trio, the command line's
--trio) against the numpy brute force of tests/test_trio_cpu.py, a known answer on a synthetic diploid contig, and
Polisher.lookup_hashes (the polish kernels' own lookup, aggregated in numpy) as an independent device path.

Every case is one bounded subprocess or a handful of in-process calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nextpolish2_amd import Opts, Polisher, api, trio
from nextpolish2_amd import io as np2io
from nextpolish2_amd._types import Yak
from nextpolish2_amd.synth import Synth
from test_gpu_qv import HALO, TILE, crowded, dump_of, edge_sequences, noisy, random_bases, yak_table
from test_kcount_cpu import numpy_count
from test_qv_cpu import kmer_hashes_at
from test_trio_cpu import aggregate, classes, numpy_trio, table_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
E_ARG = -1
K = 21


def parent_yak(seq, k, times=5):
    """the table of one parent: its sequence counted `times` times over"""
    return Yak(k, *numpy_count((seq + b"\n") * times, k))


def scaled_yak(seq, k, times=5):
    """the same table for a long sequence: counted once, every count multiplied"""
    words, off = numpy_count(seq + b"\n", k)
    c = np.minimum((words & np.uint64(1023)) * np.uint64(times), np.uint64(1023))
    return Yak(k, (words & ~np.uint64(1023)) | c, off)


def stats_row(r, i):
    return tuple(int(x) for x in r.stats[i])


def same_as_numpy(pol, k, tp, tm, seqs, min_count, mid_count, pat_idx=0, mat_idx=1):
    """struct fields and both bitmaps of every sequence == the brute force"""
    r = pol.trio_strings(pat_idx, mat_idx, seqs, min_count, mid_count, bits=True)
    assert r.stats.shape == (len(seqs), 7) and len(r.pat_bits) == len(r.mat_bits) == len(seqs)
    for i, s in enumerate(seqs):
        e_stats, e_pb, e_mb = numpy_trio(s, k, tp, tm, min_count, mid_count)
        assert stats_row(r, i) == e_stats, (k, min_count, mid_count, i, len(s))
        assert np.array_equal(r.pat_bits[i], e_pb) and np.array_equal(r.mat_bits[i], e_mb), (k, min_count, mid_count, i, len(s))
    # the bitmaps nobody asked for change nothing
    r2 = pol.trio_strings(pat_idx, mat_idx, seqs, min_count, mid_count)
    assert np.array_equal(r2.stats, r.stats) and r2.pat_bits is None and r2.mat_bits is None
    return r


def lookup_counts(pol, k, seq, pat_idx=0, mat_idx=1):
    """(valid, c_P, c_M) per base through the polish kernels' lookup of both tables (np2_lookup_hashes at threshold 1)"""
    valid, hashes = kmer_hashes_at(seq, k)
    cp, cm = np.zeros(len(valid), np.uint32), np.zeros(len(valid), np.uint32)
    cp[valid] = pol.lookup_hashes(pat_idx, hashes[valid], 1)
    cm[valid] = pol.lookup_hashes(mat_idx, hashes[valid], 1)
    return valid, cp, cm


def same_as_lookup(pol, k, seqs, thresholds):
    """the scan == that independent device path aggregated in numpy, for every pair of thresholds -> the scans' totals"""
    counts = [lookup_counts(pol, k, s) for s in seqs]
    totals = []
    for min_count, mid_count in thresholds:
        r = pol.trio_strings(0, 1, seqs, min_count, mid_count, bits=True)
        for i, (valid, cp, cm) in enumerate(counts):
            e_stats, e_pb, e_mb = aggregate(valid, classes(valid, cp, cm, min_count, mid_count))
            assert stats_row(r, i) == e_stats, (k, min_count, mid_count, i, len(seqs[i]))
            assert np.array_equal(r.pat_bits[i], e_pb) and np.array_equal(r.mat_bits[i], e_mb), (k, min_count, mid_count, i)
        totals.append(r.total)
    return totals


def chimera(h1, h2, block):
    """h1 and h2 in alternating blocks"""
    n = min(len(h1), len(h2))
    return b"".join((h1 if (a // block) % 2 == 0 else h2)[a:a + block] for a in range(0, n, block))


# ---- 1. the known answer ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def diploid():
    s = Synth(60000, depth=30, seed=11, diploid=True, read_len_mean=9000.0, read_len_sd=1500.0)
    yaks = [parent_yak(s.hap1, K), parent_yak(s.hap2, K)]
    pol = Polisher(yaks)
    yield s, yaks, [yak_table(y) for y in yaks], pol
    pol.close()


def test_known_answer_on_a_diploid_contig(diploid):
    s, yaks, (tp, tm), pol = diploid
    h1, h2 = s.hap1, s.hap2
    a, b = 20000, 40000
    chim = h1[:a] + h2[a:b] + h1[b:]
    r = same_as_numpy(pol, K, tp, tm, [h1, h2, chim], 2, 5)
    nk, n_pat, n_mat, pp, pm, mp, mm = stats_row(r, 0)
    assert nk == len(h1) - K + 1 and n_pat > 100 and n_mat == 0 and (pp, pm, mp, mm) == (n_pat - 1, 0, 0, 0)
    nk, n_pat, n_mat, pp, pm, mp, mm = stats_row(r, 1)
    assert nk == len(h2) - K + 1 and n_mat > 100 and n_pat == 0 and (pp, pm, mp, mm) == (0, 0, 0, n_mat - 1)
    # the chimera: every segment holds a marker of its own parent and of no other (from the brute force, not assumed)
    valid, hashes = kmer_hashes_at(chim, K)
    from test_qv_cpu import table_counts
    cls = classes(valid, table_counts(tp, hashes, 1), table_counts(tm, hashes, 1), 2, 5)
    ends = np.arange(len(chim))
    seg = [cls[(ends >= lo) & (ends < hi)] for lo, hi in ((K - 1, a), (a + K - 1, b), (b + K - 1, len(chim)))]
    assert (seg[0] == 1).any() and (seg[1] == 2).any() and (seg[2] == 1).any()
    assert not (seg[0] == 2).any() and not (seg[1] == 1).any() and not (seg[2] == 2).any()
    nk, n_pat, n_mat, pp, pm, mp, mm = stats_row(r, 2)
    assert (pm, mp) == (1, 1) and pp + pm + mp + mm == n_pat + n_mat - 1 and n_pat > 100 and n_mat > 100
    assert trio.rate_text(pm + mp, pp + pm + mp + mm) == "%.6f" % (2 / (n_pat + n_mat - 1))
    sites = trio.switch_sites(r.pat_bits[2], r.mat_bits[2], len(chim), K)
    assert [x[2] for x in sites] == ["pm", "mp"] and abs(sites[0][1] - a) < 2000 and abs(sites[1][0] - b) < 2000
    assert r.kernel_ms > 0
    # the parents swapped: the mirror
    m = pol.trio_strings(1, 0, [chim], 2, 5)
    assert stats_row(m, 0) == (nk, n_mat, n_pat, mm, mp, pm, pp)


# ---- 2. device == numpy brute force == lookup_hashes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_setup():
    """two parents a SNP in a hundred apart, and a base sequence that changes parent every 700 bases"""
    rng = np.random.default_rng(17)
    p = random_bases(rng, 60000)
    m = noisy(rng, p, 0.01)
    ks = (16, 21, 31)
    yaks = [y for k in ks for y in (parent_yak(p, k), parent_yak(m, k))]  # tables 2 i (paternal), 2 i + 1 (maternal) of ks[i]
    pol = Polisher(yaks)
    yield rng, chimera(p, m, 700), ks, [yak_table(y) for y in yaks], pol
    pol.close()


def test_edge_sequences(edge_setup):
    rng, base, ks, tables, pol = edge_setup
    for i, k in enumerate(ks):
        seqs = edge_sequences(rng, base, k)
        for min_count, mid_count in ((2, 5), (1, 1), (5, 5), (16, 16)):
            r = same_as_numpy(pol, k, tables[2 * i], tables[2 * i + 1], seqs, min_count, mid_count, 2 * i, 2 * i + 1)
            if mid_count <= 5:
                tot = r.total
                assert tot[1] > 0 and tot[2] > 0 and tot[4] > 0 and tot[5] > 0
            else:
                assert r.total[1:] == (0,) * 6  # no count reaches 16: a k-mer is counted 5 times, 10 where a parent holds it twice
        assert [int(x) for x in r.stats[:6, 0]] == [0, 0, 1, 2, 0, 0]
        assert pol.trio_strings(2 * i, 2 * i + 1, []).stats.shape == (0, 7)
        assert pol.trio_strings(2 * i, 2 * i + 1, [b"", b""], bits=True).total == (0,) * 7


def test_edge_sequences_equal_lookup_hashes(edge_setup):
    rng, base, ks, tables, pol = edge_setup
    sub = Polisher([pol._yaks[2], pol._yaks[3]])  # k 21
    same_as_lookup(sub, 21, edge_sequences(rng, base, 21), [(2, 5), (1, 1)])
    sub.close()


def test_5000_short_sequences_in_one_call(edge_setup):
    rng, base, ks, tables, pol = edge_setup
    seqs = []
    for _ in range(5000):
        n = int(rng.integers(0, 201))
        a = int(rng.integers(0, len(base) - n))
        seqs.append(noisy(rng, base[a:a + n], 0.02))
    for i, k in ((0, 16), (2, 31)):
        r = same_as_numpy(pol, k, tables[2 * i], tables[2 * i + 1], seqs, 2, 5, 2 * i, 2 * i + 1)
        assert r.total[1] > 0 and r.total[2] > 0


def test_repeated_keys_answer_like_lookup_hashes():
    """Hand-made dumps with repeated keys in their buckets (yak writes none): the last word in file order is the k-mer's
    count, as the polish kernels' lookup has it at threshold 1.  One table repeats keys, then both."""
    rng = np.random.default_rng(29)
    p = random_bases(rng, 20000)
    m = noisy(rng, p, 0.01)

    def with_repeats(seq, first, last):
        words, off = numpy_count((seq + b"\n") * 5, K)
        out_words, out_off = [], [0]
        for b in range(1024):
            w = words[int(off[b]):int(off[b + 1])]
            keys = w[::3] & ~np.uint64(1023)  # every third word again, with other counts, before and after the original
            w = np.concatenate([keys | np.uint64(first), w, keys | np.uint64(last)])
            out_words.append(w)
            out_off.append(out_off[-1] + len(w))
        return Yak(K, np.concatenate(out_words), np.array(out_off, np.uint64))

    seqs = [chimera(p, m, 900)[:9000], chimera(m, p, 1100)[9000:], p[100:130], noisy(rng, p[:TILE + 50])]
    seen = set()
    for yaks in ([with_repeats(p, 9, 1), parent_yak(m, K)], [parent_yak(p, K), with_repeats(m, 1, 7)],
                 [with_repeats(p, 7, 3), with_repeats(m, 2, 1)]):
        pol = Polisher(yaks)
        seen.update(same_as_lookup(pol, K, seqs, [(2, 5), (1, 1), (4, 7), (2, 3)]))
        pol.close()
    assert len(seen) >= 4  # (the repeats change the answers: a third of the keys read 1, 3 or 7 instead of 5)


def crowded_parents(k):
    """test_gpu_qv.crowded's seven k-mers per bucket split between a paternal table (3: counts 3, 5, 7) and a maternal one
    (4: counts 2, 4, 6, 8), the other way round in bucket 0: both tables get 16-slot sub-tables, and every chain starts in
    slot 14 or 15 and wraps"""
    seq, hashes, counts = crowded(k)
    pat = np.zeros(hashes.shape, bool)
    pat[:, 1::2] = True
    pat[0] = ~pat[0]
    yaks = [Yak(k, *dump_of(hashes[sel], counts[sel])) for sel in (pat, ~pat)]
    assert [int(np.diff(y.bucket_off.astype(np.int64)).max()) for y in yaks] == [4, 4]
    return seq, yaks


@pytest.mark.parametrize("k", [21, 31])
def test_probe_chains_wrap_inside_crowded_subtables(monkeypatch, k):
    seq, yaks = crowded_parents(k)
    pol = Polisher(yaks)
    tp, tm = yak_table(yaks[0]), yak_table(yaks[1])
    for stage_tiles in (None, 1):
        if stage_tiles is not None:
            monkeypatch.setenv("NP2_TRIO_TEST_STAGE_TILES", str(stage_tiles))
        r = same_as_numpy(pol, k, tp, tm, [seq], 2, 5)
        assert r.total[1] > 1024 and r.total[2] > 1024 and r.total[4] > 100 and r.total[5] > 100
        same_as_lookup(pol, k, [seq], [(2, 5), (1, 1), (3, 8)])
    pol.close()


def test_12mb_diploid_assembly_in_contigs():
    s = Synth(12_000_000, depth=1, seed=5, diploid=True)
    asm = chimera(s.hap1, s.hap2, 1_000_000)
    cuts = [0] + sorted(int(x) for x in np.random.default_rng(5).integers(1, len(asm), size=5)) + [len(asm)]
    contigs = [asm[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    yaks = [scaled_yak(s.hap1, K), scaled_yak(s.hap2, K)]
    tp, tm = yak_table(yaks[0]), yak_table(yaks[1])
    pol = Polisher(yaks)
    r = same_as_numpy(pol, K, tp, tm, contigs, 2, 5)
    nk, n_pat, n_mat, pp, pm, mp, mm = r.total
    assert n_pat > 10000 and n_mat > 10000 and 11 <= pm + mp <= 40  # (eleven block edges of the chimera)
    same_as_lookup(pol, K, contigs, [(2, 5), (1, 5), (5, 5), (6, 1023)])
    pol.close()


# ---- 3. order survives every boundary ---------------------------------------------------------------------------------------------
def planted(rng, length, markers, k):
    """a random sequence and the two tables that make exactly the k-mers ending at `markers` = {end: class} markers"""
    seq = random_bases(rng, length)
    valid, h = kmer_hashes_at(seq, k)
    assert valid[k - 1:].all() and len(np.unique(h[k - 1:])) == length - k + 1
    pat = [e for e, c in markers.items() if c == 1]
    mat = [e for e, c in markers.items() if c == 2]
    return seq, table_of(h[pat], [5] * len(pat)), table_of(h[mat], [9] * len(mat))


@pytest.fixture(scope="module")
def boundary_setup():
    rng = np.random.default_rng(41)
    L = 12 * TILE + 777
    # single markers at the last base of a tile and the first of the next, marker-free stretches of several tiles between
    # them, either side of the piece edges of 1- and 3-tile staging buffers (every tile edge / tiles 3, 6, 9, 12)
    markers = {K - 1: 1, TILE - 1: 2, TILE: 1, 5 * TILE - 1: 1, 6 * TILE - 1: 2, 6 * TILE: 2, 6 * TILE + 1: 1, 9 * TILE - 1: 1,
               9 * TILE: 2, 11 * TILE + 100: 1, 12 * TILE - 1: 2, 12 * TILE + 31: 1, 12 * TILE + 32: 2, L - 1: 1}
    seq, pat, mat = planted(rng, L, markers, K)
    # further sequences of the same call: one without any marker over several tiles, one whose only markers are its first
    # and last k-mer, short ones
    valid, h = kmer_hashes_at(seq, K)
    seqs = [seq, seq[TILE + 1:5 * TILE - 1], b"", seq[TILE - K + 1:6 * TILE], seq[:K], seq[9 * TILE - K + 1:9 * TILE + 1], seq[3:2 * TILE + 5]]
    yaks = [Yak(K, *pat), Yak(K, *mat)]
    pol = Polisher(yaks)
    yield seqs, markers, [yak_table(y) for y in yaks], pol
    pol.close()


def test_planted_markers_known_answer(boundary_setup):
    seqs, markers, (tp, tm), pol = boundary_setup
    e_stats, e_pb, e_mb = numpy_trio(seqs[0], K, tp, tm, 2, 5)
    order = [markers[e] for e in sorted(markers)]
    pairs = list(zip(order[:-1], order[1:]))
    assert e_stats == (len(seqs[0]) - K + 1, order.count(1), order.count(2), pairs.count((1, 1)), pairs.count((1, 2)),
                       pairs.count((2, 1)), pairs.count((2, 2)))
    assert sorted(np.flatnonzero(np.unpackbits(e_pb, bitorder="little")).tolist() +
                  np.flatnonzero(np.unpackbits(e_mb, bitorder="little")).tolist()) == sorted(markers)
    assert numpy_trio(seqs[1], K, tp, tm, 2, 5)[0][1:] == (0,) * 6
    assert numpy_trio(seqs[3], K, tp, tm, 2, 5)[0][1:] == (2, 1, 1, 1, 0, 0)  # TILE: P, 5 TILE - 1: P, 6 TILE - 1: M
    r = same_as_numpy(pol, K, tp, tm, seqs, 2, 5)
    assert stats_row(r, 0) == e_stats


@pytest.mark.parametrize("stage_tiles", [None, 1, 3])
@pytest.mark.parametrize("blocks", [None, 1, 3])
def test_order_survives_pieces_and_grids(boundary_setup, monkeypatch, stage_tiles, blocks):
    """NP2_TRIO_TEST_STAGE_TILES: a staging buffer of a few tiles, so that sequences go on from piece to piece;
    NP2_TRIO_TEST_BLOCKS: the grid, so that one block scans every tile in turn or three share them"""
    seqs, markers, (tp, tm), pol = boundary_setup
    if stage_tiles is not None:
        monkeypatch.setenv("NP2_TRIO_TEST_STAGE_TILES", str(stage_tiles))
    if blocks is not None:
        monkeypatch.setenv("NP2_TRIO_TEST_BLOCKS", str(blocks))
    for order in (seqs, seqs[::-1]):
        same_as_numpy(pol, K, tp, tm, order, 2, 5)
    m = pol.trio_strings(1, 0, seqs, 2, 5)  # the parents swapped: the mirror
    r = pol.trio_strings(0, 1, seqs, 2, 5)
    assert np.array_equal(m.stats[:, [0, 2, 1, 6, 5, 4, 3]], r.stats)


@pytest.mark.parametrize("stage_tiles", [1, 3])
def test_edge_sequences_in_small_pieces(edge_setup, monkeypatch, stage_tiles):
    rng, base, ks, tables, pol = edge_setup
    monkeypatch.setenv("NP2_TRIO_TEST_STAGE_TILES", str(stage_tiles))
    a = int(rng.integers(0, 1000))
    seqs = edge_sequences(rng, base, 21) + [noisy(rng, base[a:a + 5 * TILE + 77]), b"", noisy(rng, base[:4 * TILE])]
    for blocks in ("1", "2", "1000"):
        monkeypatch.setenv("NP2_TRIO_TEST_BLOCKS", blocks)
        r = same_as_numpy(pol, 21, tables[2], tables[3], seqs, 2, 5, 2, 3)
        assert r.n_switch > 10


# ---- 4. no pair spans two sequences -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage_tiles", [None, 1])
def test_no_pair_spans_two_sequences(diploid, monkeypatch, stage_tiles):
    s, yaks, (tp, tm), pol = diploid
    if stage_tiles is not None:
        monkeypatch.setenv("NP2_TRIO_TEST_STAGE_TILES", str(stage_tiles))
    lens = [TILE, 2 * TILE, 400, TILE - HALO, 300, 1000, TILE, 310, 3000, TILE + 1, 2 * TILE, 640]
    seqs, at = [], 0
    for i, n in enumerate(lens):  # pure pieces of one haplotype each, alternating
        seqs.append((s.hap1 if i % 2 == 0 else s.hap2)[at:at + n])
        at += n
    for order in (seqs, seqs[::-1]):
        r = same_as_numpy(pol, K, tp, tm, order, 2, 5)
        tot = r.total
        assert tot[4] + tot[5] == 0 and tot[1] > 0 and tot[2] > 0
        assert tot[3] + tot[6] == sum(max(0, int(x[1]) + int(x[2]) - 1) for x in r.stats)
        for i, row in enumerate(r.stats):  # a sequence holds markers of one parent only
            assert int(row[1]) == 0 or int(row[2]) == 0


# ---- 5. host path == device path ----------------------------------------------------------------------------------------------------
def test_device_path_equals_host_path_after_a_polish(diploid):
    s, pyaks, (tp, tm), tpol = diploid  # (tpol: the context of the parental tables, on the same device)
    pol = Polisher([s.yak(21), s.yak(31)])
    c = pol.upload(s.pileup)
    bases, _ = pol.polish_resident(c, Opts())
    ptr, n = pol.last_result_device()
    seq = bases.tobytes()
    assert n == len(seq)
    for skip, drop in ((0, 0), (1, 0), (3, 5), (17, 1), (HALO + 1, TILE + 3), (TILE - 1, 2 * TILE)):  # any alignment, any end
        sub = seq[skip:len(seq) - drop]
        d = tpol.trio_device(0, 1, ptr + skip, len(sub), 2, 5, bits=True)
        h = tpol.trio_strings(0, 1, [sub], 2, 5, bits=True)
        assert np.array_equal(d.stats, h.stats) and np.array_equal(d.pat_bits[0], h.pat_bits[0]) and np.array_equal(d.mat_bits[0], h.mat_bits[0])
        e_stats, e_pb, e_mb = numpy_trio(sub, K, tp, tm, 2, 5)
        assert stats_row(d, 0) == e_stats and np.array_equal(d.pat_bits[0], e_pb) and np.array_equal(d.mat_bits[0], e_mb)
        assert np.array_equal(tpol.trio_device(0, 1, ptr + skip, len(sub), 2, 5).stats, d.stats)
        # the parents swapped: the mirror (the polished sequence follows hap1, so only this call sees maternal markers)
        m = tpol.trio_device(1, 0, ptr + skip, len(sub), 2, 5, bits=True)
        assert np.array_equal(m.stats[:, [0, 2, 1, 6, 5, 4, 3]], d.stats)
        assert np.array_equal(m.pat_bits[0], d.mat_bits[0]) and np.array_equal(m.mat_bits[0], d.pat_bits[0])
    assert d.total[1] > 1000 and m.total[2] > 1000 and d.kernel_ms > 0
    assert tpol.trio_device(0, 1, ptr, 0).total == (0,) * 7 and tpol.trio_device(0, 1, ptr + 5, K - 1).total[0] == 0
    assert tpol.trio_device(0, 1, ptr + 5, K).total[0] == 1
    c.free()
    pol.close()


# ---- 6. both command lines end to end -------------------------------------------------------------------------------------------------
def parse_tsv(path):
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def expected_rows(named, k, tp, tm, min_count, mid_count):
    """rows of the module's TSV for [(name, sequence)] + the totals, from the brute force"""
    rows = [(name, k, len(seq)) + numpy_trio(seq, k, tp, tm, min_count, mid_count)[0] for name, seq in named]
    rows.append(("total", k) + tuple(int(x) for x in np.array([r[2:] for r in rows], np.int64).sum(axis=0)))
    return [ln.rstrip("\n").split("\t") for ln in trio.format_rows(rows)]


def write_fasta(path, named):
    with open(path, "wb") as f:
        for name, seq in named:
            f.write(b">" + name.encode() + b"\n" + b"".join(seq[i:i + 80] + b"\n" for i in range(0, len(seq), 80)))


def test_trio_module_on_dumps_and_on_reads(diploid, tmp_path):
    s, yaks, (tp, tm), pol = diploid
    named = [("chim", chimera(s.hap1, s.hap2, 7000)), ("h1", s.hap1[:30000]), ("none", b"ACGTNNNN" * 10), ("h2", s.hap2[5000:9000])]
    fa = str(tmp_path / "asm.fa")
    write_fasta(fa, named)
    dumps = []
    for name, y in zip(("pat", "mat"), yaks):
        dumps.append(str(tmp_path / f"{name}.yak"))
        np2io.write_yak(dumps[-1], y)
    tsv, bed = str(tmp_path / "t.tsv"), str(tmp_path / "t.bed")
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.trio", fa] + dumps + ["-o", tsv, "--bed", bed], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    head, rows = parse_tsv(tsv)
    assert head == list(trio.TSV_HEADER)
    exp = expected_rows(named, K, tp, tm, 2, 5)
    assert rows == exp
    assert int(exp[0][10]) >= 7 and exp[1][10:] == ["0", "0.000000", "0", "0.000000"] and exp[2][10:] == ["0", "nan", "0", "nan"]
    e_bed = ""
    for name, seq in named:
        _, pb, mb = numpy_trio(seq, K, tp, tm, 2, 5)
        e_bed += "".join(f"{name}\t{a}\t{b}\t{kind}\n" for a, b, kind in trio.switch_sites(pb, mb, len(seq), K))
    assert open(bed).read() == e_bed and e_bed.count("\n") == int(exp[-1][10])
    # other thresholds, on standard output
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.trio", fa] + dumps + ["--min_count", "1", "--mid_count", "3"],
                       capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert [ln.split("\t") for ln in r.stdout.decode().splitlines()[1:]] == expected_rows(named, K, tp, tm, 1, 3)
    # the parents' reads counted on the device: every haplotype five times over, one read a line, in two files each
    reads = {}
    for name, hap in (("pat", s.hap1), ("mat", s.hap2)):
        reads[name] = [str(tmp_path / f"{name}.{i}.txt") for i in range(2)]
        open(reads[name][0], "wb").write((hap + b"\n") * 2)
        open(reads[name][1], "wb").write((hap + b"\n") * 3)
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.trio", fa, "--pat_sr"] + reads["pat"] + ["--mat_sr", reads["mat"][0], "--mat_sr", reads["mat"][1],
                        "--sr_k", str(K), "--sr_min_count", "2"], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert [ln.split("\t") for ln in r.stdout.decode().splitlines()[1:]] == exp


def test_cli_trio_on_a_synthetic_diploid_bam(diploid, tmp_path):
    from nextpolish2_amd.bamio import pileup_to_records, write_bam
    s, yaks, (tp, tm), pol = diploid
    recs = pileup_to_records(s.pileup, tid=0, rng=np.random.default_rng(3), decorate=True)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    write_bam(str(tmp_path / "m.bam"), [("ctg", s.pileup.L)], recs)
    ref = s.pileup.ref.tobytes()
    tiny = s.hap1[:3000] + s.hap2[3000:6000]  # a pass-through contig with a switch in it
    write_fasta(str(tmp_path / "g.fa"), [("ctg", ref), ("tiny", tiny)])
    np2io.write_yak(str(tmp_path / "k21.yak"), s.yak(21))
    dumps = []
    for name, y in zip(("pat", "mat"), yaks):
        dumps.append(str(tmp_path / f"{name}.yak"))
        np2io.write_yak(dumps[-1], y)
    cmd = [sys.executable, "-m", "nextpolish2_amd.cli", "-t", "2", "-L", "10000", str(tmp_path / "m.bam"), str(tmp_path / "g.fa"), str(tmp_path / "k21.yak")]
    plain = subprocess.run(cmd, capture_output=True, env=ENV, timeout=600)
    assert plain.returncode == 0, plain.stderr.decode()
    tsv, prefix = str(tmp_path / "t.tsv"), str(tmp_path / "sw")
    r = subprocess.run(cmd + ["--trio", tsv, "--trio_pat", dumps[0], "--trio_mat", dumps[1], "--trio_bed", prefix], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == plain.stdout and r.stdout.count(b">") == 2  # byte for byte the FASTA written without --trio
    lines = r.stdout.split(b"\n")
    written = {lines[i][1:].split()[0].decode(): lines[i + 1] for i in range(0, len(lines) - 1, 2)}
    assert written["tiny"] == tiny and written["ctg"] != ref
    head, rows = parse_tsv(tsv)
    assert head == list(trio.CLI_HEADER)
    exp_rows = []
    for name, seq in (("ctg", ref), ("tiny", tiny)):
        exp_rows.append((name, K, len(seq)) + numpy_trio(seq, K, tp, tm, 2, 5)[0] + (len(written[name]),) + numpy_trio(written[name], K, tp, tm, 2, 5)[0])
    exp_rows.append(("total", K) + tuple(int(x) for x in np.array([r_[2:] for r_ in exp_rows], np.int64).sum(axis=0)))
    assert rows == [ln.rstrip("\n").split("\t") for ln in trio.format_rows(exp_rows)]
    assert int(rows[1][7]) + int(rows[1][8]) == 1  # tiny as read: one switch
    for side, seqs in (("in", {"ctg": ref, "tiny": tiny}), ("out", written)):
        e_bed = ""
        for name in ("ctg", "tiny"):
            _, pb, mb = numpy_trio(seqs[name], K, tp, tm, 2, 5)
            e_bed += "".join(f"{name}\t{a}\t{b}\t{kind}\n" for a, b, kind in trio.switch_sites(pb, mb, len(seqs[name]), K))
        assert open(f"{prefix}.{side}.bed").read() == e_bed
    # with --qv next to it: both reports, the same FASTA
    qv_tsv = str(tmp_path / "q.tsv")
    r2 = subprocess.run(cmd + ["--trio", str(tmp_path / "t2.tsv"), "--trio_pat", dumps[0], "--trio_mat", dumps[1], "--qv", qv_tsv],
                        capture_output=True, env=ENV, timeout=600)
    assert r2.returncode == 0, r2.stderr.decode()
    assert r2.stdout == plain.stdout and open(str(tmp_path / "t2.tsv")).read() == open(tsv).read() and os.path.getsize(qv_tsv) > 0


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(edge_setup):
    rng, base, ks, tables, pol = edge_setup
    L = api.lib()
    n_tables = 2 * len(ks)
    seq = np.frombuffer(base[:100] + b"\0", dtype=np.uint8)
    off = np.array([0, 60, 100], np.uint64)
    bad_off = np.array([0, 60, 50], np.uint64)
    out = np.zeros((2, 7), np.uint64)
    good = pol.trio_strings(2, 3, [base[:3000], b""], 2, 5)

    def strings(p, m, strs, o, n, outp, lo=2, hi=5):
        return L.np2_trio_strings(pol._h, p, m, strs, o, n, lo, hi, outp, None, None, None)

    def device(p, m, ptr, n, outp, lo=2, hi=5):
        return L.np2_trio_device(pol._h, p, m, ptr, n, lo, hi, outp, None, None, None)

    sd, od, ud = seq.ctypes.data, off.ctypes.data, out.ctypes.data
    cases = [
        (lambda: strings(n_tables, 1, sd, od, 2, ud), "pat_idx"),
        (lambda: strings(-1, 1, sd, od, 2, ud), "pat_idx"),
        (lambda: strings(0, n_tables, sd, od, 2, ud), "mat_idx"),
        (lambda: strings(0, -1, sd, od, 2, ud), "mat_idx"),
        (lambda: strings(1, 1, sd, od, 2, ud), "pat_idx == mat_idx"),
        (lambda: strings(0, 3, sd, od, 2, ud), "different k"),
        (lambda: strings(0, 1, sd, od, 2, ud, 0, 5), "thresholds"),
        (lambda: strings(0, 1, sd, od, 2, ud, 6, 5), "thresholds"),
        (lambda: strings(0, 1, sd, od, 2, ud, 2, 1024), "thresholds"),
        (lambda: strings(0, 1, sd, bad_off.ctypes.data, 2, ud), "descending"),
        (lambda: strings(0, 1, sd, od, 2, None), "out is NULL"),
        (lambda: strings(0, 1, None, od, 2, ud), "strs is NULL"),
        (lambda: strings(0, 1, sd, None, 2, ud), "off is NULL"),
        (lambda: device(n_tables, 0, None, 0, ud), "pat_idx"),
        (lambda: device(0, 0, None, 0, ud), "pat_idx == mat_idx"),
        (lambda: device(0, 2, None, 0, ud), "different k"),
        (lambda: device(0, 1, None, 0, ud, 5, 4), "thresholds"),
        (lambda: device(0, 1, None, 10, ud), "dev_seq is NULL"),
        (lambda: device(0, 1, None, 0, None), "out is NULL"),
    ]
    for call, text in cases:
        assert call() == E_ARG
        assert text in L.np2_last_error(pol._h).decode(), text
        # the context still answers
        r = pol.trio_strings(2, 3, [base[:3000], b""], 2, 5)
        assert np.array_equal(r.stats, good.stats) and int(r.stats[0, 0]) == 3000 - 21 + 1
    for bad in ((9, 0, 2, 5), (0, 0, 2, 5), (0, 1, 0, 5), (0, 1, 3, 2)):
        with pytest.raises(api.Np2Error) as e:
            pol.trio_strings(bad[0], bad[1], [b"ACGT"], bad[2], bad[3])
        assert e.value.code == E_ARG
    assert L.np2_trio_strings(None, 0, 1, None, None, 0, 2, 5, None, None, None, None) == E_ARG
    assert strings(0, 1, None, None, 0, ud) == 0  # n == 0 is fine
    assert device(0, 1, None, 0, ud) == 0  # and so is an empty sequence
