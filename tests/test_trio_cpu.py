"""The trio measurement's host side, without a GPU: the scan's per-lane core as a one-lane host program
(csrc/np2_trio_core.hpp through tests/tools/trio_core_test.cpp, which looks hashes up by binary search in two dumps), the
host helpers of nextpolish2_amd.trio, and the argument checks of both command lines.

The independent expectation is the numpy brute force below (numpy_trio): kmer_hashes_at + table_counts of test_qv_cpu.py,
the classification written out again, then np.diff over the marker sequence."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from nextpolish2_amd import trio
from test_kcount_cpu import awkward_stream, dump_bytes, numpy_count, stream_hashes
from test_qv_cpu import ASM_IN, BAM, BUNDLE, kmer_hashes_at, table_counts

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the numpy brute force ---------------------------------------------------------------------------------------------
def classes(valid, c_pat, c_mat, min_count, mid_count):
    """per base: 0 no marker, 1 paternal, 2 maternal"""
    c_pat, c_mat = c_pat.astype(np.int64), c_mat.astype(np.int64)
    pat = valid & (c_pat >= mid_count) & (c_mat < min_count)
    mat = valid & (c_mat >= mid_count) & (c_pat < min_count)
    assert not (pat & mat).any()
    return pat.astype(np.int8) + 2 * mat.astype(np.int8)


def aggregate(valid, cls):
    """((n_kmers, n_pat, n_mat, pp, pm, mp, mm), paternal bitmap, maternal bitmap) of one sequence"""
    m = cls[cls != 0].astype(np.int64)  # the markers in ascending end position
    d = np.diff(m)
    pp, mm = int(((d == 0) & (m[:-1] == 1)).sum()), int(((d == 0) & (m[:-1] == 2)).sum())
    pm, mp = int((d == 1).sum()), int((d == -1).sum())
    assert pp + pm + mp + mm == max(0, len(m) - 1)
    return ((int(valid.sum()), int((cls == 1).sum()), int((cls == 2).sum()), pp, pm, mp, mm),
            np.packbits(cls == 1, bitorder="little"), np.packbits(cls == 2, bitorder="little"))


def numpy_trio(seq, k, pat_table, mat_table, min_count, mid_count):
    valid, hashes = kmer_hashes_at(seq, k)
    return aggregate(valid, classes(valid, table_counts(pat_table, hashes, 1), table_counts(mat_table, hashes, 1), min_count, mid_count))


def table_of(hashes, counts):
    """(words, bucket_off) of a dump holding `hashes` (distinct) with `counts` (1 .. 1023)"""
    h, c = np.asarray(hashes, np.uint64), np.asarray(counts, np.uint64)
    order = np.lexsort((h, h & np.uint64(1023)))
    h, c = h[order], c[order]
    off = np.zeros(1025, np.uint64)
    off[1:] = np.cumsum(np.bincount((h & np.uint64(1023)).astype(np.int64), minlength=1024))
    return ((h >> np.uint64(10)) << np.uint64(10)) | c, off


def sorted_table(words, off):
    b = np.repeat(np.arange(1024, dtype=np.uint64), np.diff(off.astype(np.int64)))
    h = ((words >> np.uint64(10)) << np.uint64(10)) | b
    order = np.argsort(h)
    return h[order], (words & np.uint64(1023)).astype(np.uint32)[order]


def random_bases(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()


# ---- 1. the per-lane core ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trio") / "trio_core_test")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "tools", "trio_core_test.cpp"), "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_core(exe, min_count, mid_count, pat, mat, seqfile, stretch=0):
    r = subprocess.run([exe, str(min_count), str(mid_count), pat, mat, seqfile, str(stretch)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    stats, pat_bits, mat_bits = [], [], []
    for ln in r.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "seq":
            stats.append(tuple(int(x) for x in f[1:]))
        else:
            (pat_bits if f[0] == "pat" else mat_bits).append(np.frombuffer(bytes.fromhex(f[1]) if len(f) > 1 else b"", dtype=np.uint8))
    return stats, pat_bits, mat_bits


def write_tables(tmp_path, k, pat, mat, tag=""):
    paths = []
    for name, (words, off) in (("pat", pat), ("mat", mat)):
        p = tmp_path / f"{name}{tag}.k{k}.yak"
        p.write_bytes(dump_bytes(k, words, off))
        paths.append(str(p))
    return paths


def check_core(exe, tmp_path, k, pat, mat, seqs, thresholds, stretches=(0, 1, 7, 64), tag=""):
    """the core's answers for `seqs` (one per line: no sequence holds a newline) == numpy_trio, whatever the stretch"""
    src = tmp_path / f"seqs{tag}.k{k}.txt"
    src.write_bytes(b"".join(s + b"\n" for s in seqs))
    pp, mp = write_tables(tmp_path, k, pat, mat, tag)
    tp, tm = sorted_table(*pat), sorted_table(*mat)
    seen = np.zeros(7, np.int64)
    for min_count, mid_count in thresholds:
        exp = [numpy_trio(s, k, tp, tm, min_count, mid_count) for s in seqs]
        for stretch in stretches:
            stats, pb, mb = run_core(exe, min_count, mid_count, pp, mp, str(src), stretch)
            assert len(stats) == len(pb) == len(mb) == len(seqs)
            for i, (e_stats, e_pb, e_mb) in enumerate(exp):
                assert stats[i] == e_stats, (k, min_count, mid_count, stretch, i, seqs[i][:60])
                assert np.array_equal(pb[i], e_pb) and np.array_equal(mb[i], e_mb), (k, min_count, mid_count, stretch, i)
        seen += np.array([e[0] for e in exp], np.int64).sum(axis=0)
    return seen


def test_core_on_awkward_sequences(core_exe, tmp_path):
    """One sequence per line: lower case, U, N, bytes >= 0x80, lengths around k, an empty line.  The paternal table counts
    every read once and the even reads four times more, the maternal table the odd reads: k-mers of one half only are
    markers at (2, 5), none is at (1, 1) where one count of the other parent is enough to disqualify.  Reads joined in
    threes switch parents inside a sequence."""
    stream = awkward_stream()
    seqs = stream.split(b"\n")[:-1]
    even = b"".join(s + b"\n" for s in seqs[0::2])
    odd = b"".join(s + b"\n" for s in seqs[1::2])
    for k in (2, 11, 16, 31):
        pat, mat = numpy_count(stream + even * 4, k), numpy_count(stream + odd * 4, k)
        joined = [b"".join(seqs[i:i + 3]) for i in range(0, len(seqs) - 2, 3)]
        seen = check_core(core_exe, tmp_path, k, pat, mat, seqs + joined, [(2, 5), (1, 1), (5, 5), (2, 1023), (1023, 1023)], stretches=(0, 1, 5, 32))
        if k >= 11:
            assert seen[1] > 0 and seen[2] > 0 and seen[3:].min() > 0  # both kinds of marker, all four kinds of pair


def test_core_on_lengths_around_k(core_exe, tmp_path):
    rng = np.random.default_rng(3)
    for k in (2, 21, 31):
        base = random_bases(rng, 400)
        # every k-mer of `base` is paternal, every k-mer of its reverse (not the complement: other k-mers) maternal
        pat, mat = numpy_count((base + b"\n") * 5, k), numpy_count((base[::-1] + b"\n") * 5, k)
        seqs = [b"", base[:k - 1], base[:k], base[:k + 1], base[::-1][:k - 1], base[::-1][:k], base[::-1][:k + 1],
                base[:k] + b"N" + base[::-1][:k], base[:k - 1] + b"N" + base[k - 1:2 * k]]
        check_core(core_exe, tmp_path, k, pat, mat, seqs, [(2, 5), (1, 5)])
        if k > 2:
            tp, tm = sorted_table(*pat), sorted_table(*mat)
            got = [numpy_trio(s, k, tp, tm, 2, 5)[0] for s in seqs]
            assert [g[:3] for g in got[:7]] == [(0, 0, 0), (0, 0, 0), (1, 1, 0), (2, 2, 0), (0, 0, 0), (1, 0, 1), (2, 0, 2)]
            assert got[7] == (2, 1, 1, 0, 1, 0, 0)  # a non-base breaks k-mers, not adjacency: one pm pair across the N


def test_core_markers_only_at_the_first_and_last_kmer(core_exe, tmp_path):
    rng = np.random.default_rng(4)
    for k in (16, 31):
        for n in (k + 1, 100, 777):
            s = random_bases(rng, n)
            valid, h = kmer_hashes_at(s, k)
            first, last = h[k - 1], h[n - 1]
            assert first != last and (h[valid] == first).sum() == 1 and (h[valid] == last).sum() == 1
            for tag, (pat, mat, exp) in enumerate([
                    (table_of([first], [5]), table_of([last], [5]), (n - k + 1, 1, 1, 0, 1, 0, 0)),
                    (table_of([last], [5]), table_of([first], [5]), (n - k + 1, 1, 1, 0, 0, 1, 0)),
                    (table_of([first, last], [5, 9]), table_of([], []), (n - k + 1, 2, 0, 1, 0, 0, 0)),
                    (table_of([], []), table_of([first, last], [5, 9]), (n - k + 1, 0, 2, 0, 0, 0, 1))]):
                assert numpy_trio(s, k, sorted_table(*pat), sorted_table(*mat), 2, 5)[0] == exp
                check_core(core_exe, tmp_path, k, pat, mat, [s], [(2, 5)], stretches=(0, 1, 3, n - 1, n), tag=f".{n}.{tag}")


def test_core_thresholds_at_their_edges(core_exe, tmp_path):
    """every pair of counts from {absent, min_count - 1, min_count, mid_count - 1, mid_count, 1023} in the two tables"""
    rng = np.random.default_rng(6)
    k = 21
    s = random_bases(rng, 4000)
    distinct = np.unique(stream_hashes(s + b"\n", k))
    for min_count, mid_count in ((2, 5), (3, 4), (4, 4), (1, 2), (1, 1), (1022, 1023)):
        edge = sorted({0, min_count - 1, min_count, mid_count - 1, mid_count, 1023})
        cp = rng.choice(edge, size=len(distinct))
        cm = rng.choice(edge, size=len(distinct))
        pat, mat = table_of(distinct[cp > 0], cp[cp > 0]), table_of(distinct[cm > 0], cm[cm > 0])
        seen = check_core(core_exe, tmp_path, k, pat, mat, [s, s[:1000].lower()], [(min_count, mid_count)], stretches=(0, 32),
                          tag=f".{min_count}.{mid_count}")
        assert seen[1] > 0 and seen[2] > 0
        # the rule, count by count
        for a in edge:
            for b in edge:
                c = classes(np.array([True]), np.array([a]), np.array([b]), min_count, mid_count)[0]
                assert c == (1 if a >= mid_count and b < min_count else 2 if b >= mid_count and a < min_count else 0)


def test_core_refuses_thresholds_outside_the_rule(core_exe, tmp_path):
    pat, mat = write_tables(tmp_path, 5, table_of([], []), table_of([], []))
    src = tmp_path / "s.txt"
    src.write_bytes(b"ACGTACGT\n")
    for min_count, mid_count in ((0, 5), (6, 5), (2, 1024)):
        r = subprocess.run([core_exe, str(min_count), str(mid_count), pat, mat, str(src)], capture_output=True, timeout=600)
        assert r.returncode == 6
        assert not trio.thresholds_ok(min_count, mid_count)
    assert trio.thresholds_ok(1, 1) and trio.thresholds_ok(2, 5) and trio.thresholds_ok(1023, 1023)


# ---- 2. host helpers -------------------------------------------------------------------------------------------------------
def test_rates():
    assert trio.rate_text(0, 0) == "nan" and math.isnan(trio.rate(0, 0))
    assert trio.rate_text(0, 7) == "0.000000" and trio.rate_text(7, 7) == "1.000000"
    assert trio.rate_text(1, 3) == "0.333333" and trio.rate_text(2, 3) == "0.666667"
    assert trio.rate_text(1, 10 ** 7) == "0.000000" and trio.rate_text(6, 10 ** 7) == "0.000001"
    st = (100, 7, 3, 4, 2, 1, 2)  # kmers, pat, mat, pp, pm, mp, mm
    assert trio.switch_of(st) == (3, 9) and trio.hamming_of(st) == (3, 10)
    assert trio.switch_of((5, 1, 0, 0, 0, 0, 0)) == (0, 0) and trio.hamming_of((5, 0, 0, 0, 0, 0, 0)) == (0, 0)


def bitmap(length, ends):
    b = np.zeros(length, bool)
    b[list(ends)] = True
    return np.packbits(b, bitorder="little")


def test_switch_sites_from_hand_made_bitmaps():
    k = 5
    none = bitmap(40, [])
    assert trio.switch_sites(none, none, 40, k) == []
    assert trio.switch_sites(np.zeros(0, np.uint8), np.zeros(0, np.uint8), 0, k) == []
    assert trio.switch_sites(bitmap(40, [4, 10, 39]), none, 40, k) == []                       # one parent only
    assert trio.switch_sites(bitmap(40, [4]), bitmap(40, [39]), 40, k) == [(0, 40, "pm")]      # first and last k-mer
    assert trio.switch_sites(bitmap(40, [39]), bitmap(40, [4]), 40, k) == [(0, 40, "mp")]
    assert trio.switch_sites(bitmap(40, [10, 11]), bitmap(40, [12, 13]), 40, k) == [(7, 13, "pm")]  # adjacent ends
    assert trio.switch_sites(bitmap(40, [5, 20, 30]), bitmap(40, [9, 10, 25]), 40, k) == [
        (1, 10, "pm"), (6, 21, "mp"), (16, 26, "pm"), (21, 31, "mp")]
    assert trio.switch_sites(bitmap(37, [36]), bitmap(37, [8]), 37, k) == [(4, 37, "mp")]      # a length that is no multiple of 8
    assert trio.switch_sites(bitmap(40, [4, 39]), bitmap(40, [20]), 39, k) == [(0, 21, "pm")]  # bits past the length are not read


def test_format_rows_and_report_totals():
    rows = trio.format_rows([("ctg", 21, 1000, 980, 7, 3, 4, 2, 1, 2), ("e", 21, 0, 0, 0, 0, 0, 0, 0, 0)])
    assert rows == ["ctg\t21\t1000\t980\t7\t3\t4\t2\t1\t2\t3\t0.333333\t3\t0.300000\n", "e\t21\t0\t0\t0\t0\t0\t0\t0\t0\t0\tnan\t0\tnan\n"]
    assert trio.TSV_HEADER == ("contig", "k", "len", "kmers", "pat", "mat", "pp", "pm", "mp", "mm", "switch", "switch_rate", "hamming", "hamming_rate")
    rep = trio.TrioReport(21)
    rep.rows = [("a", [(100, 80, 7, 3, 4, 2, 1, 2), (101, 81, 10, 0, 9, 0, 0, 0)]),
                ("b", [(50, 30, 1, 5, 0, 0, 1, 4), (50, 30, 0, 6, 0, 0, 0, 5)])]
    lines = rep.lines(trio.CLI_HEADER)
    head = lines[0].rstrip("\n").split("\t")
    assert head[:2] == ["contig", "k"] and head[2:14] == [c + "_in" for c in ("len",) + trio.STAT_NAMES] and head[14:] == [c + "_out" for c in ("len",) + trio.STAT_NAMES]
    assert [ln.split("\t")[0] for ln in lines[1:]] == ["a", "b", "total"]
    # the totals are sums of the integers: switch 4 of 15 pairs, hamming min(8, 8) of 16 markers; out: 0 of 14, min(10, 6) of 16
    assert lines[3].rstrip("\n").split("\t")[2:] == ["150", "110", "8", "8", "4", "2", "2", "6", "4", "0.285714", "8", "0.500000",
                                                     "151", "111", "10", "6", "9", "0", "0", "5", "0", "0.000000", "6", "0.375000"]
    assert lines[1].split("\t")[10:14] == ["3", "0.333333", "3", "0.300000"]
    rep.beds["in"] = [("a", 3, 40, "pm"), ("b", 0, 9, "mp")]
    assert rep.bed_text("in") == "a\t3\t40\tpm\nb\t0\t9\tmp\n" and rep.bed_text("out") == ""


# ---- 3. arguments are checked before any device is touched -------------------------------------------------------------
ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
K21, K31 = os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")


def test_cli_rejects_trio_argument_errors_at_parsing(tmp_path):
    tsv, out = str(tmp_path / "t.tsv"), str(tmp_path / "o.fa")
    base = [sys.executable, "-m", "nextpolish2_amd.cli", BAM, ASM_IN, K21, "-o", out]
    both = ["--trio_pat", K21, "--trio_mat", K21]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, env=ENV)
        assert not os.path.exists(out) and not os.path.exists(tsv) and r.stdout == "", extra
        return r

    for extra in (["--trio", tsv], ["--trio", tsv, "--trio_pat", K21], ["--trio", tsv, "--trio_mat", K21]):
        r = run(extra)
        assert r.returncode == 2 and "--trio needs both --trio_pat and --trio_mat" in r.stderr
    r = run(both + ["--trio_bed", str(tmp_path / "p")])
    assert r.returncode == 2 and "--trio_bed needs --trio" in r.stderr
    r = run(["--trio", tsv, "--out_pos"] + both)
    assert r.returncode == 2 and "--out_pos" in r.stderr and "--trio" in r.stderr
    for lo, hi in ((0, 5), (6, 5), (2, 1024), (-1, 5)):
        r = run(["--trio", tsv, "--trio_min_count", str(lo), "--trio_mid_count", str(hi)] + both)
        assert r.returncode == 2 and "--trio_min_count" in r.stderr and "--trio_mid_count" in r.stderr
    # parental dumps of different k: a clean exit before the output exists
    r = run(["--trio", tsv, "--trio_pat", K21, "--trio_mat", K31])
    assert r.returncode == 1 and "Error:" in r.stderr and "different k" in r.stderr and "Traceback" not in r.stderr


def test_trio_module_rejects_argument_errors_at_parsing(tmp_path):
    mod = [sys.executable, "-m", "nextpolish2_amd.trio", ASM_IN]
    reads = os.path.join(BUNDLE, "sr.seq.0.gz")

    def run(extra):
        return subprocess.run(mod + extra, capture_output=True, text=True, timeout=600, env=ENV)

    for extra, text in (([], "--pat_sr"), ([K21], "exactly two"), ([K21, K21, K21], "exactly two"), (["--pat_sr", reads], "--mat_sr"),
                        (["--mat_sr", reads], "--pat_sr"), ([K21, K21, "--pat_sr", reads], "not both"),
                        ([K21, K21, "--min_count", "0"], "--min_count"), ([K21, K21, "--min_count", "6"], "--mid_count"),
                        ([K21, K21, "--mid_count", "1024"], "--mid_count"),
                        (["--pat_sr", reads, "--mat_sr", reads, "--sr_k", "32"], "--sr_k"),
                        (["--pat_sr", reads, "--mat_sr", reads, "--sr_min_count", "0"], "--sr_min_count")):
        r = run(extra)
        assert r.returncode == 2 and text in r.stderr and r.stdout == "", (extra, r.stderr)
    r = run([K21, K31])
    assert r.returncode == 1 and "Error:" in r.stderr and "different k" in r.stderr and "Traceback" not in r.stderr
    with pytest.raises(ValueError):
        trio.parental_k(K21, K31)
    assert trio.parental_k(K21, K21) == 21


def test_abi_declares_the_two_entries():
    from nextpolish2_amd import api
    L = api.lib()
    for s in ("np2_trio_strings", "np2_trio_device"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "np2.h")).read()
    assert "np2_trio_strings(" in header and "np2_trio_device(" in header and "np2_trio_t" in header
    assert hasattr(api.Polisher, "trio_strings") and hasattr(api.Polisher, "trio_device")
