"""The k-mer QV measurement's host side, without a GPU: the scan's per-lane core as a one-lane host program
(csrc/np2_qv_core.hpp through tests/tools/qv_core_test.cpp, which looks hashes up by binary search in a dump), the host
helpers of nextpolish2_amd.qv, and the command line's argument checks.

Known answer (computed with numpy: stream_hashes of test_kcount_cpu.py against the words of the committed dumps), for
tests/golden/ref_test_asm.fa.gz (input, 100 000 bases) and tests/golden/ref_bundle/expected.fa.gz (polished, 100 004
bases) against ref_bundle/k21.yak and k31.yak, min_count 1 (and 2: the dumps hold no singletons):

    k21: input 99 980 k-mers / 32 absent / QV 48.1692      polished 99 984 / 0 / inf
    k31: input 99 970 / 82 / 45.7725                       polished 99 974 / 10 / 54.9123

The independent expectation is the numpy brute force below (numpy_qv)."""
import gzip
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from nextpolish2_amd import qv
from test_kcount_cpu import hash64

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUNDLE = os.path.join(HERE, "golden", "ref_bundle")
ASM_IN = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
ASM_OUT = os.path.join(BUNDLE, "expected.fa.gz")
BAM = os.path.join(BUNDLE, "hifi.map.sort.bam")
KNOWN = {  # (k, side): (length, k-mers, absent, QV text)
    (21, "in"): (100000, 99980, 32, "48.1692"), (21, "out"): (100004, 99984, 0, "inf"),
    (31, "in"): (100000, 99970, 82, "45.7725"), (31, "out"): (100004, 99974, 10, "54.9123"),
}
FASTA = {"in": ASM_IN, "out": ASM_OUT}


# ---- the numpy brute force ---------------------------------------------------------------------------------------------
def kmer_hashes_at(seq, k):
    """(valid, hashes): per base e of `seq`, whether a k-mer ENDS there (its k bytes are all ACGTUacgtu) and its table
    hash (0 where none does)."""
    lut = np.full(256, 4, np.uint8)
    for ch, v in zip(b"ACGTU", (0, 1, 2, 3, 3)):
        lut[ch] = v
        lut[ch | 0x20] = v
    c = lut[np.frombuffer(bytes(seq), dtype=np.uint8)]
    L = c.shape[0]
    valid, hashes = np.zeros(L, bool), np.zeros(L, np.uint64)
    n = L - k + 1
    if n <= 0:
        return valid, hashes
    bad = np.concatenate([[0], np.cumsum(c == 4)])
    ok = (bad[k:] - bad[:-k]) == 0
    c64 = (c & 3).astype(np.uint64)
    fw, rv = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        fw |= c64[j:j + n] << np.uint64(2 * (k - 1 - j))
        rv |= (np.uint64(3) ^ c64[j:j + n]) << np.uint64(2 * j)
    h = hash64(np.minimum(fw, rv), np.uint64((1 << (2 * k)) - 1))
    valid[k - 1:] = ok
    hashes[k - 1:] = np.where(ok, h, np.uint64(0))
    return valid, hashes


def read_dump(path):
    """(k, sorted hashes, their counts) of a yak v2 dump without repeated keys"""
    raw = open(path, "rb").read()
    assert raw[:4] == b"YAK\x02"
    k, pre, cbits = struct.unpack("<III", raw[4:16])
    assert pre == 10 and cbits == 10
    at, hs, cs = 16, [], []
    for b in range(1024):
        n = struct.unpack("<II", raw[at:at + 8])[1]
        w = np.frombuffer(raw, dtype=np.uint64, count=n, offset=at + 8)
        at += 8 + 8 * n
        hs.append(((w >> np.uint64(10)) << np.uint64(10)) | np.uint64(b))
        cs.append((w & np.uint64(1023)).astype(np.uint32))
    h, c = np.concatenate(hs), np.concatenate(cs)
    order = np.argsort(h)
    h, c = h[order], c[order]
    assert len(np.unique(h)) == len(h)
    return k, h, c


def table_counts(table, hashes, min_count):
    """count(k-mer) per hash: the stored count if >= min_count, else 0"""
    th, tc = table
    if len(th) == 0:
        return np.zeros(len(hashes), np.uint32)
    at = np.minimum(np.searchsorted(th, hashes), len(th) - 1)
    c = np.where(th[at] == hashes, tc[at], 0).astype(np.uint32)
    return np.where(c >= min_count, c, 0).astype(np.uint32)


def aggregate(valid, counts):
    """(n_kmers, n_absent, hist[1024], bitmap bytes) of one sequence from its per-base validity and counts"""
    miss = valid & (counts == 0)
    hist = np.bincount(counts[valid].astype(np.int64), minlength=1024).astype(np.uint64)
    return int(valid.sum()), int(miss.sum()), hist, np.packbits(miss, bitorder="little")


def numpy_qv(seq, k, table, min_count):
    valid, hashes = kmer_hashes_at(seq, k)
    return aggregate(valid, table_counts(table, hashes, min_count))


def fasta_records(path):
    recs, name = [], None
    for ln in gzip.open(path, "rb").read().split(b"\n"):
        if ln.startswith(b">"):
            name = ln[1:].split()[0].decode()
            recs.append([name, b""])
        elif recs:
            recs[-1][1] += ln.strip()
    return [(n, s) for n, s in recs]


# ---- 1. the per-lane core ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qv") / "qv_core_test")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "tools", "qv_core_test.cpp"), "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_core(exe, min_count, dump, seqfile):
    r = subprocess.run([exe, str(min_count), dump, seqfile], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    stats, hist, bits = [], np.zeros(1024, np.uint64), []
    for ln in r.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "seq":
            stats.append((int(f[1]), int(f[2])))
        elif f[0] == "hist":
            hist[int(f[1])] = int(f[2])
        elif f[0] == "bits":
            bits.append(np.frombuffer(bytes.fromhex(f[1]) if len(f) > 1 else b"", dtype=np.uint8))
    return stats, hist, bits


@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("side", ["in", "out"])
@pytest.mark.parametrize("min_count", [1, 2])
def test_core_reproduces_the_known_answer(core_exe, k, side, min_count):
    dump = os.path.join(BUNDLE, f"k{k}.yak")
    stats, hist, bits = run_core(core_exe, min_count, dump, FASTA[side])
    length, n_kmers, n_absent, text = KNOWN[(k, side)]
    assert stats == [(n_kmers, n_absent)]
    (name, seq), = fasta_records(FASTA[side])
    dk, th, tc = read_dump(dump)
    assert dk == k and len(seq) == length and int(tc.min()) >= 2  # (no singletons: min_count 1 and 2 agree)
    e_kmers, e_absent, e_hist, e_bits = numpy_qv(seq, k, (th, tc), min_count)
    assert (e_kmers, e_absent) == (n_kmers, n_absent)
    assert np.array_equal(hist, e_hist) and int(hist.sum()) == n_kmers and int(hist[0]) == n_absent
    assert len(bits) == 1 and np.array_equal(bits[0], e_bits)
    assert qv.qv_text(n_kmers, n_absent, k) == text


def test_core_on_awkward_sequences(core_exe, tmp_path):
    """One sequence per line: lower case, U, N, bytes >= 0x80, lengths around k, an empty line; thresholds above 1."""
    from test_kcount_cpu import awkward_stream, dump_bytes, numpy_count
    stream = awkward_stream()
    seqs = stream.split(b"\n")[:-1]
    src = tmp_path / "s.txt"
    src.write_bytes(stream)
    for k in (2, 16, 31):
        words, off = numpy_count(stream, k, 1)
        dump = tmp_path / f"k{k}.yak"
        dump.write_bytes(dump_bytes(k, words, off))
        _, th, tc = read_dump(str(dump))
        for min_count in (0, 1, 3, 1023):
            stats, hist, bits = run_core(core_exe, min_count, str(dump), str(src))
            assert len(stats) == len(seqs) == len(bits)
            e_hist = np.zeros(1024, np.uint64)
            for s, st, bm in zip(seqs, stats, bits):
                nk, na, h, b = numpy_qv(s, k, (th, tc), min_count)
                assert st == (nk, na) and np.array_equal(bm, b), (k, min_count, s)
                e_hist += h
            assert np.array_equal(hist, e_hist)
            if min_count <= 1:  # every k-mer of the stream is in a table counted from it
                assert all(na == 0 for _, na in stats)


# ---- 2. host helpers -------------------------------------------------------------------------------------------------------
def test_qv_value():
    for (k, _), (_, n_kmers, n_absent, text) in KNOWN.items():
        assert qv.qv_text(n_kmers, n_absent, k) == text
        if n_absent:  # Merqury's formula as written
            assert abs(qv.qv_value(n_kmers, n_absent, k) - -10 * math.log10(1 - (1 - n_absent / n_kmers) ** (1 / k))) < 1e-6
    assert qv.qv_value(99984, 0, 21) == math.inf and qv.qv_text(99984, 0, 21) == "inf"
    assert math.isnan(qv.qv_value(0, 0, 21)) and qv.qv_text(0, 0, 21) == "nan"
    # the ends of the supported k: P = 0.81 at k = 2 is E = 0.1; P = 0.999^31 at k = 31 is E = 0.001
    assert qv.qv_text(100, 19, 2) == "10.0000"
    n = 10 ** 12
    assert qv.qv_text(n, round(n * (1 - 0.999 ** 31)), 31) == "30.0000"
    assert qv.qv_text(7, 7, 21) == "0.0000"  # every k-mer absent: E = 1


def bitmap(length, ends):
    b = np.zeros(length, bool)
    b[list(ends)] = True
    return np.packbits(b, bitorder="little")


def test_bed_intervals():
    k = 5
    assert qv.bed_intervals(bitmap(40, []), 40, k) == []
    assert qv.bed_intervals(np.zeros(0, np.uint8), 0, k) == []
    assert qv.bed_intervals(bitmap(40, [4]), 40, k) == [(0, 5)]                      # e = k - 1: start 0
    assert qv.bed_intervals(bitmap(40, [39]), 40, k) == [(35, 40)]                   # the last base
    assert qv.bed_intervals(bitmap(40, [10, 11, 12]), 40, k) == [(6, 13)]            # overlapping
    assert qv.bed_intervals(bitmap(40, [10, 15]), 40, k) == [(6, 16)]                # touching: [6, 11) and [11, 16)
    assert qv.bed_intervals(bitmap(40, [10, 16]), 40, k) == [(6, 11), (12, 17)]      # one base apart: two intervals
    assert qv.bed_intervals(bitmap(40, [4, 9, 20, 39]), 40, k) == [(0, 10), (16, 21), (35, 40)]
    assert qv.bed_intervals(bitmap(37, [36]), 37, k) == [(32, 37)]                   # a length that is no multiple of 8
    assert qv.bed_intervals(bitmap(8, [7]), 8, 2) == [(6, 8)]


def test_format_rows_and_report_totals():
    rows = qv.format_rows([("ctg", 21, 100000, 99980, 32, 100004, 99984, 0), ("e", 31, 0, 0, 0, 0, 0, 0)])
    assert rows == ["ctg\t21\t100000\t99980\t32\t48.1692\t100004\t99984\t0\tinf\n", "e\t31\t0\t0\t0\tnan\t0\t0\t0\tnan\n"]
    rep = qv.QvReport([21, 31])
    rep.rows = [("a", [[(10, 5, 1), (11, 6, 0)], [(10, 2, 2), (11, 3, 1)]]), ("b", [[(30, 10, 0), (30, 10, 0)], [(30, 0, 0), (30, 0, 0)]])]
    lines = rep.lines(qv.CLI_HEADER)
    assert lines[0] == "contig\tk\tlen_in\tkmers_in\tabsent_in\tqv_in\tlen_out\tkmers_out\tabsent_out\tqv_out\n"
    assert [ln.split("\t")[:2] for ln in lines[1:]] == [["a", "21"], ["a", "31"], ["b", "21"], ["b", "31"], ["total", "21"], ["total", "31"]]
    assert lines[5].split("\t")[2:] == ["40", "15", "1", qv.qv_text(15, 1, 21), "41", "16", "0", "inf\n"]
    assert lines[6].split("\t")[2:] == ["40", "2", "2", "0.0000", "41", "3", "1", qv.qv_text(3, 1, 31) + "\n"]


# ---- 3. arguments are checked before any device is touched -------------------------------------------------------------
def test_cli_rejects_qv_with_out_pos_at_argument_parsing(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tsv, out = str(tmp_path / "q.tsv"), str(tmp_path / "o.fa")
    base = [sys.executable, "-m", "nextpolish2_amd.cli", BAM, ASM_IN, os.path.join(BUNDLE, "k21.yak"), "-o", out]
    r = subprocess.run(base + ["--qv", tsv, "--out_pos"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--out_pos" in r.stderr and "--qv" in r.stderr and r.stdout == ""
    assert not os.path.exists(tsv) and not os.path.exists(out)
    r = subprocess.run(base + ["--qv_bed", str(tmp_path / "p")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--qv_bed needs --qv" in r.stderr and not os.path.exists(out)
    r = subprocess.run(base + ["--qv", tsv, "--qv_min_count", "2000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--qv_min_count" in r.stderr and not os.path.exists(out)
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.qv", ASM_IN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--sr" in r.stderr


def test_abi_declares_the_two_entries():
    from nextpolish2_amd import api
    L = api.lib()
    for s in ("np2_qv_strings", "np2_qv_device"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s)
