"""The read binner's host side, without a GPU: the scan's per-lane core as a one-lane host program
(csrc/np2_bin_core.hpp through tests/tools/bin_core_test.cpp, which walks a PACKED separator stream in stretches that
fall anywhere and joins them by the segmented scan), the reader's names and boundaries (np2_seqfile_reads), the
device-free helpers of nextpolish2_amd.triobin and its argument checks.

The independent expectation is numpy_trio of test_trio_cpu.py applied to every read on its own, and the class rule
written out again below (expected_class)."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from nextpolish2_amd import api, triobin
from nextpolish2_amd import io as np2io
from test_kcount_cpu import awkward_stream, dump_bytes, numpy_count
from test_qv_cpu import BUNDLE
from test_trio_cpu import numpy_trio, random_bases, sorted_table, table_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
K21, K31 = os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")
STRETCHES = (1, 7, 32, 64, 0)  # 0: the whole stream as one stretch


def expected_class(s_pat, s_mat, min_score=2, minor_permille=330):
    """the class rule of the issue, written out again (exact integers)"""
    if s_pat < min_score and s_mat < min_score:
        return "0"
    if s_pat == s_mat:
        return "a"
    big, small = max(s_pat, s_mat), min(s_pat, s_mat)
    if small * 1000 > big * minor_permille:
        return "a"
    return "p" if s_pat > s_mat else "m"


def brute_force(reads, k, tp, tm, min_count, mid_count, min_score=2, minor_permille=330):
    """[(tallies, class)] per read: numpy_trio of every read as a sequence of its own"""
    out = []
    for r in reads:
        st = numpy_trio(r, k, tp, tm, min_count, mid_count)[0]
        out.append((st, expected_class(st[3], st[6], min_score, minor_permille)))
    return out


# ---- 1. the per-lane core ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bin") / "bin_core_test")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "tools", "bin_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_core(exe, thresholds, score, pat, mat, stream_path, stretch):
    r = subprocess.run([exe] + [str(x) for x in thresholds + score] + [pat, mat, stream_path, str(stretch)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rows = [ln.split(" ") for ln in r.stdout.splitlines()]
    assert all(f[0] == "read" for f in rows)
    return [(tuple(int(x) for x in f[1:8]), f[8]) for f in rows]


def check_core(exe, tmp_path, k, pat, mat, reads, thresholds, scores=((2, 330),), stretches=STRETCHES, tag=""):
    """the core's tallies and classes of a packed stream == the brute force per read, wherever the stretches fall"""
    src = tmp_path / f"stream{tag}.k{k}.bin"
    src.write_bytes(b"".join(r + b"\n" for r in reads))
    paths = []
    for name, (words, off) in (("pat", pat), ("mat", mat)):
        p = tmp_path / f"{name}{tag}.k{k}.yak"
        p.write_bytes(dump_bytes(k, words, off))
        paths.append(str(p))
    tp, tm = sorted_table(*pat), sorted_table(*mat)
    seen = set()
    for th in thresholds:
        tallies = [st for st, _ in brute_force(reads, k, tp, tm, th[0], th[1])]  # (once per pair of thresholds)
        for sc in scores:
            exp = [(st, expected_class(st[3], st[6], sc[0], sc[1])) for st in tallies]
            for stretch in stretches:
                got = run_core(exe, tuple(th), tuple(sc), paths[0], paths[1], str(src), stretch)
                assert len(got) == len(reads)
                for i, (e, g) in enumerate(zip(exp, got)):
                    assert g == e, (k, th, sc, stretch, i, reads[i][:60])
            seen.update(c for _, c in exp)
    return seen


def test_core_on_awkward_reads(core_exe, tmp_path):
    """Lower case, U, N, bytes >= 0x80, empty reads and runs of consecutive separators, reads shorter than k.  The paternal
    table counts every read once and the even reads four times more, the maternal table the odd reads; reads joined in
    threes switch parents inside a read."""
    stream = awkward_stream()
    reads = stream.split(b"\n")[:-1]
    even = b"".join(s + b"\n" for s in reads[0::2])
    odd = b"".join(s + b"\n" for s in reads[1::2])
    joined = [b"".join(reads[i:i + 3]) for i in range(0, len(reads) - 2, 3)]
    packed = reads[:40] + [b"", b"", b""] + joined[:30] + [b""] + reads[40:] + [b"", b""]
    for k in (11, 21, 31):
        pat, mat = numpy_count(stream + even * 4, k), numpy_count(stream + odd * 4, k)
        seen = check_core(core_exe, tmp_path, k, pat, mat, packed, [(2, 5), (1, 1)], scores=((2, 330), (1, 0), (3, 1000)))
        if k == 11:
            assert {"p", "m", "0"} <= seen


def test_core_on_lengths_around_k(core_exe, tmp_path):
    rng = np.random.default_rng(3)
    for k in (21, 31):
        base = random_bases(rng, 400)
        rev = base[::-1]  # (not the complement: other k-mers)
        pat, mat = numpy_count((base + b"\n") * 5, k), numpy_count((rev + b"\n") * 5, k)
        reads = [b"", base[:k - 1], base[:k], base[:k + 1], base[:k + 2], rev[:k - 1], rev[:k], rev[:k + 1], rev[:k + 2], b"", b"",
                 base[:k] + b"N" + rev[:k], base[:60].lower(), rev[:60].replace(b"T", b"U"), base[:200] + rev[:100], base[:150] + rev[:150], b""]
        check_core(core_exe, tmp_path, k, pat, mat, reads, [(2, 5)], scores=((2, 330), (1, 330)))
        exp = brute_force(reads, k, sorted_table(*pat), sorted_table(*mat), 2, 5)
        # k - 1: no k-mer; k: one marker, no pair; k + 1: one pair, below min_score 2; k + 2: two pairs
        assert [c for _, c in exp[:11]] == ["0", "0", "0", "0", "p", "0", "0", "0", "m", "0", "0"]
        assert exp[4][0] == (3, 3, 0, 2, 0, 0, 0) and exp[8][0] == (3, 0, 3, 0, 0, 0, 2)
        assert exp[11] == ((2, 1, 1, 0, 1, 0, 0), "0")  # a non-base breaks k-mers, not adjacency: one pm pair, no score
        assert exp[12][1] == "p" and exp[13][1] == "m"  # lower case and U are bases
        assert exp[14][1] == "a" and exp[15][1] == "a"  # 80 to 180 maternal pairs against 180 / 130 paternal ones


def test_core_a_boundary_at_every_phase_of_a_stretch(core_exe, tmp_path):
    """the same reads behind padding reads of every length 0 .. 32: a boundary falls at every place of a 32-byte stretch"""
    rng = np.random.default_rng(8)
    k = 21
    base = random_bases(rng, 3000)
    alt = random_bases(rng, 3000)
    pat, mat = numpy_count((base + b"\n") * 5, k), numpy_count((alt + b"\n") * 5, k)
    body = [base[100:250], alt[5:70], b"", base[300:330] + alt[300:330] + base[330:360], alt[1000:1300], b"", b"", base[:k]]
    reads = []
    for pad in range(33):
        reads += [random_bases(rng, pad)] + body
    seen = check_core(core_exe, tmp_path, k, pat, mat, reads, [(2, 5)], stretches=(32, 64, 0))
    assert {"p", "m", "0"} <= seen


def test_core_refuses_options_outside_the_rule(core_exe, tmp_path):
    src = tmp_path / "s.bin"
    src.write_bytes(b"ACGTACGT\n")
    paths = []
    for name in ("p", "m"):
        p = tmp_path / f"{name}.yak"
        p.write_bytes(dump_bytes(5, *table_of([], [])))
        paths.append(str(p))
    for args in ((0, 5, 2, 330), (6, 5, 2, 330), (2, 1024, 2, 330), (2, 5, 2, 1001)):
        r = subprocess.run([core_exe] + [str(x) for x in args] + paths + [str(src), "0"], capture_output=True, timeout=600)
        assert r.returncode == 6, args
    src.write_bytes(b"ACGTACGT")  # no separator at the end
    r = subprocess.run([core_exe, "2", "5", "2", "330"] + paths + [str(src), "0"], capture_output=True, timeout=600)
    assert r.returncode == 7


# ---- 2. the class rule ---------------------------------------------------------------------------------------------------
HAND_TABLE = [((0, 0), "0"), ((1, 0), "0"), ((2, 0), "p"), ((0, 2), "m"), ((3, 3), "a"), ((100, 33), "p"), ((100, 34), "a"), ((1, 5), "m")]


def core_class(exe, s_pat, s_mat, min_score, permille):
    r = subprocess.run([exe, "class", str(s_pat), str(s_mat), str(min_score), str(permille)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0
    return r.stdout.strip()


def test_hand_derived_class_table(core_exe):
    for (pp, mm), cls in HAND_TABLE:  # at the defaults; (100, 33): 33 000 <= 33 000 is not "more than"
        assert triobin.classify(pp, mm) == cls, (pp, mm)
        assert core_class(core_exe, pp, mm, 2, 330) == cls, (pp, mm)
        assert expected_class(pp, mm) == cls
        mirror = {"p": "m", "m": "p"}.get(cls, cls)
        assert triobin.classify(mm, pp) == mirror and core_class(core_exe, mm, pp, 2, 330) == mirror
    # minor_permille 0: any S > 0 gives a; 1000: only equal scores do
    for pp, mm, at0, at1000 in ((5, 0, "p", "p"), (5, 1, "a", "p"), (1, 5, "a", "m"), (1000000, 1, "a", "p"), (7, 7, "a", "a"),
                                (1000, 999, "a", "p"), (4000000000, 3999999999, "a", "p"), (4000000000, 4000000000, "a", "a")):
        for fn in (triobin.classify, lambda a, b, s, p: core_class(core_exe, a, b, s, p), expected_class):
            assert fn(pp, mm, 2, 0) == at0, (pp, mm)
            assert fn(pp, mm, 2, 1000) == at1000, (pp, mm)
    # min_score: both scores below it is class 0, whatever their ratio; 0 lets nothing be class 0
    assert triobin.classify(4, 0, 5, 330) == "0" and triobin.classify(5, 0, 5, 330) == "p" and triobin.classify(5, 4, 5, 330) == "a"
    assert triobin.classify(0, 0, 0, 330) == "a" and core_class(core_exe, 0, 0, 0, 330) == "a"
    assert core_class(core_exe, 4, 0, 5, 330) == "0" and core_class(core_exe, 0, 5, 5, 330) == "m"
    # the largest scores a read can have do not overflow the 64-bit products
    top = 2 ** 32 - 2
    assert core_class(core_exe, top, top - 1, 2, 999) == "a" and core_class(core_exe, top, top // 3, 2, 330) == "a"
    assert core_class(core_exe, top, top // 4, 2, 330) == "p" and triobin.classify(top, top // 4) == "p"


def test_keep_rule_and_permille():
    assert [triobin.keep(c, "pat") for c in "pma0"] == [True, False, True, True]
    assert [triobin.keep(c, "mat") for c in "pma0"] == [False, True, True, True]
    for bad in (("x", "pat"), ("p", "both"), ("", "mat")):
        with pytest.raises(ValueError):
            triobin.keep(*bad)
    assert triobin.permille_of(0.33) == 330 and triobin.permille_of(0) == 0 and triobin.permille_of(1) == 1000
    assert triobin.permille_of(0.0005) == 0 and triobin.permille_of(0.0015) == 2 and triobin.permille_of(0.29) == 290
    assert triobin.TSV_HEADER == ("read", "class", "s_pat", "s_mat", "n_pat", "n_mat", "pm", "mp", "kmers", "len")
    text = triobin.summary_text({"p": 3, "m": 1, "a": 0, "0": 4})
    assert "p\t3\t0.375000\n" in text and "paternal bin\t7\n" in text and "maternal bin\t5\n" in text
    assert "nan" in triobin.summary_text({"p": 0, "m": 0, "a": 0, "0": 0})


# ---- 3. the reader: names and boundaries -----------------------------------------------------------------------------------
def reads_of(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    names, ends = np2io.seqfile_reads(str(p))
    stream = np2io.seqfile_stream(str(p))
    # the boundaries are the stream's separators, one per read
    assert [int(e) for e in ends] == [i for i, c in enumerate(stream) if c == 10] and len(names) == len(ends)
    assert stream == b"" or stream.endswith(b"\n")
    cuts = [0] + [int(e) + 1 for e in ends]
    return names, [stream[a:b - 1] for a, b in zip(cuts[:-1], cuts[1:])]


def test_reader_names_and_boundaries(tmp_path):
    # multi-line FASTA joined, a description behind the name, an empty record, a tab after the name, no final newline
    fa = b">c1 desc ription\nACG\nTTA\n>c2\n>c3\tx\nGG\nAA"
    assert reads_of(tmp_path, "a.fa", fa) == (["c1", "c2", "c3"], [b"ACGTTA", b"", b"GGAA"])
    assert reads_of(tmp_path, "crlf.fa", fa.replace(b"\n", b"\r\n")) == (["c1", "c2", "c3"], [b"ACGTTA", b"", b"GGAA"])
    assert reads_of(tmp_path, "a.fa.gz", gzip.compress(fa)) == (["c1", "c2", "c3"], [b"ACGTTA", b"", b"GGAA"])
    # FASTQ by the 4-line rule: quality lines that begin with '@' and with '>', an empty read, a missing final newline
    fq = b"@r1 x\nACGT\n+\n@III\n@r2/1\nGGNcc\n+r2\n>>>>>\n@r3\n\n+\n\n@r4\nTTTT\n+\nIIII"
    exp = (["r1", "r2/1", "r3", "r4"], [b"ACGT", b"GGNcc", b"", b"TTTT"])
    assert reads_of(tmp_path, "a.fq", fq) == exp
    assert reads_of(tmp_path, "crlf.fq", fq.replace(b"\n", b"\r\n")) == exp
    assert reads_of(tmp_path, "a.fq.gz", gzip.compress(fq)) == exp
    two = gzip.compress(b"@r1\nACGT\n+\nIIII\n") + gzip.compress(b"@r2\nGGCC\n+\nIIII\n")  # two gzip members
    assert reads_of(tmp_path, "two.fq.gz", two) == (["r1", "r2"], [b"ACGT", b"GGCC"])
    assert reads_of(tmp_path, "cut.fq", b"@r1\nACGT\n+\nIIII\n@r2\nGG") == (["r1", "r2"], [b"ACGT", b"GG"])
    assert reads_of(tmp_path, "head.fq", b"@r1\nACGT\n+\nIIII\n@r2\n") == (["r1"], [b"ACGT"])  # a header that names nothing
    # one sequence per line: no names, the reads are numbered from 1
    assert reads_of(tmp_path, "lines.txt", b"ACGT\nGG\n\nTT") == (["1", "2", "3", "4"], [b"ACGT", b"GG", b"", b"TT"])
    assert reads_of(tmp_path, "empty.fa", b"") == ([], [])
    # a header longer than the reader's buffer pieces, names kept whole across them
    long_name = b"n" * 70000
    big = b"".join(b">" + long_name + b"%d rest\n" % i + b"ACGT" * 5000 + b"\n" for i in range(60))
    names, reads = reads_of(tmp_path, "big.fa.gz", gzip.compress(big))
    assert names == [(long_name + b"%d" % i).decode() for i in range(60)] and reads == [b"ACGT" * 5000] * 60
    with pytest.raises(api.Np2Error) as e:
        np2io.seqfile_reads(str(tmp_path / "missing.fq"))
    assert e.value.code == -1 and "cannot open" in str(e.value)


# ---- 4. arguments are checked before any device is touched -------------------------------------------------------------
def test_triobin_module_rejects_argument_errors_at_parsing(tmp_path):
    mod = [sys.executable, "-m", "nextpolish2_amd.triobin"]
    reads = os.path.join(BUNDLE, "sr.seq.0.gz")
    tsv = str(tmp_path / "t.tsv")

    def run(extra):
        r = subprocess.run(mod + ["-o", tsv] + extra, capture_output=True, text=True, timeout=600, env=ENV)
        assert not os.path.exists(tsv) and r.stdout == "", extra
        return r

    missing = str(tmp_path / "missing.yak")
    for extra, text in (([], "--pat_sr"), ([K21], "--pat_sr"), ([K21, K21], "no read file"), (["--pat_sr", reads, reads], "--mat_sr"),
                        (["--mat_sr", reads, reads], "--pat_sr"), (["--pat_sr", reads, "--mat_sr", reads], "no read file"),
                        ([K21, K21, reads, "--min_count", "0"], "--min_count"), ([K21, K21, reads, "--min_count", "6"], "--mid_count"),
                        ([K21, K21, reads, "--mid_count", "1024"], "--mid_count"), ([K21, K21, reads, "--min_score", "-1"], "--min_score"),
                        ([K21, K21, reads, "--max_minor", "1.01"], "--max_minor"), ([K21, K21, reads, "--max_minor", "-0.1"], "--max_minor"),
                        ([K21, K21, reads, "--max_minor", "nan"], "--max_minor"), ([K21, K21, reads, "--max_minor", "x"], "--max_minor"),
                        ([missing, K21, reads], "cannot open"), ([K21, missing, reads], "cannot open"),
                        ([K21, K21, str(tmp_path / "missing.fa")], "cannot open"),
                        (["--pat_sr", reads, "--mat_sr", str(tmp_path / "missing.fq"), "--", reads], "cannot open"),
                        (["--pat_sr", reads, "--mat_sr", reads, "--sr_k", "32", "--", reads], "--sr_k"),
                        (["--pat_sr", reads, "--mat_sr", reads, "--sr_min_count", "0", "--", reads], "--sr_min_count")):
        r = run(extra)
        assert r.returncode == 2 and text in r.stderr, (extra, r.stderr)
    r = run([K21, K31, reads])  # parental dumps of different k: a clean exit before the output exists
    assert r.returncode == 1 and "Error:" in r.stderr and "different k" in r.stderr and "Traceback" not in r.stderr
    a = triobin.parse_args([K21, K21, reads, reads, "--max_minor", "0.25", "--pat_list", "x"])
    assert (a.yak, a.reads, a.minor_permille, a.min_score) == ([K21, K21], [reads, reads], 250, 2)
    a = triobin.parse_args(["--pat_sr", reads, "--mat_sr", reads, reads, "--", reads])
    assert (a.yak, a.reads, a.pat_sr, a.mat_sr) == ([], [reads], [reads], [reads, reads])


def test_abi_declares_the_entries():
    L = api.lib()
    assert "np2_bin_stream" in api.ABI_SYMBOLS and hasattr(L, "np2_bin_stream")
    for s in ("np2_bin_files", "np2_seqfile_reads"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "np2.h")).read()
    assert "np2_bin_stream(" in header and "np2_bin_t" in header and "np2_bin_opts_t" in header
    assert hasattr(api.Polisher, "bin_stream")
    import ctypes as C
    assert C.sizeof(api.np2_bin_opts_t) == 12 and api.np2_bin_opts_t.min_score.offset == 4 and api.BIN_DTYPE.itemsize == 28
