"""Short-read adapter trimming on the device (np2_sradapt_*, the *_ad counting entry points, python -m nextpolish2_amd.srqc
--sr_adapter, the command lines' --sr_adapter) against the plain-Python model of tests/sradapt_model.py.  The pairs are the
model's seeded generator (tests/test_sradapt_cpu.py asserts what it exercises) plus its hand-written edge pairs."""
import ctypes as C
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import sradapt_model as am
import srqc_model as sm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from test_kcount_cpu import BUNDLE, stream_hashes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ASM = os.path.join(ROOT, "tests", "golden", "ref_test_asm.fa.gz")
BAM = os.path.join(BUNDLE, "hifi.map.sort.bam")
REF_PAIRS = [os.path.join(HERE, "golden", "ref_pairs", f"sr.{r}.2000.fastq.gz") for r in ("R1", "R2")]
ENV = dict(os.environ, PYTHONPATH=ROOT)
KS = [21, 31]
E_ARG = -1
BOTH = dict(seq=am.ADAPTER1, seq2=am.ADAPTER2)


def freeze(d):
    return tuple(sorted(d.items()))


@functools.lru_cache(maxsize=None)
def gen_reads():
    return tuple(am.generate()[0])


@functools.lru_cache(maxsize=None)
def edge_reads():
    return tuple(am.edge_pairs())


@functools.lru_cache(maxsize=None)
def _model(which, qc, o):
    reads = {"gen": gen_reads, "edge": edge_reads}[which]()
    return am.run(list(reads), dict(qc), dict(o))


def model(which, qc, o):
    """the model's (results, masked, totals) of the generated or the edge pairs, computed once per option set"""
    return _model(which, freeze(qc), freeze(o))


def device(reads, qc, o):
    seq, qual = sm.streams(reads)
    masked, got, totals = np2io.sradapt_bytes(seq, qual, np2io.SrQc(**qc), np2io.SrAdapt(**o))
    return [tuple(r) for r in got.tolist()], masked, totals


def same_as_model(reads, got, exp):
    bad = [(i, g, e, len(reads[i][0])) for i, (g, e) in enumerate(zip(got[0], exp[0])) if g != e]
    assert len(got[0]) == len(exp[0]) and not bad, (len(bad), bad[:5])
    assert got[1] == exp[1]
    assert got[2] == exp[2]


def same_yaks(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.k == e.k and np.array_equal(g.bucket_off, e.bucket_off) and np.array_equal(g.words, e.words), g.k


def write_pair_files(d, reads, tag="g"):
    """mates 1 as a plain FASTQ file, mates 2 as a gzip one"""
    a, b = d / f"{tag}.R1.fq", d / f"{tag}.R2.fq.gz"
    a.write_bytes(sm.fastq(reads[0::2], b"p"))
    b.write_bytes(gzip.compress(sm.fastq(reads[1::2], b"p"), 1))
    return [str(a), str(b)]


# ---- 1. np2_sradapt_bytes against the model -------------------------------------------------------------------------------------
VARIANTS = [("defaults", sm.opts(), am.adopts()), ("D10", sm.opts(), am.adopts(diff=10)), ("O15", sm.opts(), am.adopts(overlap=15)),
            ("single_by_sequence", sm.opts(), am.adopts(pair=False, seq=am.ADAPTER1)), ("pair_and_sequences", sm.opts(), am.adopts(**BOTH)),
            ("neutral", sm.NEUTRAL, am.adopts(**BOTH))]


@pytest.mark.parametrize("name,qc,o", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_stream_equals_the_model(name, qc, o):
    for which in ("gen", "edge"):  # (two calls: the model's two results are shared with the other tests)
        reads = list({"gen": gen_reads, "edge": edge_reads}[which]())
        same_as_model(reads, device(reads, qc, o), model(which, qc, o))
    assert {k: v for k, v in np2io.sradapt_last_stats().items() if k != "kernel_ms"} == model("edge", qc, o)[2]


# the edge pairs are written for the NEUTRAL quality options: here every one of them is what its comment says
EDGE_VARIANTS = [("D5", am.adopts()), ("D10", am.adopts(diff=10)), ("seq13", am.adopts(seq=am.EDGE_ADAPTER)), ("seq4", am.adopts(seq=am.EDGE_ADAPTER_4)),
                 ("seq64", am.adopts(seq=am.EDGE_ADAPTER_64)), ("seq13_seq64", am.adopts(seq=am.EDGE_ADAPTER, seq2=am.EDGE_ADAPTER_64)),
                 ("single_seq64", am.adopts(pair=False, seq=am.EDGE_ADAPTER_64)), ("single_seq4", am.adopts(pair=False, seq=am.EDGE_ADAPTER_4))]


@pytest.mark.parametrize("name,o", EDGE_VARIANTS, ids=[v[0] for v in EDGE_VARIANTS])
def test_edge_pairs_under_neutral_quality_options(name, o):
    reads = list(edge_reads())
    exp = model("edge", sm.NEUTRAL, o)
    same_as_model(reads, device(reads, sm.NEUTRAL, o), exp)
    if name == "D5":  # the cases are what they were written to be
        res, t = exp[0], exp[2]
        assert [r[4] for r in res[0:6:2]] == [30, 0, 0]                      # d = 5 accepted, 6 and 7 refused
        assert t["pairs_unsearched"] == 3 and t["too_short"] >= 4 and t["trimmed_overlap"] >= 10
        starts = np.cumsum([0] + [len(s) + 1 for s, _ in reads])[:-1]
        assert {int(x) % 4 for x in starts[-24:]} == {0, 1, 2, 3}
    if name == "D10":
        assert [r[4] for r in exp[0][0:10:2]] == [30, 30, 0, 49, 0]             # l = 30: 6 | 7; l = 49: 9 | 10
    if name == "seq13":
        assert exp[2]["trimmed_seq"] >= 10


def test_stream_argument_errors():
    seq, qual = sm.streams(list(edge_reads())[:6])
    L = np2io._bind()
    s, q = np.frombuffer(seq, np.uint8), np.frombuffer(qual, np.uint8)

    def call(o, n_reads=6, sq=s):
        return L.np2_sradapt_bytes(0, sq.ctypes.data, q.ctypes.data, len(s), None, C.byref(o) if o is not None else None, None, None, n_reads, None)
    o = np2io.SrAdapt(pair=True).c()
    assert call(o, 5) == E_ARG and "odd" in L.np2_io_last_error().decode()
    assert call(o, 8) == E_ARG and "n_reads" in L.np2_io_last_error().decode()
    o.overlap_min = 0
    assert call(o) == E_ARG and "overlap_min" in L.np2_io_last_error().decode()
    o = np2io.SrAdapt(pair=True).c()
    o.adapter1 = b"ACGN"
    assert call(o) == E_ARG and "ACGT" in L.np2_io_last_error().decode()
    o.adapter1, o.adapter2 = None, b"ACGT"
    assert call(o) == E_ARG and "adapter1" in L.np2_io_last_error().decode()
    o = np2io.SrAdapt(pair=True).c()
    o.flags = 0
    assert call(o) == E_ARG and "adapter1" in L.np2_io_last_error().decode()
    assert call(None) == 0  # NULL: pair mode with the defaults
    assert np2io.sradapt_bytes(b"", b"")[2] == dict.fromkeys(am.STAT_NAMES, 0)


# ---- 2. word ownership ----------------------------------------------------------------------------------------------------------
def test_neighbouring_mates_share_words():
    """mates of 1 .. 9 bases back to back in every rotation and at every offset of a word, every fourth read failing: every
    separator falls on each of the four byte positions, and a word at a boundary is shared by reads that are rewritten
    (failed, mate failed, trimmed) and reads that are not"""
    reads, k = [], 0
    for lead in range(4):
        if lead:
            reads += [(b"ACGT"[:lead - 1], b"I" * (lead - 1)), (b"", b"")]  # shifts what follows by `lead` + 1 bytes
        for rot in range(9):
            for j in range(10):
                n = 1 + (rot + j) % 9
                reads.append((b"ACGTAGATC"[:n], (b"#" if k % 4 == 1 else b"I") * n))
                k += 1
    seq, _ = sm.streams(reads)
    assert {int(x) % 4 for x in np.flatnonzero(np.frombuffer(seq, np.uint8) == 10)} == {0, 1, 2, 3}
    qc, o = sm.opts(sm.NEUTRAL, qualified_q=20, unqualified_percent=40), am.adopts(overlap=4, diff=0, seq="AGAT")
    exp = am.run(reads, qc, o)
    t = exp[2]
    assert t["pass"] > 100 and t["low_quality"] > 50 and t["mate_failed"] > 50 and t["trimmed_seq"] > 10 and t["pairs_overlap"] > 10
    same_as_model(reads, device(reads, qc, o), exp)


# ---- 3. piece boundaries --------------------------------------------------------------------------------------------------------
def test_a_piece_boundary_never_splits_a_pair(tmp_path, monkeypatch):
    """pairs of 150 + 150 bases are 302 bytes: pieces that hold one, two and three of them, through the stream entry point
    and through the two files read in step"""
    idx = [i for i in range(0, len(gen_reads()), 2) if len(gen_reads()[i][0]) == 150 and len(gen_reads()[i + 1][0]) == 150][:41]
    reads = [gen_reads()[i + m] for i in idx for m in (0, 1)]
    qc, o = sm.opts(), am.adopts(**BOTH)
    exp = am.run(reads, qc, o)
    assert exp[2]["pairs_overlap"] >= 5 and exp[2]["mate_failed"] >= 1
    files = write_pair_files(tmp_path, reads)
    rec = [[(b"@p%d" % i, s, q) for i, (s, q) in enumerate(reads[m::2])] for m in (0, 1)]
    clean = am.clean_fastq_pair(rec[0], rec[1], qc, o)
    for piece, per_piece in ((None, 41), (302 + 150, 1), (604 + 301, 2), (906, 3)):
        if piece is not None:
            monkeypatch.setenv("NP2_KCOUNT_TEST_PIECE", str(piece))
        same_as_model(reads, device(reads, qc, o), exp)
        outs = [str(tmp_path / f"c{per_piece}.{m}.fq") for m in (0, 1)]
        st = np2io.sradapt_files(files, np2io.SrQc(**qc), np2io.SrAdapt(**o), outs)
        assert st == [exp[2], exp[2]], per_piece
        assert (open(outs[0], "rb").read(), open(outs[1], "rb").read()) == clean
    monkeypatch.setenv("NP2_KCOUNT_TEST_PIECE", "301")  # a pair that fits no piece is refused, not split
    with pytest.raises(api.Np2Error) as e:
        np2io.sradapt_files(files, np2io.SrQc(**qc), np2io.SrAdapt(**o))
    assert e.value.code == -4 and "pair" in str(e.value) and "301" in str(e.value)


# ---- 4. counting through it -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen_files(tmp_path_factory):
    return write_pair_files(tmp_path_factory.mktemp("sradapt"), list(gen_reads()))


def test_counting_through_the_trimmer_equals_counting_the_clean_reads(gen_files, tmp_path):
    qc, o = sm.opts(), am.adopts(**BOTH)
    res, _, totals = model("gen", qc, o)
    clean = b"".join(s[a:b] + b"\n" for (s, _), (a, b, cls, _, _) in zip(gen_reads(), res) if cls == 0)
    exp = np2io.count_kmers(clean, KS, min_count=1)
    assert all(len(y.words) > 1000 for y in exp)
    same_yaks(np2io.count_kmers(gen_files, KS, min_count=1, qc=np2io.SrQc(**qc), ad=np2io.SrAdapt(**o)), exp)
    assert {k: v for k, v in np2io.sradapt_last_stats().items() if k != "kernel_ms"} == totals
    outs = [str(tmp_path / f"k{k}.yak") for k in KS]
    np2io.count_kmers_to_files(gen_files, KS, outs, min_count=1, qc=np2io.SrQc(**qc), ad=np2io.SrAdapt(**o))
    for out, y in zip(outs, exp):
        ref = str(tmp_path / f"ref{y.k}.yak")
        np2io.write_yak(ref, y)
        assert open(out, "rb").read() == open(ref, "rb").read()
    # without the adapter options the same files count as the quality filter alone counts them: ad=None is the *_qc call
    qc_only = np2io.count_kmers(sm.clean_stream(list(gen_reads()), qc), KS, min_count=1)
    same_yaks(np2io.count_kmers(gen_files, KS, min_count=1, qc=np2io.SrQc(**qc), ad=None), qc_only)
    assert len(qc_only[0].words) != len(exp[0].words)  # the option is not a no-op here
    L = np2io._bind()
    arr, n = np2io._paths(gen_files)
    kk = np.array(KS, np.uint32)
    ko = np2io.np2_kcount_opts_t(1, 0)
    via = [[str(tmp_path / f"{tag}{k}.yak").encode() for k in KS] for tag in ("qc", "ad")]
    q = np2io.SrQc(**qc).c()
    assert L.np2_kcount_files_to_dumps_qc(0, arr, n, kk.ctypes.data, 2, C.byref(ko), C.byref(q), (C.c_char_p * 2)(*via[0])) == 0
    assert L.np2_kcount_files_to_dumps_ad(0, arr, n, kk.ctypes.data, 2, C.byref(ko), C.byref(q), None, (C.c_char_p * 2)(*via[1])) == 0
    for a, b in zip(*via):
        assert open(a, "rb").read() == open(b, "rb").read()
    # resident tables
    pol = np2io.polisher_from_reads(gen_files, KS, min_count=1, qc=np2io.SrQc(**qc), ad=np2io.SrAdapt(**o))
    present = np.unique(stream_hashes(sm.streams(list(gen_reads())[:600])[0], KS[0]))  # of the raw reads: some survive, some do not
    hs = np.concatenate([present, np.random.default_rng(2).integers(0, 1 << 42, size=500, dtype=np.uint64)])
    from nextpolish2_amd import Polisher
    assert np.array_equal(pol.lookup_hashes(0, hs, 1), Polisher(list(exp)).lookup_hashes(0, hs, 1))


# ---- 5. files and the module ----------------------------------------------------------------------------------------------------
def test_files_in_step_and_the_module_report(gen_files, tmp_path):
    reads = list(gen_reads())
    qc, o = sm.opts(), am.adopts(**BOTH)
    totals = model("gen", qc, o)[2]
    rec = [[(b"@p%d" % i, s, q) for i, (s, q) in enumerate(reads[m::2])] for m in (0, 1)]
    clean = am.clean_fastq_pair(rec[0], rec[1], qc, o)
    rep, prefix = tmp_path / "ad.tsv", str(tmp_path / "clean")
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.srqc"] + gen_files + ["--sr_adapter", f"seq={am.ADAPTER1},seq2={am.ADAPTER2}",
                        "--report", str(rep), "--out_fq", prefix], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [x.split("\t") for x in rep.read_text().splitlines()]
    assert rows[0] == ["file"] + list(am.STAT_NAMES) and [x[0] for x in rows[1:]] == [",".join(gen_files), "total"]
    for row in rows[1:]:
        assert [int(x) for x in row[1:]] == [totals[k] for k in am.STAT_NAMES]
    got = [open(f"{prefix}.{m}.fq", "rb").read() for m in (0, 1)]
    assert (got[0], got[1]) == clean
    assert got[0].count(b"\n") == got[1].count(b"\n") > 4 * 500  # in step: as many records in both
    # files whose record counts differ
    short = tmp_path / "short.R2.fq"
    short.write_bytes(sm.fastq(reads[1::2][:700], b"p"))
    with pytest.raises(api.Np2Error) as e:
        np2io.sradapt_files([gen_files[0], str(short)], np2io.SrQc(**qc), np2io.SrAdapt(**o))
    assert e.value.code == E_ARG and gen_files[0] in str(e.value) and str(short) in str(e.value) and "record 701" in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        np2io.count_kmers([str(short), gen_files[1]], KS, qc=np2io.SrQc(**qc), ad=np2io.SrAdapt(**o))
    assert e.value.code == E_ARG and gen_files[1] in str(e.value) and str(short) in str(e.value) and "record 701" in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        np2io.sradapt_files(gen_files + [gen_files[0]], None, np2io.SrAdapt(pair=True))
    assert e.value.code == E_ARG and "odd" in str(e.value)


# ---- 6. the known answer ---------------------------------------------------------------------------------------------------------
def _fastq_reads(path):
    lines = gzip.open(path, "rb").read().split(b"\n")
    return [(lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def test_reference_pairs_known_answer(tmp_path):
    """the first 2 000 pairs of the reference's test reads (tests/golden/ref_pairs): the kernel's totals equal the core
    program's, and the figures of the README's row.  (The reference's two files are simulated apart: all but one pair have
    no overlap.)"""
    r1, r2 = (_fastq_reads(p) for p in REF_PAIRS)
    reads = [x for pair in zip(r1, r2) for x in pair]
    qc, o = sm.opts(), am.adopts()
    exe, case = str(tmp_path / "sradapt_core_test"), tmp_path / "case.txt"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "tools", "sradapt_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    case.write_bytes(am.text_case(reads, qc, o))
    lines = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=600).stdout.splitlines()
    core = dict(zip(am.STAT_NAMES, (int(x) for x in lines[-1].split()[1:])))
    st = np2io.sradapt_files(REF_PAIRS, np2io.SrQc(**qc), np2io.SrAdapt(**o))
    assert st[0] == st[1] == core
    assert {k: core[k] for k in ("pairs", "pairs_overlap", "trimmed_overlap", "adapter_bases", "pass")} == \
        dict(pairs=2000, pairs_overlap=1, trimmed_overlap=2, adapter_bases=50, **{"pass": 4000})
    got = device(reads, qc, o)
    assert [" ".join(str(x) for x in r) for r in got[0]] == lines[:-1]


# ---- 7. the command line --------------------------------------------------------------------------------------------------------
def _cli(args, yaks=()):
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", "-t", "5", "-L", "1000", BAM, ASM] + list(yaks) + ["-k", "2"] + args,
                       capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout, r.stderr.decode()


def test_cli_polishes_from_trimmed_pairs(tmp_path):
    sr = [x for f in REF_PAIRS for x in ("--sr", f)]
    with_ad, err = _cli(sr + ["--sr_qc", "--sr_adapter"])
    assert with_ad.startswith(b">")
    line = [x for x in err.splitlines() if x.startswith("[INFO] sr_adapter:")]
    assert len(line) == 1 and "pairs 2000, pairs_overlap 1," in line[0] and "adapter_bases 50" in line[0]
    # the tables are count.py's with the same options
    yaks = [str(tmp_path / f"k{k}.yak") for k in KS]
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.count"] + REF_PAIRS + ["-m", "2", "--sr_qc", "--sr_adapter"] +
                       [x for k, y in zip(KS, yaks) for x in ("-k", str(k), "-o", y)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "sr_adapter: reads 4000" in r.stderr, r.stderr[-3000:]
    from_yaks, _ = _cli([], yaks)
    assert from_yaks == with_ad
    # without --sr_adapter: the quality filter alone, as before
    qc_only, err = _cli(sr + ["--sr_qc"])
    assert "sr_adapter" not in err and "[INFO] sr_qc: reads 4000" in err
    clean = tmp_path / "model_cleaned.fq"
    clean.write_bytes(sm.clean_fastq([(b"@r%d" % i, s, q) for p in REF_PAIRS for i, (s, q) in enumerate(_fastq_reads(p))], sm.opts()))
    from_clean, _ = _cli(["--sr", str(clean)])
    assert qc_only == from_clean
