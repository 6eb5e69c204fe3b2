"""The short-read quality filter without a device: the rule's core (csrc/np2_srqc_core.hpp) as a stand-alone host program
under the address and undefined-behaviour sanitizers, the reader's quality stream (np2_seqfile_stream_qual) against a
Python parse, the option text of the command lines, and the coverage the seeded generator gives the model of
tests/srqc_model.py.  tests/test_gpu_srqc.py compares the device against that model."""
import gzip
import os
import subprocess
import sys

import pytest

import srqc_model as sm
from nextpolish2_amd import api, cli, count, srqc
from nextpolish2_amd import io as np2io

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
E_ARG = -1


# ---- 1. the core ----------------------------------------------------------------------------------------------------------------
def test_core_program_under_sanitizers(tmp_path):
    """judge_serial against a brute-force restatement: every option alone, W = 1 / 1000, M = 0, lengths 0, 1, W - 1, W, W + 1,
    trims that meet and cross, a single bad base at each of 12 positions, N next to either cut, nN / lowq / len at and one
    past their thresholds, 3 000 pseudo-random reads"""
    exe = str(tmp_path / "srqc_core_test")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "tools", "srqc_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stderr == ""  # (a sanitizer report goes there)


def test_model_agrees_with_the_core_programs_known_answers():
    """the same hand-computed answers the core program asserts, so that model and core are pinned to one statement"""
    G, B = b"I", b"#"
    s = bytearray(b"ACGTACGTAC" * 4)
    s[7], s[32], s[20] = ord("N"), ord("n"), ord("N")
    s, q = bytes(s), B * 7 + G * 26 + B * 7
    n = sm.NEUTRAL
    assert sm.judge(s, q, n) == (0, 40, 0)
    assert sm.judge(s, q, sm.opts(n, trim_front=5)) == (5, 40, 0) and sm.judge(s, q, sm.opts(n, trim_tail=5)) == (0, 35, 0)
    assert sm.judge(s, q, sm.opts(n, cut_front=True)) == (5, 40, 0) and sm.judge(s, q, sm.opts(n, cut_tail=True)) == (0, 35, 0)
    assert sm.judge(s, q, sm.opts(n, n_base_limit=2))[2] == 2 and sm.judge(s, q, sm.opts(n, n_base_limit=3))[2] == 0
    assert sm.judge(s, q, sm.opts(n, qualified_q=20, unqualified_percent=34))[2] == 3
    assert sm.judge(s, q, sm.opts(n, qualified_q=20, unqualified_percent=35))[2] == 0
    assert sm.judge(s, q, sm.opts(n, min_len=40))[2] == 0 and sm.judge(s, q, sm.opts(n, min_len=41))[2] == 1
    s2 = bytearray(b"ACGTACGTAC" * 4)
    s2[5] = s2[6] = s2[33] = ord("N")
    s2[34] = ord("n")
    assert sm.judge(bytes(s2), q, sm.opts()) == (7, 33, 0)
    assert sm.judge(b"N" * 40, G * 40, sm.opts(n, cut_front=True, cut_tail=True)) == (40, 40, 1)
    assert sm.judge(b"ACG", G * 3, sm.opts(n, cut_front=True, cut_mean_q=0)) == (3, 3, 1)  # no window fits, whatever M
    res, masked, t = sm.run([(bytes(s2), q), (b"ACGT", G * 4), (b"", b"")], sm.opts())
    assert masked == b"N" * 7 + bytes(s2[7:33]) + b"N" * 7 + b"\nNNNN\n\n"
    assert t == dict(zip(sm.STAT_NAMES, (3, 1, 2, 0, 0, 44, 26)))


# ---- 2. the reader --------------------------------------------------------------------------------------------------------------
RECORDS = [(b"@r1 first", b"ACGTN", b"IIII#"), (b"@r2", b"", b""), (b"@r3", b"ACGTACGTAC", b"@>IIIIIII+"), (b"@r4", b"GG", b">@"),
           (b"@r5", b"T", b"@")]


def fastq_text(recs, nl=b"\n", final=True, blank=False):
    t = (nl if blank else b"").join(h + nl + s + nl + b"+" + nl + q + nl for h, s, q in recs)
    return t if final else t[:-len(nl)]


def python_parse(recs):
    return b"".join(s + b"\n" for _, s, _ in recs), b"".join(q + b"\n" for _, _, q in recs)


@pytest.mark.parametrize("shape", ["plain", "crlf", "blank", "nofinal", "nofinal_crlf", "gzip2"])
def test_quality_stream_equals_a_python_parse(tmp_path, shape):
    """quality lines beginning with '@' and '>' are in RECORDS; an empty read keeps its place in both streams"""
    p = tmp_path / ("a.fq.gz" if shape == "gzip2" else "a.fq")
    if shape == "gzip2":  # two members
        p.write_bytes(gzip.compress(fastq_text(RECORDS[:2])) + gzip.compress(fastq_text(RECORDS[2:])))
    else:
        p.write_bytes(fastq_text(RECORDS, nl=b"\r\n" if "crlf" in shape else b"\n", final="nofinal" not in shape, blank=shape == "blank"))
    seq, qual = np2io.seqfile_stream_qual(p)
    assert (seq, qual) == python_parse(RECORDS)
    assert np2io.seqfile_stream(p) == seq  # ... and the reader without qualities gives what it always gave


def test_existing_reader_is_unchanged_on_other_formats(tmp_path):
    fa, ln = tmp_path / "a.fa", tmp_path / "a.txt"
    fa.write_bytes(b">x\nAC\nGT\n>y\n\n>z\nTT")
    ln.write_bytes(b"ACGT\r\n\r\nGG")
    assert np2io.seqfile_stream(fa) == b"ACGT\n\nTT\n"
    assert np2io.seqfile_stream(ln) == b"ACGT\n\nGG\n"
    names, ends = np2io.seqfile_reads(fa)
    assert names == ["x", "y", "z"] and ends.tolist() == [4, 5, 8]


def test_reader_errors_name_the_file_and_the_record(tmp_path):
    bad = tmp_path / "bad.fq"
    bad.write_bytes(fastq_text(RECORDS[:2]) + b"@r3\nACGT\n+\nIII\n" + fastq_text(RECORDS[3:]))
    with pytest.raises(api.Np2Error) as e:
        np2io.seqfile_stream_qual(bad)
    assert e.value.code == E_ARG and str(bad) in str(e.value) and "record 3" in str(e.value)
    long_q = tmp_path / "long.fq"
    long_q.write_bytes(b"@r1\nACGT\n+\nIIIII\n")
    with pytest.raises(api.Np2Error) as e:
        np2io.seqfile_stream_qual(long_q)
    assert e.value.code == E_ARG and "record 1" in str(e.value)
    cut = tmp_path / "cut.fq"
    cut.write_bytes(fastq_text(RECORDS[:1]) + b"@r2\nACGT\n")
    with pytest.raises(api.Np2Error) as e:
        np2io.seqfile_stream_qual(cut)
    assert e.value.code == E_ARG and "record 2" in str(e.value)
    for name, text in (("a.fa", b">x\nACGT\n"), ("a.txt", b"ACGT\nGGCC\n")):
        f = tmp_path / name
        f.write_bytes(text)
        with pytest.raises(api.Np2Error) as e:
            np2io.seqfile_stream_qual(f)
        assert e.value.code == E_ARG and str(f) in str(e.value) and "FASTQ" in str(e.value)
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    assert np2io.seqfile_stream_qual(empty) == (b"", b"")


# ---- 3. the option text ---------------------------------------------------------------------------------------------------------
def as_model(q):
    return {a: getattr(q, a) for a in sm.RECIPE}


def test_option_text_preset_and_overrides():
    assert as_model(np2io.SrQc.recipe()) == sm.RECIPE == as_model(np2io.SrQc.parse("")) == as_model(np2io.SrQc.parse(None))
    q = np2io.SrQc.parse("front=0,tail=0,mean=25")
    assert as_model(q) == sm.opts(trim_front=0, trim_tail=0, cut_mean_q=25)
    q = np2io.SrQc.parse("cut5=0, cut3=0,window=1000,n=4294967295,q=93,u=100,len=0,mean=0")
    assert as_model(q) == sm.opts(cut_front=False, cut_tail=False, cut_window=1000, n_base_limit=2 ** 32 - 1, qualified_q=93,
                                  unqualified_percent=100, min_len=0, cut_mean_q=0)
    c = q.c()
    assert (c.trim_front, c.trim_tail, c.cut_window, c.cut_mean_q, c.n_base_limit, c.qualified_q, c.unqualified_percent, c.min_len, c.flags) == \
        (5, 5, 1000, 0, 2 ** 32 - 1, 93, 100, 0, 0)
    assert np2io.SrQc().c().flags == 3 and np2io.SrQc(cut_tail=False).c().flags == 1
    a = count.build_parser().parse_args(["x.fq", "--sr_qc"])
    assert as_model(a.sr_qc) == sm.RECIPE and count.build_parser().parse_args(["x.fq"]).sr_qc is None
    a = count.build_parser().parse_args(["--sr_qc", "len=30", "x.fq"])
    assert a.sr_qc.min_len == 30 and a.reads == ["x.fq"]
    assert as_model(srqc.build_parser().parse_args(["x.fq"]).sr_qc) == sm.RECIPE
    assert srqc.build_parser().parse_args(["x.fq", "--sr_qc", "u=7"]).sr_qc.unqualified_percent == 7
    for mod in (cli, count, srqc):
        h = mod.build_parser().format_help()
        assert "--sr_qc [SPEC]" in h
    assert "paired files are not kept in step" in srqc.build_parser().format_help()


REJECTED = ["window=0", "window=1001", "mean=94", "q=94", "u=101", "front=-1", "tail=4294967296", "n=-1", "len=4294967296", "cut5=2", "cut3=-1",
            "bogus=1", "front", "front=", "front=x", "front=1,front=2", "mean=2.5"]


def test_option_text_rejections_end_in_the_parser(tmp_path):
    """run as children: exit 2 from argparse with the library never loaded (without a device a call that reached
    one would fail differently); also --sr_qc without --sr"""
    fq = tmp_path / "r.fq"
    fq.write_bytes(fastq_text(RECORDS))
    bam = os.path.join(HERE, "golden", "ref_bundle", "hifi.map.sort.bam")
    asm = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
    mods = {"srqc": [sys.executable, "-m", "nextpolish2_amd.srqc", str(fq)],
            "count": [sys.executable, "-m", "nextpolish2_amd.count", str(fq), "-o", str(tmp_path / "never.yak")],
            "cli": [sys.executable, "-m", "nextpolish2_amd.cli", bam, asm, "--sr", str(fq)]}
    for spec in REJECTED:
        with pytest.raises(ValueError):
            np2io.SrQc.parse(spec)
        with pytest.raises(SystemExit) as e:
            srqc.build_parser().parse_args([str(fq), "--sr_qc", spec])
        assert e.value.code == 2
    for name, cmd in mods.items():  # every rejection through one module each in turn, all of them through the first
        for spec in (REJECTED if name == "srqc" else REJECTED[:2] + REJECTED[-6:-4]):
            r = subprocess.run(cmd + ["--sr_qc", spec], capture_output=True, text=True, timeout=600, env=ENV)
            assert r.returncode == 2 and r.stdout == "" and "--sr_qc" in r.stderr, (name, spec, r.stderr[-500:])
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", bam, asm, os.path.join(HERE, "golden", "ref_bundle", "k21.yak"), "--sr_qc"],
                       capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 2 and "--sr_qc" in r.stderr and "--sr" in r.stderr and r.stdout == ""
    assert not (tmp_path / "never.yak").exists()
    # the srqc module refuses to overwrite
    rep = tmp_path / "qc.tsv"
    rep.write_text("keep me\n")
    r = subprocess.run(mods["srqc"] + ["--report", str(rep)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode != 0 and "already exists" in r.stderr and rep.read_text() == "keep me\n"
    (tmp_path / "out.0.fq").write_text("keep me\n")
    with pytest.raises(SystemExit) as e:
        srqc.parse_args([str(fq), "--out_fq", str(tmp_path / "out")])
    assert "already exists" in str(e.value)


def test_report_text():
    st = [dict(zip(sm.STAT_NAMES, range(1, 8))), dict(zip(sm.STAT_NAMES, range(1, 8)))]
    assert srqc.report_text(["a.fq"], st) == ("file\treads\tpass\ttoo_short\ttoo_many_n\tlow_quality\tbases_in\tbases_out\n"
                                              "a.fq\t1\t2\t3\t4\t5\t6\t7\ntotal\t1\t2\t3\t4\t5\t6\t7\n")


# ---- 4. the coverage guard ------------------------------------------------------------------------------------------------------
def test_generator_exercises_every_branch():
    """A condition on the inputs of the device tests, not a measurement.  Read i is judged under the recipe with
    n_base_limit = (0, 1, 5)[i % 3] (srqc_model.mixture): the three limits in one mixture."""
    reads = sm.generate()
    assert len(reads) == 5000
    assert {len(s) for s, _ in reads} >= set(sm.LENGTHS)
    classes, cut_front, cut_tail, emptied = sm.guard(reads)
    print("classes", classes, "cut front", cut_front, "cut tail", cut_tail, "emptied", emptied)
    assert sum(classes) == 5000  # no read is left out
    assert all(c >= 100 for c in classes), classes
    assert cut_front >= 100 and cut_tail >= 100 and emptied >= 100
    assert sm.generate() == reads  # seeded
