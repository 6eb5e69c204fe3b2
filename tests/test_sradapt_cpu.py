"""Short-read adapter trimming without a device: the rule's core (csrc/np2_sradapt_core.hpp) as a stand-alone host program
under the address and undefined-behaviour sanitizers against the plain-Python model of tests/sradapt_model.py, the coverage
the seeded generator gives that model, a plant-and-recover check of the model, and the option text of the command lines.
tests/test_gpu_sradapt.py compares the device against the same model."""
import functools
import os
import subprocess
import sys

import pytest

import sradapt_model as am
import srqc_model as sm
from nextpolish2_amd import cli, count, srqc
from nextpolish2_amd import io as np2io

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

# the model's defaults are the product's (checked where the module loads: every test here is about the product's rule)
_D = np2io.SrAdapt.parse("")
assert dict(pair=_D.pair, overlap=_D.overlap, diff=_D.diff, diffpct=_D.diffpct, seq=_D.seq, seq2=_D.seq2) == am.DEFAULTS

# (quality options, adapter options)
OPTION_SETS = {"defaults": (sm.opts(), am.adopts()),
               "D10": (sm.NEUTRAL, am.adopts(diff=10)),
               "by_sequence": (sm.opts(), am.adopts(pair=False, seq=am.ADAPTER1))}


@functools.lru_cache(maxsize=None)
def gen():
    return am.generate()


@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sradapt_core") / "sradapt_core_test")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "tools", "sradapt_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_core(exe, tmp_path, reads, qc, o):
    case = tmp_path / "case.txt"
    case.write_bytes(am.text_case(reads, qc, o))
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-300:], r.stderr[-3000:])  # (a sanitizer report goes to stderr)
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("totals ")
    return [tuple(int(x) for x in ln.split()) for ln in lines[:-1]], dict(zip(am.STAT_NAMES, (int(x) for x in lines[-1].split()[1:])))


# ---- 1. the core against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OPTION_SETS))
@pytest.mark.parametrize("which", ["generated", "edges"])
def test_core_program_equals_the_model(core_exe, tmp_path, which, name):
    qc, o = OPTION_SETS[name]
    reads = gen()[0] if which == "generated" else am.edge_pairs()
    res, _, totals = am.run(reads, qc, o)
    got, got_totals = run_core(core_exe, tmp_path, reads, qc, o)
    bad = [(i, g, e, len(reads[i][0])) for i, (g, e) in enumerate(zip(got, res)) if g != e]
    assert len(got) == len(res) and not bad, (len(bad), bad[:5])
    assert got_totals == totals


def test_core_program_refuses_bad_options(core_exe, tmp_path):
    for bad in (dict(overlap=0), dict(overlap=1025), dict(diff=1025), dict(diffpct=101), dict(seq="ACG"), dict(seq="A" * 65), dict(seq="ACGN"),
                dict(seq="acgt"), dict(seq2="ACGT"), dict(pair=False)):
        case = tmp_path / "bad.txt"
        case.write_bytes(am.text_case([], sm.opts(), am.adopts(**bad)))
        r = subprocess.run([core_exe, str(case)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("invalid "), (bad, r.stdout, r.stderr[-2000:])
        with pytest.raises(ValueError):
            np2io.SrAdapt(**bad)


def test_model_known_answers():
    """hand-computed, so that the model is pinned to the statement and not only to the core"""
    n, d = sm.NEUTRAL, am.adopts()
    ins = b"ACGTTGCAAGGCTTAACCGGATATCGCGAATTCCGGAAGT"  # 40 bases
    r1, r2 = am._good(ins + b"AGATCGGAAG"), am._good(am.revcomp(ins) + b"AGATCGGAAG")
    assert am.judge_pair(r1, r2, n, d) == ((0, 40, 0, 1, 40), (0, 40, 0, 1, 40))  # s = -10
    assert am.judge_pair(am._good(ins), am._good(am.revcomp(ins)), n, d) == ((0, 40, 0, 0, 40), (0, 40, 0, 0, 40))  # s = 0, nothing moves
    assert am.judge_pair(am._good(ins), am._good(am.revcomp(ins[5:])), n, d) == ((0, 40, 0, 0, 40), (0, 35, 0, 0, 40))  # s = 5, T = 40 = n1
    assert am.judge_pair(am._good(ins), am._good(am.revcomp(ins[:35])), n, d) == ((0, 35, 0, 1, 35), (0, 35, 0, 0, 35))  # s = 0, n1 > T
    assert am.judge_pair(am._good(ins[:29]), am._good(am.revcomp(ins[:29])), n, d)[0] == (0, 29, 0, 0, 0)  # shorter than O
    assert am.find_overlap(b"A" * 60, b"T" * 60, d) == 0 and am.find_overlap(b"AC" * 40, am.revcomp(b"CA" * 40), d) == 1
    assert am.find_adapter(b"TTTTTTAGATCG", "AGATCGGAAGAGC") == 6 and am.find_adapter(b"TTTTTTTTAGAT", "AGATCGGAAGAGC") == 8
    assert am.find_adapter(b"TTTTTTTTTAGA", "AGATCGGAAGAGC") is None and am.find_adapter(b"AGA", "AGAT") is None
    assert am.judge_single(am._good(b"ACGTAGATCGGAAGAGCTT"), n, am.adopts(pair=False, seq="AGATCGGAAGAGC")) == (0, 4, 0, 2, 0)
    assert am.judge_single(am._good(b"AGATCGGAAGAGCTT"), n, am.adopts(pair=False, seq="AGATCGGAAGAGC")) == (0, 0, 1, 2, 0)  # emptied: class 1
    # the pair rule
    short = am.judge_pair(am._good(b"ACGTACGTACGTACGTACGT"), am._good(ins * 3), sm.opts(), d)
    assert (short[0][2], short[1][2]) == (1, 4)
    res, masked, t = am.run([r1, r2], n, d)
    assert masked == ins + b"N" * 10 + b"\n" + am.revcomp(ins) + b"N" * 10 + b"\n"
    assert t == dict(zip(am.STAT_NAMES, (2, 2, 0, 0, 0, 100, 80, 0, 1, 1, 0, 2, 0, 20)))


# ---- 2. what the generator exercises --------------------------------------------------------------------------------------------
def test_generator_exercises_every_branch():
    """A condition on the inputs of the device tests, not a measurement: the model, under the recipe with pair mode and both
    adapter sequences, sees at least 50 of each."""
    reads, meta = gen()
    assert len(reads) == 8000 and len(meta) == 4000
    assert {m["insert"] for m in meta} >= set(am.special_inserts())
    assert {(m["m1"], m["m2"]) for m in meta} == set(am.UNEQUAL) | {(am.M, am.M)}
    g = am.guard(reads, sm.opts(), am.adopts(seq=am.ADAPTER1, seq2=am.ADAPTER2))
    print(g)
    assert all(v >= 50 for v in g.values()), g
    again, _ = am.generate()
    assert again == reads  # seeded


def test_planted_adapters_are_recovered():
    """error-free pairs whose insert is shorter than the reads: mate 1 keeps exactly the insert and no base of the adapter"""
    reads, meta = gen()
    n = 0
    for i, m in enumerate(meta):
        if m["clean"] and (m["m1"], m["m2"]) == (am.M, am.M) and 30 <= m["insert"] < am.M:
            r1, r2 = am.judge_pair(reads[2 * i], reads[2 * i + 1], sm.NEUTRAL, am.adopts())
            assert r1 == (0, m["insert"], 0, 1, m["insert"]) and r2 == (0, m["insert"], 0, 1, m["insert"]), (i, m["insert"], r1, r2)
            assert reads[2 * i][0][r1[0]:r1[1]] == m["frag"]
            n += 1
    assert n >= 50, n


# ---- 3. the option text ---------------------------------------------------------------------------------------------------------
def as_model(a):
    return dict(pair=a.pair, overlap=a.overlap, diff=a.diff, diffpct=a.diffpct, seq=a.seq, seq2=a.seq2)


def test_option_text():
    assert as_model(np2io.SrAdapt.parse("")) == as_model(np2io.SrAdapt.parse(None)) == am.DEFAULTS
    assert as_model(np2io.SrAdapt.parse("pair=0,seq=AGATCGGAAGAGC")) == am.adopts(pair=False, seq="AGATCGGAAGAGC")
    a = np2io.SrAdapt.parse("overlap=15, diff=10,diffpct=0,seq=ACGT,seq2=" + "T" * 64)
    assert as_model(a) == am.adopts(overlap=15, diff=10, diffpct=0, seq="ACGT", seq2="T" * 64)
    c = a.c()
    assert (c.flags, c.overlap_min, c.overlap_diff, c.overlap_diff_percent, c.adapter1, c.adapter2) == (1, 15, 10, 0, b"ACGT", b"T" * 64)
    assert np2io.SrAdapt(pair=False, seq="ACGT").c().flags == 0 and np2io.SrAdapt(pair=True).c().adapter1 is None
    assert repr(np2io.SrQc()) == "SrQc(front=5, tail=5, cut5=1, cut3=1, window=4, mean=20, n=0, q=20, u=40, len=15)"  # untouched
    for mod in (cli, count, srqc):
        h = mod.build_parser().format_help()
        assert "--sr_adapter [SPEC]" in h and "fastp binary is not claimed" in " ".join(h.split())
    a = count.parse_args(["a.fq", "b.fq", "--sr_adapter"])
    assert as_model(a.sr_adapter) == am.DEFAULTS and count.parse_args(["a.fq"]).sr_adapter is None
    assert count.parse_args(["a.fq", "--sr_adapter", "pair=0,seq=ACGT"]).sr_adapter.seq == "ACGT"


REJECTED = ["overlap=0", "overlap=1025", "diff=-1", "diff=1025", "diffpct=101", "pair=2", "seq=ACG", "seq=" + "A" * 65, "seq=ACGU", "seq=acgt",
            "seq2=ACGT", "pair=0", "bogus=1", "overlap", "overlap=", "overlap=x", "diff=1,diff=2", "seq="]


def test_option_rejections_end_in_the_parser(tmp_path):
    """children: exit 2 from argparse with the library never loaded, on a bad key, a bad adapter letter, an odd file count"""
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"@r1\nACGT\n+\nIIII\n")
    bam = os.path.join(HERE, "golden", "ref_bundle", "hifi.map.sort.bam")
    asm = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
    for spec in REJECTED:
        with pytest.raises(ValueError):
            np2io.SrAdapt.parse(spec)
        with pytest.raises(SystemExit) as e:
            srqc.build_parser().parse_args([str(fq), str(fq), "--sr_adapter", spec])
        assert e.value.code == 2
    mods = {"srqc": [sys.executable, "-m", "nextpolish2_amd.srqc"], "count": [sys.executable, "-m", "nextpolish2_amd.count", "-o", str(tmp_path / "never.yak")],
            "cli": [sys.executable, "-m", "nextpolish2_amd.cli", bam, asm]}
    for name, cmd in mods.items():
        one = ["--sr", str(fq)] if name == "cli" else [str(fq)]
        for args in (one + one + ["--sr_adapter", "bogus=1"], one + one + ["--sr_adapter", "seq=ACGU"], one + ["--sr_adapter"],
                     one * 3 + ["--sr_adapter", "overlap=20"]):
            r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=600, env=ENV)
            assert r.returncode == 2 and r.stdout == "" and "--sr_adapter" in r.stderr, (name, args, r.stderr[-500:])
    r = subprocess.run(mods["cli"] + [os.path.join(HERE, "golden", "ref_bundle", "k21.yak"), "--sr_adapter"], capture_output=True, text=True,
                       timeout=600, env=ENV)
    assert r.returncode == 2 and "--sr_adapter" in r.stderr and "--sr" in r.stderr and r.stdout == ""
    assert not (tmp_path / "never.yak").exists()


def test_report_text_with_the_new_columns():
    st = [dict(zip(am.STAT_NAMES, range(1, 15)))] * 2
    text = srqc.report_text(["a.fq,b.fq"], st, am.STAT_NAMES)
    assert text == ("file\t" + "\t".join(am.STAT_NAMES) + "\na.fq,b.fq\t" + "\t".join(str(i) for i in range(1, 15)) + "\ntotal\t" +
                    "\t".join(str(i) for i in range(1, 15)) + "\n")
    assert srqc.report_text(["a.fq"], [dict(zip(sm.STAT_NAMES, range(7)))] * 2).startswith("file\treads\tpass\ttoo_short\ttoo_many_n\tlow_quality\tbases_in\tbases_out\na.fq")


# ---- 4. the paired reader's record feed under the host sanitizers -------------------------------------------------------------------
SANITIZERS = {"thread": ["-fsanitize=thread"], "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def feed_exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("recordfeed") / f"recordfeed_test_{request.param}")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + SANITIZERS[request.param] +
                       ["-o", out, os.path.join(HERE, "tools", "recordfeed_test.cpp"), "-lz", "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _feed(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    return r.stdout


def test_record_feed_under_the_host_sanitizers(feed_exe, tmp_path):
    """two files in step over many batches (plain with CRLF and without a final newline against gzip in two members, empty
    reads included), a file that ends early, a consumer that leaves while the readers are blocked on a full queue, and a
    reader's error met where the consumer stands"""
    import gzip
    reads = gen()[0] * 3  # 12 000 records a file: six batches of 2 048, more than the queue of 4 holds
    recs = [[(b"@p%d/%d extra" % (i, m + 1), s, q) for i, (s, q) in enumerate(reads[m::2])] for m in (0, 1)]
    assert any(len(s) == 0 for _, s, _ in recs[0])

    def text(rs, nl=b"\n"):
        return b"".join(h + nl + s + nl + b"+" + nl + q + nl for h, s, q in rs)
    r1, r2 = tmp_path / "r1.fq", tmp_path / "r2.fq.gz"
    r1.write_bytes(text(recs[0], b"\r\n")[:-2])
    r2.write_bytes(gzip.compress(text(recs[1][:5000]), 1) + gzip.compress(text(recs[1][5000:]), 1))
    exp = b"".join(b"\t".join(a) + b"\n" + b"\t".join(b) + b"\n" for a, b in zip(*recs)) + b"end 12000 12000\n"
    assert _feed(feed_exe, "in_step", r1, r2) == exp
    short = tmp_path / "short.fq"
    short.write_bytes(text(recs[1][:2500]))
    out = _feed(feed_exe, "in_step", r1, short).splitlines()
    assert out[-1] == b"end 12000 2500" and len(out) == 14501
    assert _feed(feed_exe, "leave", r1, r2, 10) == b"left\n"
    assert _feed(feed_exe, "leave", r1, r2, 0) == b"left\n"
    bad = tmp_path / "bad.fq"
    bad.write_bytes(text(recs[1][:2100]) + b"@x\nACGT\n+\nIII\n" + text(recs[1][2101:]))
    out = _feed(feed_exe, "in_step", r1, bad).splitlines()
    assert out[-1].startswith(b"error -1 ") and b"bad.fq" in out[-1] and b"record 2101" in out[-1]
    out = _feed(feed_exe, "in_step", tmp_path / "missing.fq", r2).splitlines()
    assert out[-1].startswith(b"error -1 ") and b"cannot open" in out[-1]
