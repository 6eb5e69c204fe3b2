"""The SAM reader on the device (np2_sam.hip, np2_sam_host.cpp) against the plain-Python model of its rule (tests/sam_model.py):
the parsed and sorted arrays, the error lines, the pileups a resident SAM gives, and the command line on SAM input against the
same run on the BAM of the same records, and against the committed answer of the reference bundle."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import sam_cases as sc
import sam_model as sm
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.bamio import pileup_to_records, read_bam, records_to_arrays, write_bam, write_sam
from nextpolish2_amd.synth import Synth
from oracle import np2_oracle as orc
from test_frontend_cpu import same_pileup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNDLE = os.path.join(ROOT, "tests", "golden", "ref_bundle")
ASM = os.path.join(ROOT, "tests", "golden", "ref_test_asm.fa.gz")
E_ARG = -1


def assert_arrays(got, want, what):
    names = ("recs", "tids", "cigar", "seq4")
    for g, w, n in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n, g.shape, w.shape)
        assert np.array_equal(g, w), (what, n, np.flatnonzero(g != w)[:5] if g.shape else None)


def check_text(text, tie):
    m = sm.model(text, tie)
    *arrays, stats = np2io.sam_parse_bytes(text, tie=tie)
    assert {k: stats[k] for k in m.stats} == m.stats, (stats, m.stats)
    assert_arrays(arrays, m.arrays(), tie)
    return m, stats


@pytest.fixture(scope="module")
def gen_text():
    return sc.generated(seed=7, n=400)


# ---- 1. sam_parse_bytes against the model, array for array -----------------------------------------------------------------------
@pytest.mark.parametrize("crlf,final_newline,empty_lines", [(False, True, False), (True, False, True), (False, False, False)])
def test_hand_cases(crlf, final_newline, empty_lines):
    for tie in ("strand", "input"):
        check_text(sc.good_text(crlf, final_newline, empty_lines), tie)
    m, _ = check_text(sc.TIE_TEXT, "strand")
    assert m.order == [1, 0, 2]
    check_text(sc.TIE_TEXT, "input")
    for text in (b"", sc.HEADER, sc.HEADER + sc.GOOD["flag_max"][0]):  # nothing to keep
        check_text(text, "strand")


@pytest.mark.parametrize("tie", ["strand", "input"])
def test_generated_records(gen_text, tie):
    m, _ = check_text(gen_text, tie)
    assert m.stats["kept"] > 200 and m.stats["unmapped"] > 50


def test_generated_records_in_many_pieces(gen_text, monkeypatch):
    monkeypatch.setenv("NP2_SAM_TEST_PIECE", "4096")  # records, CIGAR offsets and SEQ offsets carry across some 70 pieces
    assert max(len(ln) for ln in gen_text.split(b"\n")) < 4000 and len(gen_text) > 60 * 4096
    check_text(gen_text, "strand")
    monkeypatch.setenv("NP2_SAM_TEST_PIECE", "1000")
    with pytest.raises(Np2Error, match="does not fit a piece") as e:
        np2io.sam_parse_bytes(gen_text)
    assert e.value.code == -4
    monkeypatch.delenv("NP2_SAM_TEST_PIECE")
    check_text(gen_text, "input")  # the process stays usable


def test_two_gzip_files_through_sam_open(gen_text, tmp_path):
    lines = gen_text.split(b"\n")[:-1]
    head, body = [ln for ln in lines if ln.startswith(b"@")], [ln for ln in lines if not ln.startswith(b"@")]
    half = len(body) // 2
    texts = [b"\n".join(head + body[half:]) + b"\n", b"\n".join(head + body[:half])]  # (the second one without a last newline)
    paths = [str(tmp_path / "a.sam.gz"), str(tmp_path / "b.gz")]
    for p, t in zip(paths, texts):
        with gzip.open(p, "wb") as f:
            f.write(t)
    pol = Polisher([])
    for tie in ("strand", "input"):
        m = sm.model(texts, tie)  # records equal in the key: file order, files in argument order
        sam = np2io.Sam(pol, paths, tie=tie)
        assert sam.refs() == sc.REFS == m.refs
        st = sam.stats()
        assert {k: st[k] for k in m.stats} == m.stats
        assert_arrays(sam.export(pol), m.arrays(), tie)
        sam.close()
    swapped = sm.model(texts[::-1], "input").arrays()
    assert not np.array_equal(swapped[0], m.arrays()[0])  # the order across files is part of the result
    with gzip.open(paths[1], "wb") as f:
        f.write(texts[1].replace(b"LN:30000", b"LN:30001"))
    with pytest.raises(Np2Error, match="@SQ") as e:
        np2io.Sam(pol, paths)
    assert e.value.code == E_ARG
    pol.close()


# ---- 2. error lines ------------------------------------------------------------------------------------------------------------
def test_malformed_lines_name_their_line_and_leave_the_process_usable(gen_text):
    good = sc.GOOD["pos_zero"][0]
    for name, (ln, why) in sc.BAD.items():
        text = sc.HEADER + good + b"\n\n" + ln + b"\n" + good + b"\n"
        with pytest.raises(sm.SamError) as me:
            sm.model(text)
        with pytest.raises(Np2Error, match=r"line 7\b") as e:
            np2io.sam_parse_bytes(text)
        assert e.value.code == E_ARG == me.value.code and me.value.line == 7, name
        check_text(sc.good_text(), "strand")  # a following good call
    # two bad lines: the first in input order speaks, whatever the other one is
    body = gen_text.split(b"\n")
    n_head = sum(1 for ln in body if ln.startswith(b"@"))
    body[n_head + 300] = sc.line(rname=b"chrA", flag=b"1x")
    body[n_head + 20] = sc.line(rname=b"chrA", cigar=b"12M3")
    with pytest.raises(Np2Error, match=rf"line {n_head + 21}\b.*CIGAR") as e:
        np2io.sam_parse_bytes(b"\n".join(body))
    assert e.value.code == E_ARG
    for bad in (b"@SQ\tSN:c1\n", b"@SQ\tSN:c1\tLN:5\n@SQ\tSN:c1\tLN:6\n"):
        with pytest.raises(Np2Error, match=rf"line {1 + bad.count(bytes([10]))}\b") as e:
            np2io.sam_parse_bytes(b"@HD\tVN:1.6\n" + bad + good + b"\n")
        assert e.value.code == E_ARG
    check_text(gen_text, "strand")


def test_first_bad_line_speaks_across_pieces(gen_text, monkeypatch):
    monkeypatch.setenv("NP2_SAM_TEST_PIECE", "4096")
    body = gen_text.split(b"\n")
    n_head = sum(1 for ln in body if ln.startswith(b"@"))
    body[n_head + 350] = sc.BAD["ten_fields"][0]
    body[n_head + 100] = sc.BAD["unknown_rname"][0]
    with pytest.raises(Np2Error, match=rf"line {n_head + 101}\b.*RNAME") as e:
        np2io.sam_parse_bytes(b"\n".join(body))
    assert e.value.code == E_ARG


# ---- 3. pileup parity ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_refs():
    s1 = Synth(30000, depth=20, seed=71, diploid=True, read_len_mean=5000.0, name="ctgA")
    s2 = Synth(20000, depth=15, seed=72, name="ctgB")
    recs = pileup_to_records(s1.pileup, tid=0, rng=np.random.default_rng(5), decorate=True) + \
        pileup_to_records(s2.pileup, tid=1, rng=np.random.default_rng(6), decorate=True)
    refs = [("ctgA", s1.pileup.L), ("ctgB", s2.pileup.L)]
    shuffled = [recs[k] for k in np.random.default_rng(8).permutation(len(recs))]
    for i, r in enumerate(shuffled):
        r["name"] = b"read%d" % i
    return (s1, s2), refs, shuffled


def shuffled_text(refs, shuffled, tmp_path, gz=False):
    p = str(tmp_path / ("shuffled.sam.gz" if gz else "shuffled.sam"))
    write_sam(p, refs, shuffled, gz=gz)
    return p, (gzip.open(p, "rb") if gz else open(p, "rb")).read()


@pytest.mark.parametrize("fopts", [None, dict(use_supplementary=True, min_map_qual=0, min_read_len=2000, max_clip_len=10)])
def test_pileup_from_sam_equals_the_pileup_from_the_sorted_records(two_refs, tmp_path, fopts):
    synths, refs, shuffled = two_refs
    path, text = shuffled_text(refs, shuffled, tmp_path)
    m = sm.model(text)  # the model sorts
    fo = np2io.FrontOpts(**fopts) if fopts else np2io.FrontOpts()
    pol = Polisher([])
    sam = np2io.Sam(pol, [path])
    assert sam.refs() == refs
    for tid, s in enumerate(synths):
        ref = s.pileup.ref
        rr = [r for r in m.records if r["tid"] == tid]
        assert len(rr) > 20
        arr, cig, seq4, asc, asc_off = records_to_arrays(rr)
        got = np2io.export_contig(pol, np2io.contig_from_sam(pol, sam, refs[tid][0], ref.tobytes(), fo), ref)
        assert same_pileup(got, np2io.export_contig(pol, np2io.contig_from_records(pol, ref.tobytes(), arr, cig, seq4, fo), ref))
        assert same_pileup(got, orc.front_end(ref.tobytes(), arr, cig, asc, asc_off, fo))
    with pytest.raises(Np2Error, match="@SQ") as e:
        np2io.contig_from_sam(pol, sam, "ctgC", synths[0].pileup.ref.tobytes(), fo)
    assert e.value.code == E_ARG
    with pytest.raises(Np2Error, match="BAM") as e:
        np2io.contig_from_sam(pol, sam, "ctgA", synths[0].pileup.ref.tobytes(), np2io.FrontOpts(use_secondary=True))
    assert e.value.code == -4
    sam.close()
    pol.close()


# ---- 4. the command line on the synthetic assembly -------------------------------------------------------------------------------
def run_cli(args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli"] + args, capture_output=True, env=env, timeout=600, **kw)


def test_cli_on_sam_writes_what_it_writes_on_the_bam_of_the_sorted_records(two_refs, tmp_path):
    from test_oracle import yak_from_seqs
    synths, refs, shuffled = two_refs
    sam_gz, text = shuffled_text(refs, shuffled, tmp_path, gz=True)
    m = sm.model(text)
    write_bam(str(tmp_path / "m.bam"), refs, m.records)
    with gzip.open(tmp_path / "g.fa.gz", "wt") as f:
        for (nm, _), s in zip(refs, synths):
            f.write(f">{nm}\n{s.pileup.ref.tobytes().decode()}\n")
        f.write(">tiny\nACGTACGTNNacgt\n")
    haps = [synths[0].hap1.decode(), synths[0].hap2.decode(), synths[1].hap1.decode()]
    np2io.write_yak(str(tmp_path / "k21.yak"), yak_from_seqs(haps, 21))
    np2io.write_yak(str(tmp_path / "k31.yak"), yak_from_seqs(haps, 31))
    rest = [str(tmp_path / "g.fa.gz"), str(tmp_path / "k21.yak"), str(tmp_path / "k31.yak")]
    r = run_cli(["-L", "10000", str(tmp_path / "m.bam")] + rest)
    assert r.returncode == 0, r.stderr.decode()
    want = r.stdout
    assert want.count(b">") == 3 and b">ctgA start:" in want
    r = run_cli(["-L", "10000", sam_gz] + rest)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want
    r = run_cli(["-t", "3", "-L", "10000", sam_gz] + rest)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want
    # SAM text on standard input, fed by a child process started fresh
    feeder = subprocess.Popen([sys.executable, "-c", "import sys; sys.stdout.buffer.write(open(sys.argv[1], 'rb').read())", sam_gz],
                              stdout=subprocess.PIPE)
    r = run_cli(["-L", "10000", "-"] + rest, stdin=feeder.stdout)
    feeder.stdout.close()
    assert feeder.wait(timeout=60) == 0
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want


# ---- 5. a known answer that does not rest on the code under test -------------------------------------------------------------------
def test_reference_bundle_from_sam(tmp_path):
    refs, recs = read_bam(os.path.join(BUNDLE, "hifi.map.sort.bam"))
    assert len(recs) == 574 and max(len(r["cigar"]) for r in recs) == 937
    sam = str(tmp_path / "bundle.sam")
    write_sam(sam, refs, recs)  # in file order
    text = open(sam, "rb").read()
    assert len(text) > 7_000_000  # (QUAL is written as *)
    rest = ["-L", "1000", sam, ASM, os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")]
    r = run_cli(["--sam_tie", "input"] + rest)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == gzip.open(os.path.join(BUNDLE, "expected.fa.gz"), "rb").read()
    # the samtools order differs in 17 places of the file: the run succeeds, its records are in the model's order
    r = run_cli(["--sam_tie", "strand"] + rest)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.startswith(b">") and r.stdout.count(b"\n") == 2
    m = sm.model(text, "strand")
    assert m.order != list(range(574))
    assert_arrays(np2io.sam_parse_bytes(text, tie="strand")[:4], m.arrays(), "bundle")
