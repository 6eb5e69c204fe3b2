"""The full BAM on the device (NP2_SAM_KEEP_ALL: k_sam_tail_len, k_sam_tail_emit, k_bam_emit with tails; io.Sam(keep_all=True),
samsort --full, cli --sorted_bam_full) against the host walk of the same rule (np2_sam_tails_host), the encoder's host twin
and the plain-Python model (tests/bamfull_model.py), byte for byte; the written file through the project's own readers; and
the path on recycled, poisoned memory."""
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bamfull_model as fm
import bamout_model as bm
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.bamio import pileup_to_records
from nextpolish2_amd.synth import Synth
from test_frontend_cpu import same_pileup
from test_gpu_dirty_memory import POISON  # the bytes that scheme fills recycled blocks with

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_UNSUPPORTED = -1, -2, -4
REFS = bm.REFS


def device_error(e, what):
    """nothing more may run on a device that has reported an error: the session ends here"""
    pytest.exit(f"device error in {what}: {e}", returncode=3)


@pytest.fixture(scope="module")
def pol():
    p = Polisher([])
    yield p
    p.close()


def rec(pos, l_seq=8, **kw):
    r = bm.rec(kw.pop("tid", 0), pos, [("M", l_seq)] if l_seq else [], l_seq=l_seq, name=kw.pop("name", b"q%d" % pos), seed=pos)
    r.update(kw)
    return r


def accepted_records():
    """the accepted cases of test_bamfull_cpu.py, one record each, in an order that is not the sorted one"""
    rng = random.Random(7)
    cases = [dict(tags=[b"XA:A:!", b"NM:i:-7", b"de:f:0.0012", b"MD:Z:10A5^AC6", b"XH:H:1AE301", b"XB:B:c,-1,2", b"ZB:B:f,1.5,-2e3", b"Z9:Z:"])]
    cases += [dict(tags=[b"XI:i:%d" % v]) for v in (-2 ** 31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2 ** 32 - 1)]
    cases += [dict(tags=[b"XF:f:" + t for t in (b"0.0012", b"1", b"-3.5E+2", b"1e-5", b"0.1", b"16777217", b"9007199254740991", b"1e22", b"1e-22")])]
    decimals = []
    while len(decimals) < 200:
        digits = "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 16)))
        cut = rng.randint(1, len(digits))
        frac = len(digits) - cut
        if int(digits) < 2 ** 53:
            ex = rng.randint(-22 + frac, 22 + frac)
            decimals.append((rng.choice(["", "-"]) + digits[:cut] + ("." + digits[cut:] if frac else "") + "e%d" % ex).encode())
    cases += [dict(tags=[b"X%d:f:" % (j % 10) + t for j, t in enumerate(decimals[k:k + 40])]) for k in range(0, 200, 40)]
    for sub, vals in (("c", [-128, 127]), ("C", [0, 255]), ("s", [-32768, 32767]), ("S", [0, 65535]), ("i", [-2 ** 31, 2 ** 31 - 1]),
                      ("I", [0, 2 ** 32 - 1]), ("f", ["0.5", "-1e3"])):
        text = lambda v: b"XB:B:" + sub.encode() + b"".join(b",%s" % str(x).encode() for x in v)
        cases += [dict(tags=[text([]), text(vals[:1]), text(vals * 40)])]
    cases += [dict(tags=[b"NM:i:1", b"XZ:Z:" + bytes(32 + (i * 7) % 95 for i in range(n)), b"XT:A:x"]) for n in (0, 1, 63, 64, 65, 255, 256, 5000)]
    cases += [dict(tags=[b"XH:H:" + bytes(b"0123456789abcdefABCDEF"[(i * 5) % 22] for i in range(n))]) for n in (0, 2, 64, 66, 200)]
    cases += [dict(tags=[b"%s%d:i:%d" % (b"XYZ"[j % 3:j % 3 + 1], j % 10, j * 311 - 20000) for j in range(n)]) for n in (1, 64, 65, 130)]
    for l_seq in (1, 2, 63, 64, 65, 15001):
        q = fm.qual_of(l_seq, l_seq)
        cases += [dict(l_seq=l_seq, qual=q), dict(l_seq=l_seq), dict(l_seq=l_seq, qual=q, tags=[b"NM:i:1"])]
    cases += [dict(l_seq=15001, qual=fm.qual_of(15001, k), tags=[b"MD:Z:" + b"".join(b"%dA" % (j % 40 + k) for j in range(900))]) for k in (1, 2, 3)]
    cases += [dict(l_seq=0), dict(l_seq=0, tags=[b"NM:i:0"])]
    cases += [dict(rnext=b"=", pnext=1, tlen=-1), dict(rnext=b"c2", pnext=2 ** 31 - 1, tlen=-(2 ** 31 - 1)), dict(rnext=b"c1", pnext=12, tlen=2 ** 31 - 1),
              dict(tid=1, rnext=b"=", tlen=b"+17"), dict(tid=2, rnext=b"c3", flag=16)]
    recs = [rec(10 + 3 * i, **c) for i, c in enumerate(cases)]
    rng.shuffle(recs)
    return recs


EXTRA = [b"@RG\tID:a\tSM:s", b"@PG\tID:minimap2\tPN:minimap2", b"@CO\tfree text", b"@RG\tID:a\tSM:s"]


def write_text(path, refs, recs, **kw):
    with open(path, "wb") as f:
        f.write(fm.sam_text(refs, recs, **kw))
    return str(path)


def device_full(pol, paths, tie="strand", out=None):
    """-> (stream, tails, tail_ref, header text, (bam, bai, stats) when `out`) of SAM files through io.Sam(keep_all=True)"""
    try:
        sam = np2io.Sam(pol, paths, tie=tie, keep_all=True)
        try:
            S = sam.bam_stream(pol)
            tails, tail_ref = sam.export_tails(pol)
            text = sam.header_text()
            files = None
            if out:
                st = sam.write_bam(pol, out)
                files = (open(out, "rb").read(), open(out + ".bai", "rb").read(), st)
            arrays = sam.export(pol) + sam.export_names(pol)
        finally:
            sam.close()
    except Np2Error as e:
        if e.code == E_DEVICE:
            device_error(e, "the full BAM")
        raise
    return S, tails, tail_ref, text, files, arrays


def sorted_order(given, tie="strand"):
    return sorted(range(len(given)), key=lambda i: (given[i]["tid"], given[i]["pos"] + 1, (given[i].get("flag", 0) >> 4) & 1 if tie == "strand" else 0))


# ---- 1. the CPU cases through the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece,batch", [(None, None), (32768, 1), (32768, 2)])
def test_accepted_cases_equal_the_host_walk_the_twin_and_the_model(pol, tmp_path, monkeypatch, piece, batch):
    given = accepted_records()
    text = fm.sam_text(REFS, given, extra=EXTRA)
    if piece is not None:  # the text falls into pieces, the stream into batches of `batch` blocks
        assert len(text) > 2 * piece  # (pieces end at a line's end: three or more)
        monkeypatch.setenv("NP2_SAM_TEST_PIECE", str(piece))
        monkeypatch.setenv("NP2_BGZF_TEST_BATCH", str(batch))
    path = str(tmp_path / "in.sam")
    open(path, "wb").write(text)
    S, tails, tail_ref, header, (bam, bai, st), arrays = device_full(pol, [path], out=str(tmp_path / "dev.bam"))
    order = sorted_order(given)
    want = [given[i] for i in order]
    host = np2io.sam_tails_host(text)
    assert host["code"] == 0 and len(host["status"]) == len(given)
    assert tails.tobytes() == host["tails"].tobytes()  # every line is kept: the tails lie as the lines were met
    assert list(tail_ref) == [int(host["tail_ref"][i]) for i in order]
    extras = [EXTRA]
    assert header == host["header_text"] == fm.header_text(REFS, extras)
    model_S, _ = fm.stream(REFS, want, extras)
    assert S == model_S, (len(S), len(model_S), next((i for i, (a, b) in enumerate(zip(S, model_S)) if a != b), None))
    twin_S, twin_st = np2io.bamout_host(*arrays, REFS, path=str(tmp_path / "twin.bam"), tails=tails, tail_ref=tail_ref, header_text=header)
    assert twin_S == S and bam == open(tmp_path / "twin.bam", "rb").read() and bai == open(tmp_path / "twin.bam.bai", "rb").read()
    assert bam == np2io.bgzf_deflate_host(model_S)
    fm.check_files(REFS, want, bam, bai, extras)
    assert st["records"] == len(want) and st["stream_bytes"] == len(S) and st["blocks"] >= 3


def refusals():
    """(record, status, what the message says) of the refused cases of test_bamfull_cpu.py"""
    t = lambda *tags, **kw: dict(tags=list(tags), **kw)
    out = [(t(b"XI:i:" + x), E_ARG, "(XI)") for x in (b"4294967296", b"-2147483649", b"+", b"1x")]
    out += [(t(b"XF:f:" + x), E_UNSUPPORTED, "(XF)") for x in (b"nan", b"inf", b"9007199254740993", b"1e23", b"1e-23")]
    out += [(t(b"XF:f:1e"), E_ARG, "(XF)"), (t(b"XB:B:c,1,128"), E_ARG, "(XB)"), (t(b"XB:B:f,1,1e23"), E_UNSUPPORTED, "(XB)"),
            (t(b"XB:B:x,1"), E_ARG, "(XB)"), (t(b"XH:H:abc"), E_ARG, "(XH)"), (t(b"XH:H:" + b"ab" * 50 + b"0g"), E_ARG, "(XH)"),
            (t(b"XZ:Z:a\x7fb"), E_ARG, "(XZ)"), (t(b"NM:i:1", b"XZ:Z:" + b"a" * 300 + b"\x1f" + b"a" * 99), E_ARG, "optional field 2 (XZ)"),
            (t(b"NM:i"), E_ARG, "optional field 1:"), (t(b"N_:i:1"), E_ARG, "optional field 1:"), (t(b"NM:q:1"), E_ARG, "(NM)"),
            (t(b"XA:A:ab"), E_ARG, "(XA)"), (t(*([b"NM:i:1"] * 70 + [b"XX:i:z"])), E_ARG, "optional field 71 (XX)"),
            (t(*([b"NM:i:1"] * 64 + [b"XX:i:z"] + [b"NM:i:1"] * 70)), E_ARG, "optional field 65 (XX)")]
    for l_seq in (1, 64, 65, 15001):
        q = fm.qual_of(l_seq, 1)
        out += [(dict(l_seq=l_seq, qual=q[:-1]), E_ARG, "QUAL"), (dict(l_seq=l_seq, qual=q + b"I"), E_ARG, "QUAL"),
                (dict(l_seq=l_seq, qual=q[:-1] + b" "), E_ARG, "QUAL"), (dict(l_seq=l_seq, qual=b"\x7f" + q[1:]), E_ARG, "QUAL")]
    out += [(dict(l_seq=0, qual=b"II"), E_ARG, "QUAL"), (dict(rnext=b"nope"), E_ARG, "RNEXT"), (dict(pnext=2 ** 31), E_ARG, "PNEXT"),
            (dict(tlen=2 ** 31), E_ARG, "TLEN"), (dict(pnext=b"x", tags=[b"XX:i:z"], qual=b"short"), E_ARG, "PNEXT")]
    return out


def test_refusals_come_with_their_code_and_line(pol, tmp_path):
    good = [rec(5), rec(6, tags=[b"NM:i:3"], qual=fm.qual_of(8))]
    for k, (case, status, says) in enumerate(refusals()):
        recs = good + [rec(9 + k, **case), rec(900, tags=[b"XF:f:nan"])]  # (a later bad line does not speak)
        path = write_text(tmp_path / ("bad%d.sam" % k), REFS, recs)
        with pytest.raises(Np2Error) as e:
            np2io.Sam(pol, [path], keep_all=True)
        if e.value.code == E_DEVICE:
            device_error(e.value, "a refusal")
        assert e.value.code == status and "line 7: " in str(e.value) and says in str(e.value), (k, str(e.value))
        host = np2io.sam_tails_host(fm.sam_text(REFS, recs))
        assert host["code"] == status and str(e.value).endswith(host["message"].split(": line ", 1)[1])
    # two bad lines in different pieces, a bad name before a bad tail, and an error of the lean parse behind both
    recs = good + [rec(20 + i) for i in range(40)]
    recs[30]["tags"], recs[12]["name"], recs[35]["flag"] = [b"XX:i:z"], b"n" * 255, 70000
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("NP2_SAM_TEST_PIECE", "512")
        with pytest.raises(Np2Error, match="line 17: QNAME"):
            np2io.Sam(pol, [write_text(tmp_path / "two.sam", REFS, recs)], keep_all=True)
    with pytest.raises(Np2Error, match="line 40: FLAG"):  # one piece: what the lean parse refuses speaks first
        np2io.Sam(pol, [write_text(tmp_path / "two.sam", REFS, recs)], keep_all=True)
    # the handle is usable afterwards, and an unmapped record's tail is not looked at
    recs = good + [rec(7, flag=4, tags=[b"bad"], qual=b"x")]
    S = device_full(pol, [write_text(tmp_path / "ok.sam", REFS, recs)])[0]
    assert S == fm.stream(REFS, good)[0]


# ---- 2. the cuts ----------------------------------------------------------------------------------------------------------------
TARGET_TAGS = [b"NM:i:5", b"XB:B:S,1,2,3", b"XZ:Z:abc"]
# in the target: the mate words are bytes 24 .. 35, the qualities 277 .. 476, NM 477 .. 480, XB's count word 485 .. 488, the last
# optional field's last byte 501, the end 502
CUT_PLACES = (30, 277, 278, 476, 477, 487, 501, 502)


def case_full_cuts():
    """block edge k falls `inside` the k-th target: in its mate words, in front of and behind its first and its last quality
    byte, in a B array's count word, in front of its last optional byte and exactly at its end"""
    recs, pos = [], 10
    for k, inside in enumerate(CUT_PLACES, start=1):
        at = len(fm.header(REFS, [EXTRA])) + sum(fm.size_of(r) for r in recs)
        target = bm.BLOCK * k - inside
        while at < target:
            left = target - at
            take = left if left <= 50000 else min(40000, left - 100)
            recs.append(bm.filler(0, pos, take, seed=pos))
            at, pos = at + take, pos + 1
        assert at == target
        r = bm.rec(0, pos, [("M", 5), ("I", 1)] * 14 + [("M", 5), ("S", 111)], name=b"target_%013d" % k, seed=k)
        r.update(qual=fm.qual_of(200, k), tags=TARGET_TAGS, rnext=b"=", pnext=1000 + k, tlen=-77 - k)
        assert fm.size_of(r) == 502
        recs.append(r)
        pos += 1
    recs.append(bm.filler(0, pos, 100, seed=pos))  # (the last edge lies between two records)
    return recs


@pytest.mark.parametrize("batch", [None, 1])
def test_cuts_through_mates_qualities_and_optional_fields(pol, tmp_path, monkeypatch, batch):
    if batch is not None:
        monkeypatch.setenv("NP2_BGZF_TEST_BATCH", str(batch))  # every block edge is a batch edge
    want = case_full_cuts()
    S_model, off = fm.stream(REFS, want, [EXTRA])
    targets = [i for i, r in enumerate(want) if r["name"].startswith(b"target_")]
    assert [bm.BLOCK * (k + 1) - off[i] for k, i in enumerate(targets)] == list(CUT_PLACES)
    given = [want[k] for k in np.random.default_rng(5).permutation(len(want))]
    path = write_text(tmp_path / "cuts.sam", REFS, given, extra=EXTRA)
    S, _, _, _, (bam, bai, st), _ = device_full(pol, [path], out=str(tmp_path / "cuts.bam"))
    assert S == S_model, next((i for i, (a, b) in enumerate(zip(S, S_model)) if a != b), None)
    assert bam == np2io.bgzf_deflate_host(S_model) and st["blocks"] == len(CUT_PLACES) + 1
    fm.check_files(REFS, want, bam, bai, [EXTRA], "cuts")


# ---- 3. the lean handle, two files ------------------------------------------------------------------------------------------------
def test_lean_handle_writes_the_lean_bytes_of_a_decorated_text(pol, tmp_path):
    given = accepted_records()
    path = write_text(tmp_path / "in.sam", REFS, given, extra=EXTRA)
    sam = np2io.Sam(pol, [path], keep_names=True)
    try:
        S = sam.bam_stream(pol)
        st = sam.write_bam(pol, str(tmp_path / "lean.bam"))
        for call in (lambda: sam.export_tails(pol), sam.header_text):
            with pytest.raises(Np2Error, match="NP2_SAM_KEEP_ALL"):
                call()
        assert sam.tail_stats()["tail_bytes"] == 0
    finally:
        sam.close()
    want = bm.sort_records(given)
    assert S == bm.stream(REFS, want)[0] and st["stream_bytes"] == len(S)
    bm.check_files(REFS, want, open(tmp_path / "lean.bam", "rb").read(), open(tmp_path / "lean.bam.bai", "rb").read(), "lean")


def test_header_lines_of_two_files(pol, tmp_path):
    a, b = [rec(5, tags=[b"NM:i:1"]), rec(9, tid=1)], [rec(7, qual=fm.qual_of(8)), rec(2, tid=2)]
    ea, eb = [b"@RG\tID:a", b"@CO\tone", b"@PG\tID:p"], [b"@CO\ttwo", b"@RG\tID:a", b"@RG\tID:b", b"@HD\tVN:1.5"]
    pa = write_text(tmp_path / "a.sam", REFS, a, extra=ea, end=b"\r\n")
    pb = write_text(tmp_path / "b.sam", REFS, b, extra=eb)
    S, _, _, header, _, _ = device_full(pol, [pa, pb])
    assert header == fm.header_text(REFS, [ea, eb]) and header.endswith(b"@RG\tID:a\n@CO\tone\n@PG\tID:p\n@CO\ttwo\n@RG\tID:b\n")
    given = a + b
    assert S == fm.stream(REFS, [given[i] for i in sorted_order(given)], [ea, eb])[0]
    # no kept record at all is still a BAM with its header lines
    pc = write_text(tmp_path / "c.sam", REFS, [rec(5, flag=4)], extra=ea)
    S, tails, tail_ref, header, (bam, bai, st), _ = device_full(pol, [pc], out=str(tmp_path / "c.bam"))
    assert S == fm.header(REFS, [ea]) and len(tails) == 0 and len(tail_ref) == 0 and st["records"] == 0
    fm.check_files(REFS, [], bam, bai, [ea], "no record")


# ---- 4. the written file through the project's own readers, and the command lines ------------------------------------------------
def run_module(module, args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd." + module] + args, capture_output=True, env=env, timeout=600, **kw)


@pytest.fixture(scope="module")
def two_refs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamfull")
    s1 = Synth(20000, depth=20, seed=71, diploid=True, read_len_mean=5000.0, name="ctgA")
    s2 = Synth(20000, depth=15, seed=72, name="ctgB")
    recs = pileup_to_records(s1.pileup, tid=0, rng=np.random.default_rng(5), decorate=True) + \
        pileup_to_records(s2.pileup, tid=1, rng=np.random.default_rng(6), decorate=True)
    refs = [("ctgA", s1.pileup.L), ("ctgB", s2.pileup.L)]
    given = [recs[k] for k in np.random.default_rng(8).permutation(len(recs))]
    for i, r in enumerate(given):
        r["name"] = b"read%d" % i
    fm.decorate(given, refs, seed=3)
    sam = write_text(tmp / "decorated.sam", refs, given, extra=EXTRA)
    return (s1, s2), refs, given, sam, tmp


@pytest.fixture(scope="module")
def samsorted_full(two_refs):
    _, refs, given, sam, tmp = two_refs
    out, lean = str(tmp / "full.bam"), str(tmp / "lean.bam")
    r = run_module("samsort", [sam, "-o", out, "--full"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"[samsort] full BAM" in r.stderr
    want = fm.sort_records(given)
    fm.check_files(refs, want, open(out, "rb").read(), open(out + ".bai", "rb").read(), [EXTRA], "samsort --full")
    r = run_module("samsort", [sam, "-o", lean])
    assert r.returncode == 0 and b"[samsort] lean BAM" in r.stderr, r.stderr.decode()[-3000:]
    bm.check_files(refs, want, open(lean, "rb").read(), open(lean + ".bai", "rb").read(), "samsort")
    return out, lean


@pytest.mark.parametrize("mode", ["gpu", "host"])
def test_the_full_bam_gives_the_pileup_of_the_text(pol, two_refs, samsorted_full, monkeypatch, mode):
    synths, refs, _, sam_path, _ = two_refs
    monkeypatch.setenv("NP2_INFLATE", mode)  # (read at every fetch)
    sam, bam = np2io.Sam(pol, [sam_path]), np2io.Bam(samsorted_full[0])
    assert bam.refs() == refs
    for (name, _), s in zip(refs, synths):
        ref = s.pileup.ref
        want = np2io.export_contig(pol, np2io.contig_from_sam(pol, sam, name, ref.tobytes()), ref)
        got = np2io.export_contig(pol, np2io.contig_from_bam(pol, bam, name, ref.tobytes()), ref)
        assert len(want.reads) > 10 and same_pileup(got, want), (name, mode)
    sam.close(), bam.close()


def test_lowdepth_prints_the_same_on_the_full_and_the_lean_bam(two_refs, samsorted_full):
    synths, refs, _, _, tmp = two_refs
    fa = tmp / "genome.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s.pileup.ref.tobytes()) for (n, _), s in zip(refs, synths)))
    outs = []
    for bam in samsorted_full:
        bed = bam + ".bed"
        r = run_module("lowdepth", [bam, str(fa), "-d", "12", "-l", "500", "--bed", bed])
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        outs.append((r.stdout, open(bed, "rb").read()))
    assert outs[0] == outs[1] and outs[0][0].count(b">") >= 1


def test_cli_sorted_bam_full_from_a_stream(two_refs, samsorted_full):
    from test_oracle import yak_from_seqs
    synths, refs, _, sam, tmp = two_refs
    with gzip.open(tmp / "g.fa.gz", "wt") as f:
        for (nm, _), s in zip(refs, synths):
            f.write(f">{nm}\n{s.pileup.ref.tobytes().decode()}\n")
    haps = [synths[0].hap1.decode(), synths[0].hap2.decode(), synths[1].hap1.decode()]
    np2io.write_yak(str(tmp / "k21.yak"), yak_from_seqs(haps, 21))
    np2io.write_yak(str(tmp / "k31.yak"), yak_from_seqs(haps, 31))
    rest = [str(tmp / "g.fa.gz"), str(tmp / "k21.yak"), str(tmp / "k31.yak")]
    # refused before a device is touched: no device in sight of the child
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", "-L", "10000", sam, "--sorted_bam_full"] + rest, capture_output=True, env=env, timeout=120)
    assert r.returncode != 0 and b"--sorted_bam" in r.stderr
    kept = str(tmp / "kept.bam")
    with open(sam, "rb") as text:  # the stream cannot be read twice: one pass polishes and keeps the whole mapping
        r = run_module("cli", ["-L", "10000", "-", "--sorted_bam", kept, "--sorted_bam_full"] + rest, stdin=text)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.count(b">") == 2
    for ext in ("", ".bai"):
        assert open(kept + ext, "rb").read() == open(samsorted_full[0] + ext, "rb").read()


# ---- 5. recycled memory: the scheme of test_gpu_dirty_memory.py --------------------------------------------------------------------
def poison_inputs():
    a = accepted_records()
    return {"A": a[:40], "B": case_full_cuts()[:30] + a}


_POISON_CODE = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import test_gpu_bamfull as t\n"
                "from nextpolish2_amd import Polisher, api\n"
                "byte, out = int(sys.argv[1]), sys.argv[2]\n"
                "try:\n"
                "    with api.alloc_poison(byte):\n"
                "        p = Polisher([])\n"
                "        for i, k in enumerate('ABA'):\n"
                "            S, tails, ref, _, _, _ = t.device_full(p, ['%%s.%%s.sam' %% (out, k)], out='%%s.%%d.bam' %% (out, i))\n"
                "            open('%%s.%%d.stream' %% (out, i), 'wb').write(S)\n"
                "            open('%%s.%%d.tails' %% (out, i), 'wb').write(tails.tobytes())\n"
                "        p.close()\n"
                "    assert api.alloc_poison_stats()[0] > 0\n"
                "except api.Np2Error as e:\n"
                "    print(e, file=sys.stderr)\n"
                "    sys.exit(3 if e.code == -2 else 1)\n" % (ROOT, os.path.join(ROOT, "tests")))


@pytest.mark.parametrize("byte", POISON)
def test_on_poisoned_recycled_blocks(tmp_path, byte):
    """a small input A, a larger B and A again on one context, every pool block filled with `byte` before it is handed out: the
    two A outputs are identical and equal to the model, the padding bytes between the tails included.  (A process of its own:
    the hook's counters are the process's, and tests/test_gpu_dirty_memory.py reads them.)"""
    inputs = poison_inputs()
    out = str(tmp_path / "w")
    for k, v in inputs.items():
        write_text(f"{out}.{k}.sam", REFS, v, extra=EXTRA)
    env = dict(os.environ, PYTHONPATH=ROOT, NP2_BGZF_TEST_BATCH="2", NP2_SAM_TEST_PIECE=str(1 << 16))
    r = subprocess.run([sys.executable, "-c", _POISON_CODE, str(byte), out], capture_output=True, env=env, timeout=300)
    if r.returncode == 3 or r.returncode < 0:
        device_error(r.stderr.decode(errors="replace")[-2000:], f"the full BAM under poison {byte:#x}")
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    outs = []
    for i, k in enumerate("ABA"):
        S, tails, bam, bai = (open(f"{out}.{i}.{e}", "rb").read() for e in ("stream", "tails", "bam", "bam.bai"))
        given = inputs[k]
        assert fm.check_files(REFS, [given[j] for j in sorted_order(given)], bam, bai, [EXTRA], (k, byte)) == S
        assert tails == fm.tails(REFS, given, range(len(given)))[0].tobytes()
        outs.append((S, tails, bam, bai))
    assert outs[0] == outs[2]
