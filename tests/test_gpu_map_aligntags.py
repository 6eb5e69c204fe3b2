"""The aligner's opt-in outputs on the device (include/np2_io.h: np2_map_align_*, "Tags"; kernels: csrc/np2_aligntags.hip).
Hand-built and seeded random records through np2_align_tags_device against the Python model of tests/aligntags_model.py and the
host twin: all flags and each alone, record counts around a wavefront, on recycled memory.  Every aligner edge case
(tests/align_cases.py) through MapIndex.align_x against np2_map_align_host_x, again with piece, group and traceback-budget
boundaries and a quality stream.  The first 100 reads of the committed bundle as FASTQ + FASTA through `map -a --qual --MD --cs
--eqx`: the plain line's fields, QUAL, MD and cs; the polisher's output from it byte for byte; and the full BAM the SAM door
writes from it, read back with gzip and numpy.

(The file's name sorts it behind test_gpu_map_align.py on purpose, for that file's reasons: tests/test_gpu_bai_forms.py holds only
while no device work has recycled memory in the pytest process before it, and tests/test_gpu_dirty_memory.py's first test asserts
that the poison hook was never on before it.  As test_gpu_aligntags.py this file would run in front of both.)"""
import contextlib
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import align_cases as ac
import aligntags_model as tm
import map_model as mm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from test_aligntags_cpu import FLAG_SETS, check_case_outputs, check_tags, host_x

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
ASM = os.path.join(ROOT, "tests", "golden", "ref_test_asm.fa.gz")
BUNDLE = os.path.join(ROOT, "tests", "golden", "ref_bundle")
ALL = FLAG_SETS[0]


@contextlib.contextmanager
def env(**kw):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in kw.items():
            mp.setenv(k, str(v))
        yield


_HAND = []


def hand():
    """the hand-built records, an empty one in the middle, with the model's and the host twin's answers: computed once"""
    if not _HAND:
        h = tm.hand_cases()
        records = [h[name] for name in h if name != "empty"]
        records.insert(len(records) // 2, h["empty"])
        packed = tm.pack(records)
        twin = np2io.align_tags_host(*packed, **ALL)
        check_tags(twin, records, ALL)
        _HAND.append((records, packed, twin))
    return _HAND[0]


def same_as(got, twin, flags):
    """a device answer under `flags` against the host twin's full answer, byte for byte"""
    for g, w, f in zip(got, twin, ("md", "cs", "eqx")):
        if not flags[f]:
            assert g is None
        elif f == "eqx":
            assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w))
        else:
            assert g == w


# ---- 1. hand-built records ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAG_SETS, ids=["all", "md", "cs", "eqx"])
def test_hand_records_equal_the_model_and_the_host_twin(flags):
    records, packed, twin = hand()
    got = np2io.align_tags_device(*packed, **flags)
    check_tags(got, records, flags)
    same_as(got, twin, flags)
    st = np2io.align_last_tag_stats()
    assert st["md_bytes"] == (sum(map(len, twin[0])) if flags["md"] else 0) and st["cs_bytes"] == (sum(map(len, twin[1])) if flags["cs"] else 0)
    assert st["eqx_words"] == (sum(map(len, twin[2])) if flags["eqx"] else 0) and st["tags_ms"] > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_record_counts_around_a_wavefront(n):
    records, _, _ = hand()
    short = [r for r in records if sum(k for _, k in r[2]) < 400]
    take = [short[i % len(short)] for i in range(n)]
    check_tags(np2io.align_tags_device(*tm.pack(take), **ALL), take, ALL)


def test_each_hand_record_alone_and_no_record():
    records, _, _ = hand()
    for rec in records:  # at offset 0 with nothing behind it: a walk that runs over reads beyond the buffers
        check_tags(np2io.align_tags_device(*tm.pack([rec], pad=0), **ALL), [rec], ALL)
    assert np2io.align_tags_device(b"", b"", [], [], [], **ALL) == ([], [], [])


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_dirty_memory_changes_nothing(byte):
    records, packed, twin = hand()
    with api.alloc_poison(byte):
        for flags in FLAG_SETS:
            same_as(np2io.align_tags_device(*packed, **flags), twin, flags)
        contigs, reads, _, _, _ = ac.case("pure_gaps_snv")
        with np2io.MapIndex(contigs, stream=True) as ix:
            got = ix.align_x(reads, md=True, cs=True, eqx=True)
    want = host_x("pure_gaps_snv", md=True, cs=True, eqx=True)
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4])) and got[4:] == want[4:]


def test_random_records_equal_the_model():
    records = tm.random_records()
    assert len(records) == 200
    check_tags(np2io.align_tags_device(*tm.pack(records), **ALL), records, ALL)


# ---- 2. the aligner's edge cases through MapIndex.align_x --------------------------------------------------------------------------
HOOKS = [dict(), dict(NP2_MAP_TEST_PIECE="64"), dict(NP2_MAP_TEST_BUDGET="130"), dict(NP2_ALIGN_TEST_BUDGET="1"),
         dict(NP2_MAP_TEST_PIECE="64", NP2_MAP_TEST_BUDGET="130", NP2_ALIGN_TEST_BUDGET="1")]


def seeded_quals(reads, seed=5, every=2):
    """a quality string for every `every`-th read, None for the others"""
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(33, 127, len(r)).astype(np.uint8)) if i % every == 0 and len(r) else None for i, r in enumerate(reads)]


def anchor_budget(name, least=130):
    """NP2_MAP_TEST_BUDGET for a case: `least`, or the anchors of the case's largest read where that has more (a group is whole
    reads, and a read beyond the budget is refused); counted by the host mapper, one read a call"""
    contigs, reads, _, _, _ = ac.case(name)
    kw = {f: v for f, v in ac.call_kw(name).items() if f in np2io.MAP_DEFAULTS}
    most = 0
    for r in reads:
        np2io.map_host(contigs, [r], **kw)
        most = max(most, int(np2io.map_last_stats()["anchors"]))
    return str(max(least, most))


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_align_x_equals_the_host_on_the_aligner_cases(name):
    contigs, reads, _, _, case_env = ac.case(name)
    want = host_x(name, md=True, cs=True, eqx=True)
    quals = seeded_quals(reads)
    budget = anchor_budget(name)
    for hooks in HOOKS:
        if "NP2_MAP_TEST_BUDGET" in hooks:
            hooks = dict(hooks, NP2_MAP_TEST_BUDGET=budget)
        kw = ac.call_kw(name)
        with env(**case_env, **hooks):
            with np2io.MapIndex(contigs, k=kw.pop("k", 19), w=kw.pop("w", 19), stream=True) as ix:
                plain = ix.align(reads, **kw)
                none = ix.align_x(reads, **kw)
                assert np2io.align_last_tag_stats()["tags_ms"] == 0
                got = ix.align_x(reads, quals=quals, md=True, cs=True, eqx=True, **kw)
                st = np2io.align_last_tag_stats()
                only_cs = ix.align_x(reads, cs=True, **kw)
        assert none[4] is None and none[5] is None and all(np.array_equal(a, b) for a, b in zip(plain, none[:4])), hooks
        assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4])) and got[4:] == want[4:], hooks
        assert st["qual_reads"] == sum(q is not None for q in quals) and st["md_bytes"] == sum(map(len, want[4])), hooks
        assert (st["tags_ms"] > 0) == any(int(t) >= 0 for t in want[1]["tid"]), hooks
        assert only_cs[5] == want[5] and only_cs[4] is None and np.array_equal(only_cs[2], plain[2]), hooks
        if not hooks:
            check_case_outputs(name, plain, got)


def test_quality_stream_refusals():
    contigs, reads, _, _, _ = ac.case("all_equal")
    good = seeded_quals(reads, every=1)
    with np2io.MapIndex(contigs, stream=True) as ix:
        with pytest.raises(api.Np2Error) as e:  # a byte that is no quality
            ix.align_x(reads, quals=[good[0][:-1] + b" "] + good[1:])
        assert e.value.code == -1 and "read 1: a quality byte outside '!' .. '~'" in str(e.value)
        with pytest.raises(api.Np2Error) as e:  # the stream's length is right, the first read's line is one short
            ix.align_x(reads, quals=b"".join(q + b"\n" for q in [good[0][:-1], good[1] + b"I"] + good[2:]))
        assert e.value.code == -1 and "read 1: the quality stream has no newline where the read ends" in str(e.value)
        with pytest.raises(ValueError):
            ix.align_x(reads, quals=[good[0][:-1]] + good[1:])
        ix.align_x(reads, quals=[None] * len(reads))
        assert np2io.align_last_tag_stats()["qual_reads"] == 0


# ---- 3. files: the bundle's first 100 reads, half of them with qualities -----------------------------------------------------------
def run(module, *args):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd." + module] + [str(a) for a in args], capture_output=True, text=True, env=ENV,
                          timeout=600)


class Files:
    def __init__(self, tmp):
        _, _, reads, names, _ = mm.bundle_reads(os.path.join(BUNDLE, "hifi.map.sort.bam"))
        self.reads, self.names = reads[:100], names[:100]
        assert len(set(self.names)) == 100
        self.quals = seeded_quals(self.reads, seed=9)
        self.contigs = mm.split_stream(np2io.seqfile_stream(ASM))
        self.fq, self.fa = tmp / "hifi.fastq.gz", tmp / "hifi.fa"
        with gzip.open(self.fq, "wb") as f:
            for n, r, q in zip(self.names, self.reads, self.quals):
                if q is not None:
                    f.write(b"@" + n.encode() + b" a comment\n" + r + b"\n+\n" + q + b"\n")
        with open(self.fa, "wb") as f:
            for n, r, q in zip(self.names, self.reads, self.quals):
                if q is None:
                    f.write(b">" + n.encode() + b"\n" + r + b"\n")
        self.qual_of = {n: q for n, q in zip(self.names, self.quals)}
        self.plain, self.x, self.stats = tmp / "plain.sam", tmp / "x.sam", tmp / "x.stats"
        r = run("map", ASM, self.fq, self.fa, "-a", "-o", self.plain)
        assert r.returncode == 0, r.stderr[-3000:]
        r = run("map", ASM, self.fq, self.fa, "-a", "--qual", "--MD", "--cs", "--eqx", "-o", self.x, "--stats", self.stats)
        assert r.returncode == 0, r.stderr[-3000:]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return Files(tmp_path_factory.mktemp("aligntags"))


def parse_cigar(text):
    import re
    return [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)] if text != "*" else []


def test_map_a_with_every_flag(files):
    plain, x = files.plain.read_text().splitlines(), files.x.read_text().splitlines()
    assert len(plain) == len(x) and [ln for ln in plain if ln[0] == "@"] == [ln for ln in x if ln[0] == "@"]
    tid = {ln.split("\t")[1][3:]: i for i, ln in enumerate(ln for ln in plain if ln.startswith("@SQ"))}
    n_qual = n_rev = n_x = 0
    for p, ln in zip((ln for ln in plain if ln[0] != "@"), (ln for ln in x if ln[0] != "@")):
        pf, xf = p.split("\t"), ln.split("\t")
        split = parse_cigar(xf[5])
        assert "M" not in xf[5] and "".join(f"{n}{op}" for op, n in tm.collapse(split)) == (pf[5] if pf[5] != "*" else "")
        assert xf[:5] + xf[6:10] + xf[11:16] == pf[:5] + pf[6:10] + pf[11:16] and pf[10] == "*"
        q = files.qual_of[xf[0]]
        rev = int(xf[1]) & 16
        assert xf[10] == ("*" if q is None else (q[::-1] if rev else q).decode())
        n_qual, n_rev = n_qual + (q is not None), n_rev + (q is not None and rev != 0)
        if int(xf[1]) & 4:
            assert len(xf) == 11
            continue
        assert len(xf) == 18 and xf[16].startswith("MD:Z:") and xf[17].startswith("cs:Z:")
        contig, pos = files.contigs[tid[xf[2]]], int(xf[3]) - 1
        want = tm.tags(contig[pos:], xf[9].encode(), parse_cigar(pf[5]))
        assert (xf[16][5:].encode(), xf[17][5:].encode(), split) == want, xf[0]
        n_t = sum(n for op, n in split if op in "=XD")
        assert tm.rebuild_reference(xf[9].encode(), split, want[0]) == bytes(tm.L(b) for b in contig[pos:pos + n_t])
        assert int(xf[11][5:]) == tm.nm_of(split)
        n_x += sum(op == "X" for op, _ in split)
    assert n_qual == 50 and n_rev > 5 and n_x > 0
    rows = files.stats.read_text().splitlines()
    assert len(rows) == 6 and rows[4].split("\t")[:4] == ["md_bytes", "cs_bytes", "eqx_words", "qual_reads"]
    st = dict(zip(rows[4].split("\t"), rows[5].split("\t")))
    assert st["qual_reads"] == "50" and float(st["tags_ms"]) > 0
    assert int(st["md_bytes"]) == sum(len(ln.split("\t")[16]) - 5 for ln in x if ln[0] != "@" and len(ln.split("\t")) > 16)


def test_pieces_and_groups_cut_the_qualities_as_they_cut_the_bases(files, tmp_path):
    with np2io.MapIndex(ASM) as ix:
        with env(NP2_MAP_TEST_PIECE="4096", NP2_MAP_TEST_BUDGET="20000", NP2_ALIGN_TEST_BUDGET="100000"):
            mst = np2io.map_align_files(ix, [files.fq, files.fa], tmp_path / "small.sam", qual=True, md=True, cs=True, eqx=True)
        assert mst["groups"] > 20 and mst["pieces"] > 200 and (tmp_path / "small.sam").read_bytes() == files.x.read_bytes()
        np2io.map_align_files(ix, [files.fq, files.fa], tmp_path / "md.sam", md=True)
        lines = [(a.split("\t"), b.split("\t")) for a, b in zip((tmp_path / "md.sam").read_text().splitlines(), files.x.read_text().splitlines())]
        assert all(a[-1] == b[16] and len(a) == 17 and a[10] == "*" for a, b in lines if a[0][0] != "@" and len(b) > 16)
        # a quality line that is too short, and one with a byte that is no quality: the file and the 1-based record
        for k, (line, text) in enumerate(((b"II", "the quality line is not as long as the sequence"), (b"II I", "the quality line holds a byte outside '!' .. '~'"))):
            bad = tmp_path / f"bad{k}.fastq"
            bad.write_bytes(b"@r1\nACGT\n+\nIIII\n@r2\nACGT\n+\n" + line + b"\n")
            with pytest.raises(api.Np2Error) as e:
                np2io.map_align_files(ix, [bad], tmp_path / "bad.sam", qual=True)
            assert e.value.code == -1 and f"bad{k}.fastq: record 2: {text}" in str(e.value)
            np2io.map_align_files(ix, [bad], tmp_path / "unread.sam")  # without the flag the quality lines stay unread
    r = run("map", ASM, tmp_path / "bad0.fastq", "-a", "--qual", "-o", tmp_path / "bad.sam")
    assert r.returncode != 0 and "bad0.fastq: record 2: the quality line is not as long as the sequence" in r.stderr


# ---- 4. end to end: the polisher and the full BAM ----------------------------------------------------------------------------------
def test_the_polisher_sees_no_difference(files, tmp_path):
    yaks = [os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")]
    outs = []
    for sam in (files.plain, files.x):
        out = tmp_path / (sam.name + ".fa")
        r = run("cli", "-L", "10000", sam, ASM, *yaks, "-o", out)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] and outs[0].count(b">") == len(files.contigs)


def bam_records(path):
    """name -> (flag, CIGAR words, QUAL bytes, {tag: value of a Z field}): the BAM inflated with gzip, its records walked here"""
    with gzip.open(path, "rb") as f:
        raw = f.read()
    assert raw[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    out = {}
    while at < len(raw):
        size, _, _, l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", raw, at)
        p = at + 36
        name = raw[p:p + l_name - 1].decode()
        p += l_name
        cigar = np.frombuffer(raw, "<u4", n_cig, p)
        p += 4 * n_cig + (l_seq + 1) // 2
        qual = raw[p:p + l_seq]
        p += l_seq
        tags, end = {}, at + 4 + size
        while p < end:
            tag, typ = raw[p:p + 2].decode(), raw[p + 2:p + 3]
            p += 3
            if typ == b"Z":
                z = raw.index(b"\0", p)
                tags[tag] = raw[p:z]
                p = z + 1
            else:
                p += {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}[typ]
        out[name] = (flag, cigar, qual, tags)
        at = end
    return out


def test_the_full_bam_carries_qualities_md_and_eqx(files, tmp_path):
    from nextpolish2_amd.api import Polisher
    pol = Polisher([])
    try:
        sam = np2io.Sam(pol, [str(files.x)], keep_names=True, keep_all=True)
        try:
            sam.write_bam(pol, str(tmp_path / "x.bam"))
        finally:
            sam.close()
    finally:
        pol.close()
    recs = bam_records(tmp_path / "x.bam")
    lines = [ln.split("\t") for ln in files.x.read_text().splitlines() if ln[0] != "@"]
    assert len(recs) == len(lines) == 100
    ops = set()
    for f in lines:
        flag, cigar, qual, tags = recs[f[0]]
        assert flag == int(f[1])
        assert qual == (b"\xff" * len(f[9]) if f[10] == "*" else bytes(b - 33 for b in f[10].encode()))
        if not flag & 4:
            assert tags["MD"] == f[16][5:].encode() and tags["cs"] == f[17][5:].encode()
            assert "".join(f"{int(w) >> 4}{tm.OPS[int(w) & 15]}" for w in cigar) == f[5]
            ops |= set(int(w) & 15 for w in cigar)
    assert {7, 8} <= ops and 0 not in ops
