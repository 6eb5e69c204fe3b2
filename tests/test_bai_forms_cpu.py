"""The .bai reader (csrc/np2_bai_core.hpp, np2_bam_open) on indexes in the forms of tests/bai_model.py — its own writer's, the
one htslib writes (modelled, see bai_model), a sparse one, one that spells block ends the other way — over the BAMs of
tests/bai_cases.py: what the reader derives (first and last offset of a reference, where a zone starts) against an
index-free scan of the file; and the parser as a stand-alone program under the address and undefined-behaviour sanitizers
on every truncation of an index and on absurd counts, each of which must be refused and none read past its bytes."""
import os
import subprocess

import pytest

import bai_cases as bc
import bai_model as bm
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.bamio import read_bam, records_to_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "nextpolish2_amd", "csrc")
NP2_E_ARG = -1
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("bai_forms")
    recs, refs, paths = bc.build(d)
    own = {cut: open(p + ".bai", "rb").read() for cut, p in paths.items()}  # what write_bam wrote, before it is replaced
    exe = str(d / "bai_core_test")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
                        os.path.join(HERE, "tools", "bai_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(d=d, recs=recs, refs=refs, paths=paths, own=own, exe=exe, scans={cut: bm.scan(p) for cut, p in paths.items()})


def own_copy(case, cut, tag):
    """a name of its own for the BAM of `cut` (a link to it), so that a test's <name>.bai is that test's alone"""
    path = str(case["d"] / ("%s.%s.bam" % (cut, tag)))
    if not os.path.lexists(path):
        os.symlink(case["paths"][cut], path)
    return path


def tool(case, bai, cmd):
    r = subprocess.run([case["exe"], bai, str(len(bc.REFS)), cmd], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (cmd, r.returncode, r.stderr[-3000:])  # (a sanitizer report ends the program)
    lines = r.stdout.splitlines()
    assert lines and lines[-1].startswith("done "), lines[-3:]
    return lines[:-1], int(lines[-1].split()[1])


@pytest.mark.parametrize("cut", list(bc.CUTS))
def test_scan_reads_the_records_that_were_written(case, cut):
    sc = case["scans"][cut]
    assert sc.refs == bc.REFS == read_bam(case["paths"][cut])[0]
    assert len(sc.records) == len(case["recs"]) > 200
    for got, want in zip(sc.records, case["recs"]):
        assert {k: got[k] for k in ("tid", "pos", "mapq", "flag", "name", "cigar", "seq")} == \
               {k: (want[k].upper() if k == "seq" else want[k]) for k in ("tid", "pos", "mapq", "flag", "name", "cigar", "seq")}
    # offsets: ascending, each record's end the next one's begin, the last end at the end-of-file marker
    assert all(a["end"] == b["beg"] and a["beg"] < b["beg"] for a, b in zip(sc.records, sc.records[1:]))
    assert sc.records[-1]["end"] == sc.blocks[-1][0] << 16 and sc.blocks[-1][1] == 0


def test_the_bams_hold_the_edges_they_are_made_for(case):
    sc = case["scans"]["rec"]
    W = bc.W
    covered = lambda tid: {w for r in sc.of(tid) for w in range(r["pos"] >> 14, ((r["pos"] + max(r["span"], 1) - 1) >> 14) + 1)}
    assert covered(0) == {0, 1, 2, 3, 4} and covered(1) == {2, 4, 5} and covered(2) == set() and covered(3) == {0}
    a = sc.of(0)
    assert any(r["span"] == bc.LONG_LEN and len(set(range(r["pos"] >> 14, (r["pos"] + r["span"] - 1 >> 14) + 1))) >= 3 for r in a)
    assert any(r["flag"] & 4 and r["span"] == 0 and r["pos"] == bc.UNMAPPED_POS for r in a) and not a[0]["flag"] & 4 and not a[-1]["flag"] & 4
    assert any((r["pos"] + r["span"]) % W == 0 and r["span"] for r in a) and any(r["pos"] % W == 0 and r["pos"] for r in a)
    assert sc.of(3)[0]["beg"] >> 16 == sc.of(1)[-1]["beg"] >> 16  # ctgD begins in the block ctgB's last record lies in
    # blocks: records end on block ends | almost never do | length words and fixed fields straddle blocks
    ends = lambda c: {so + n for _, n, so in case["scans"][c].blocks if n}
    assert len(sc.blocks) >= 10 and all(any(r["spos"] == so for r in sc.records) for _, n, so in sc.blocks[1:] if n)
    b600 = case["scans"]["b600"]
    assert len(b600.blocks) > 1000
    assert b600.records[bc.STRADDLED]["spos"] + 2 in ends("b600")
    assert any(r["spos"] + 4 < e < r["spos"] + 36 for r in b600.records for e in (ends("b600") & set(range(r["spos"], r["spos"] + 36))))
    # every record but the one with flag 0x4 is admitted under the tests' options (the shard test counts on it)
    from oracle import np2_oracle as orc
    for tid in (0, 1, 3):
        rr = sc.of(tid)
        arr, cig, _, asc, asc_off = records_to_arrays(rr)
        pu = orc.front_end(case["refs"][tid], arr, cig, asc, asc_off, bc.front_opts())
        assert pu.n_reads - 1 == sum(1 for r in rr if not r["flag"] & 4), tid


def test_own_form_reproduces_write_bam_byte_for_byte(case):
    sc = case["scans"]["rec"]
    assert bm.pack_bai(*bm.index_of(sc, "own")) == case["own"]["rec"]
    # (and the pack / unpack pair the GPU tests edit indexes with is exact)
    for form in bm.FORMS:
        data = bm.pack_bai(*bm.index_of(sc, form, seed=5))
        assert bm.pack_bai(*bm.unpack_bai(data)) == data
    # on the cut BAMs write_bam sees a block closed the moment it is full, so the two differ there at most in how an end on a
    # block's end is spelled and in the chunk that spelling splits: the same linear index, the same stream positions
    for cut in ("ff00", "b600"):
        s2 = case["scans"][cut]
        mine, theirs = bm.index_of(s2, "own")[0], bm.unpack_bai(case["own"][cut])[0]
        for (mb, ml), (tb, tl) in zip(mine, theirs):
            assert ml == tl and [b for b, _ in mb] == [b for b, _ in tb]
            for (_, mc), (_, tc) in zip(mb, tb):
                assert s2.spos(mc[0][0]) == s2.spos(tc[0][0]) and s2.spos(mc[-1][1]) == s2.spos(tc[-1][1])


def test_the_htslib_form_has_what_htslib_adds(case):
    """the model's htslib form really differs from the own form in every feature the readers must cope with"""
    sc = case["scans"]["ff00"]
    refs, tail = bm.index_of(sc, "htslib", seed=1)
    own, _ = bm.index_of(sc, "own")
    assert len(tail) == 8
    for tid in (0, 1, 3):
        bins, lin = refs[tid]
        ids = [b for b, _ in bins]
        assert bm.META_BIN in ids
        if tid != 3:  # (ctgD: one bin, nothing to merge or to put out of order)
            assert ids != sorted(ids) and len(ids) - 1 < len(own[tid][0])  # hash order; children went into their parents
            assert any(len(ch) < sum(len(c) for b2, c in own[tid][0] if b2 == b or (b2 - 1) >> 3 == b) for b, ch in bins if b != bm.META_BIN)
        meta = dict(bins)[bm.META_BIN]
        rr = sc.of(tid)
        assert meta[0] == (rr[0]["beg"], rr[-1]["end"]) and meta[1] == (sum(1 for r in rr if not r["flag"] & 4), sum(1 for r in rr if r["flag"] & 4))
    assert refs[2] == ([], [])
    linB, ownB = refs[1][1], own[1][1]
    assert linB[0] == linB[1] == linB[2] == sc.of(1)[0]["beg"] and ownB[0] == ownB[1] == 0  # leading windows: back-filled | 0
    assert linB[3] == linB[4] != linB[2] and ownB[3] == ownB[2]                              # the interior one: next | previous
    assert bm.index_of(sc, "sparse")[0][1][1][:4] == [0, 0, linB[2], 0]


def derived(case, path):
    """what the stand-alone parser derives from <path>.bai -> {tid: (ref_start, ref_end, lin, zone starts)}"""
    lines, _ = tool(case, path + ".bai", "parse")
    assert not lines[0].startswith("error"), lines[0]
    out = {}
    for i in range(0, len(lines), 3):
        r = lines[i].split()
        assert r[0] == "ref" and lines[i + 1].split()[:2] == ["lin", r[1]] and lines[i + 2].split()[:2] == ["zone", r[1]]
        lin = [int(x) for x in lines[i + 1].split()[2:]]
        assert len(lin) == int(r[4])
        out[int(r[1])] = (int(r[2]), int(r[3]), lin, [int(x) for x in lines[i + 2].split()[2:]])
    return out


@pytest.mark.parametrize("cut", list(bc.CUTS))
@pytest.mark.parametrize("form", bm.FORMS)
def test_what_the_reader_derives_equals_the_scan(case, form, cut):
    sc, path = case["scans"][cut], own_copy(case, cut, "derives_" + form)
    bm.write_bai(path, sc, form, seed=11)
    bam = np2io.Bam(path)
    assert bam.refs() == bc.REFS
    bam.close()
    dv = derived(case, path)
    starts = {r["spos"] for r in sc.records}
    # the own form spells an end on a block's end (this block, inflated size), as write_bam does; end_at_isize every such
    # offset: there the same stream position is asked for, everywhere else the very offset
    same = (lambda got, want_spos: sc.spos(got) == want_spos) if form in ("own", "end_at_isize") else (lambda got, want_spos: got == sc.voff(want_spos))
    for tid, (name, L) in enumerate(bc.REFS):
        ref_start, ref_end, lin, zones = dv[tid]
        rr = sc.of(tid)
        if not rr:
            assert (ref_start, ref_end, lin) == (NONE, 0, []) and set(zones) == {NONE}
            continue
        assert same(ref_start, rr[0]["spos"]), (name, ref_start, rr[0]["beg"])
        if form != "end_at_isize":
            assert ref_start == rr[0]["beg"]
        assert same(ref_end, rr[-1]["send"]), (name, ref_end, rr[-1]["end"])
        indexed = [r for r in rr if not (form in ("own", "end_at_isize") and r["flag"] & 4)]
        assert len(lin) == max((r["pos"] + max(r["span"], 1) - 1) >> 14 for r in indexed) + 1
        for w, z in enumerate(zones):  # zone_lo = w * 16384, up to one window past the index's last
            at = sc.spos(z)
            assert at in starts, (name, w, z)  # a record's start, in either spelling
            if form != "end_at_isize":
                assert z == sc.voff(at)
            hit = [r for r in bm.fetch_rule(sc, tid, w * bc.W, L) if not (form in ("own", "end_at_isize") and r["flag"] & 4)]
            if hit:
                assert at <= hit[0]["spos"], (name, w, z, hit[0]["beg"])
            if w == 0:
                assert z == ref_start


FORM_CUT = [("htslib", "ff00"), ("own", "rec"), ("sparse", "b600"), ("htslib_nometa", "rec"), ("end_at_isize", "rec")]


@pytest.mark.parametrize("form,cut", FORM_CUT)
def test_every_truncation_is_refused(case, form, cut):
    sc, path = case["scans"][cut], own_copy(case, cut, "truncations_" + form)
    data = bm.write_bai(path, sc, form, seed=3)
    lines, n = tool(case, path + ".bai", "truncations")
    assert n == len(data)
    # the one prefix that is a whole index: the htslib form without its trailing count (what htslib_nometa would be with the
    # pseudo-bins).  A prefix that ends behind a reference other than the last still names n_ref references: refused.
    want = [len(data) - 8] if form == "htslib" else []
    assert all(e - 8 not in want for e in bm.ref_block_ends(bm.index_of(sc, form, seed=3)[0])[:-1])
    assert [int(l.split()[1]) for l in lines] == want, lines[:10]


@pytest.mark.parametrize("form,cut", FORM_CUT[:3])
def test_absurd_counts_are_refused(case, form, cut):
    sc, path = case["scans"][cut], own_copy(case, cut, "counts_" + form)
    refs, _ = bm.index_of(sc, form, seed=3)
    bm.write_bai(path, sc, form, seed=3)
    lines, n = tool(case, path + ".bai", "counts")
    assert n == 2 * (1 + sum(2 + len(bins) for bins, _ in refs))  # n_ref; per reference n_bin, n_intv and a n_chunk per bin
    assert lines == []


def test_np2_bam_open_refuses_a_truncated_index(case):
    sc, path = case["scans"]["ff00"], own_copy(case, "ff00", "open_refuses")
    data = bm.write_bai(path, sc, "htslib", seed=3)
    refs, _ = bm.index_of(sc, "htslib", seed=3)
    ends = bm.ref_block_ends(refs)
    cuts = [8 + 4 + 8 + 20,                      # inside a chunk of the first bin of ctgA
            ends[0] - 8 * len(refs[0][1]) + 12,  # inside ctgA's linear index
            ends[1],                             # behind ctgB's part: two of four references
            len(data) - 3]                       # inside the trailing count
    for k in cuts:
        with open(path + ".bai", "wb") as f:
            f.write(data[:k])
        with pytest.raises(Np2Error) as e:
            np2io.Bam(path)
        assert e.value.code == NP2_E_ARG and ".bai" in str(e.value), (k, str(e.value))
        assert ("truncated" in str(e.value)) == (k != len(data) - 3)  # (bytes behind the last reference have a message of their own)
    for field_off in (4, 8):  # n_ref, ctgA's n_bin
        with open(path + ".bai", "wb") as f:
            f.write(data[:field_off] + b"\xff\xff\xff\x7f" + data[field_off + 4:])
        with pytest.raises(Np2Error) as e:
            np2io.Bam(path)
        assert e.value.code == NP2_E_ARG
    bm.write_bai(path, sc, "htslib", seed=3)
    np2io.Bam(path).close()
