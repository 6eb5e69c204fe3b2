"""The aligner on the device (np2_map_align_bytes, np2_map_align_files, python -m nextpolish2_amd.map -a) against the Python model
of tests/align_model.py: records, CIGAR words and counts equal on the edge cases of tests/align_cases.py, again with piece, group
and traceback-budget boundaries inside and between reads, around a wavefront of reads and on recycled memory; the SAM of a
100-read subset of the committed bundle byte for byte; and the whole bundle through `map -a` into the polisher.

(The file's name sorts it behind test_gpu_map.py on purpose.  tests/test_gpu_bai_forms.py takes its expected answers as raw
pileup buffers, unwritten padding included, from the pytest process and compares them with a fresh child process's: it holds
only while no device work has recycled memory in the process before it, and it fails behind this file even when the poison
hook is kept out of the process.  tests/test_gpu_dirty_memory.py's first test asserts that the hook was never on before it.)"""
import contextlib
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases as ac
import align_model as am
import map_cases as mc
import map_model as mm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from test_map_cpu import ASM, BAM, bundle, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
BUNDLE = os.path.dirname(BAM)


@contextlib.contextmanager
def env(**kw):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in kw.items():
            mp.setenv(k, str(v))
        yield


def device_equals_model(name, **hooks):
    contigs, reads, _, _, case_env = ac.case(name)
    kw = ac.call_kw(name)
    with env(**case_env, **hooks):
        with np2io.MapIndex(contigs, k=kw.pop("k", 19), w=kw.pop("w", 19), stream=True) as ix:
            got = ix.align(reads, **kw)
            st, mst = np2io.align_last_stats(), np2io.map_last_stats()
    ac.check(got, name)
    cnt, tot = ac.expected(name)[3], ac.expected(name)[4]
    assert {f: st[f] for f in cnt} == cnt and {f: mst[f] for f in tot} == tot
    return mst


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_edge_case_equals_the_model(name):
    device_equals_model(name)


@pytest.mark.parametrize("name", ["pure_gaps_snv", "overhang", "homopolymer", "cells_overflow"])
@pytest.mark.parametrize("hooks", [dict(NP2_MAP_TEST_PIECE="256"), dict(NP2_MAP_TEST_BUDGET="130"), dict(NP2_ALIGN_TEST_BUDGET="2000"),
                                   dict(NP2_MAP_TEST_PIECE="64", NP2_MAP_TEST_BUDGET="130", NP2_ALIGN_TEST_BUDGET="1")],
                         ids=["piece", "anchors", "traceback", "all"])
def test_piece_group_and_traceback_boundaries_change_nothing(name, hooks):
    whole = device_equals_model(name)
    st = device_equals_model(name, **hooks)
    n_reads = len(ac.case(name)[1])
    if "NP2_MAP_TEST_PIECE" in hooks:
        assert st["pieces"] > n_reads  # pieces inside reads
    if "NP2_MAP_TEST_BUDGET" in hooks or "NP2_ALIGN_TEST_BUDGET" in hooks:
        assert whole["groups"] < n_reads and st["groups"] > whole["groups"]
    if "NP2_ALIGN_TEST_BUDGET" in hooks and len(hooks) > 1:
        assert st["groups"] >= n_reads  # one read a group


class Pool:
    """reads of several cases against the one contig, with the model's answers, to draw read counts from"""

    def __init__(self):
        self.reads, self.hits, self.recs, self.cigars = [], [], [], []
        for name in ("pure_gaps_snv", "all_equal", "overhang", "unmapped_between", "n_bases"):
            contigs, reads, o, ao, _ = ac.case(name)
            assert contigs == [ac.CONTIG] and not o and not ao
            hits, recs, cigars, _, _ = ac.expected(name)
            self.reads += reads
            self.hits += hits
            self.recs += recs
            self.cigars += cigars

    def take(self, n):
        pick = [i % len(self.reads) for i in range(n)]
        return [self.reads[i] for i in pick], [self.recs[i] for i in pick], [self.cigars[i] for i in pick]


_POOL = []


def pool():
    if not _POOL:
        _POOL.append(Pool())
    return _POOL[0]


def check_pool(got, recs, cigars):
    _, gr, gc, go = got
    have = np.array([[int(r[f]) for f in am.REC_FIELDS] for r in gr], np.int64).reshape(len(recs), len(am.REC_FIELDS))
    assert np.array_equal(have, am.recs_array(recs))
    words, off = am.cigar_words(cigars)
    assert np.array_equal(go, off) and np.array_equal(gc, words)


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65])
def test_read_counts_around_a_wavefront(n_reads):
    reads, recs, cigars = pool().take(n_reads)
    with np2io.MapIndex([ac.CONTIG], stream=True) as ix:
        check_pool(ix.align(reads), recs, cigars)


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_dirty_memory_changes_nothing(byte):
    reads, recs, cigars = pool().take(40)
    with api.alloc_poison(byte):
        with np2io.MapIndex([ac.CONTIG], stream=True) as ix:
            check_pool(ix.align(reads), recs, cigars)
            with env(NP2_MAP_TEST_PIECE="2048", NP2_MAP_TEST_BUDGET="300", NP2_ALIGN_TEST_BUDGET="5000"):
                check_pool(ix.align(reads), recs, cigars)
        device_equals_model("band_129")
        device_equals_model("cells_overflow")
        device_equals_model("gaps_merge")


def test_mapping_is_unchanged_after_an_align_call(tmp_path):
    s = synthetic()
    with np2io.MapIndex(s.contigs, stream=True) as ix:
        before = ix.map(s.reads, chains=True)
        hits, recs, _, _ = ix.align(s.reads)
        after = ix.map(s.reads, chains=True)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)) and np.array_equal(hits, before[0])
        mc.check(after[0], after[1], after[2], s.hits, s.chains, s.reads)
        assert [int(r["tid"]) for r in recs] == [h["tid"] for h in s.hits]
        # and the PAF text: before, between and after SAM runs on the same index
        names = ["s%d" % i for i in range(len(s.reads))]
        want = mm.paf(names, s.hits, ix.names, ix.lens)
        fa = tmp_path / "reads.fa"
        fa.write_text("".join(f">{n}\n{r.decode()}\n" for n, r in zip(names, s.reads)))
        for paf in ("a.paf", "b.paf"):
            np2io.map_files(ix, [fa], tmp_path / paf)
            assert (tmp_path / paf).read_text() == want
            np2io.map_align_files(ix, [fa], tmp_path / "x.sam")
        assert [int(r["pos"]) for r, c in zip(recs, s.cases) if c["kind"] == "clear"] == [c["origin"] for c in s.cases if c["kind"] == "clear"]


# ---- the committed bundle: the first 30, 40 middle and the last 30 of its 574 reads (both contig-end overhangs are among them) ----
SUBSET = list(range(30)) + list(range(267, 307)) + list(range(544, 574))


class Subset:
    def __init__(self):
        b = bundle()
        self.b = b
        self.reads, self.names = [b.reads[i] for i in SUBSET], [b.names[i] for i in SUBSET]
        self.hits, self.chains = [b.hits[i] for i in SUBSET], [b.chains[i] for i in SUBSET]
        _, self.recs, self.cigars, self.cnt = am.align_mapped(b.contigs, self.reads, self.hits, self.chains, 19)
        self.sam = am.sam(self.names, self.reads, self.hits, self.recs, self.cigars, b.tnames, [len(c) for c in b.contigs])


_SUBSET = []


def subset():
    if not _SUBSET:
        _SUBSET.append(Subset())
    return _SUBSET[0]


def run_map(*args):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd.map"] + [str(a) for a in args], capture_output=True, text=True, env=ENV,
                          timeout=600)


def test_bundle_subset_records_and_sam(tmp_path):
    s = subset()
    b = s.b
    # the model's known answers
    assert (s.cnt["pins"], s.cnt["cores"], s.cnt["clipped_bases"], s.cnt["overflow"]) == (26295, 1096, 565281, 0)
    assert (s.cnt["segments"], s.cnt["equal"], s.cnt["pure_gap"], s.cnt["snv"], s.cnt["cells"]) == (26195, 21676, 2467, 956, 1708033)
    assert ac.cigar_str(s.cigars[0]).startswith("12310S152M1I") and ac.cigar_str(s.cigars[-1]).endswith("42M12529S")
    start_slack = end_slack = 0
    for i, rec in zip(SUBSET, s.recs):
        assert rec["tid"] == b.recs[i]["tid"] and rec["flag"] == (b.recs[i]["flag"] & 16)
        start_slack, end_slack = max(start_slack, abs(rec["pos"] - b.recs[i]["pos"])), max(end_slack, abs(rec["end"] - b.ends[i]))
    assert (start_slack, end_slack) == (4, 5)
    fa = tmp_path / "hifi.fa"
    fa.write_text("".join(f">{n} some comment\n{r.decode()}\n" for n, r in zip(s.names, s.reads)))
    with np2io.MapIndex(ASM) as ix:
        got = ix.align(s.reads)
        check_pool(got, s.recs, s.cigars)
        st = np2io.align_last_stats()
        assert {f: st[f] for f in s.cnt} == s.cnt
        mst = np2io.map_align_files(ix, [fa], tmp_path / "out.sam")
        assert (mst["reads"], mst["mapped"]) == (100, 100) and (tmp_path / "out.sam").read_text() == s.sam
        np2io.map_align_files(ix, [fa], tmp_path / "out.sam.gz")
        with gzip.open(tmp_path / "out.sam.gz", "rt") as f:
            assert f.read() == s.sam
        with env(NP2_MAP_TEST_PIECE="4096", NP2_MAP_TEST_BUDGET="20000", NP2_ALIGN_TEST_BUDGET="100000"):
            mst = np2io.map_align_files(ix, [fa], tmp_path / "small.sam")
        assert mst["groups"] > 20 and (tmp_path / "small.sam").read_text() == s.sam
    r = run_map(ASM, fa, "-a", "--stats", tmp_path / "stats.tsv")
    assert r.returncode == 0 and r.stdout == s.sam, r.stderr[-3000:]
    lines = (tmp_path / "stats.tsv").read_text().splitlines()
    assert len(lines) == 4 and dict(zip(lines[0].split("\t"), lines[1].split("\t")))["mapped"] == "100"
    assert dict(zip(lines[2].split("\t"), lines[3].split("\t")))["cores"] == "1096"
    r = run_map(ASM, fa, "-a", "-E", "0")
    assert r.returncode != 0 and "gap_ext" in r.stderr


def test_whole_bundle_through_map_a_into_the_polisher(tmp_path):
    """map -a | cli: exits 0, writes every contig, and leaves no more k-mers absent from the short-read tables than the input
    assembly has.  (How far the result is from the bundle's own polish is a measurement: profiles/align_cost.txt.)"""
    b = bundle()
    fa = tmp_path / "hifi.fa.gz"
    with gzip.open(fa, "wt") as f:
        f.write("".join(f">{n}\n{r.decode()}\n" for n, r in zip(b.names, b.reads)))
    r = run_map(ASM, fa, "-a", "-o", tmp_path / "map.sam")
    assert r.returncode == 0, r.stderr[-3000:]
    yaks = [os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")]
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", "-L", "10000", str(tmp_path / "map.sam"), ASM] + yaks +
                       ["-o", str(tmp_path / "out.fa"), "--qv", str(tmp_path / "qv.tsv")], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = (tmp_path / "out.fa").read_text()
    assert [ln[1:].split()[0] for ln in out.splitlines() if ln.startswith(">")] == b.tnames
    rows = [ln.split("\t") for ln in (tmp_path / "qv.tsv").read_text().splitlines()]
    head = rows[0]
    totals = [dict(zip(head, row)) for row in rows[1:] if row[0] == "total"]
    assert [t["k"] for t in totals] == ["21", "31"]
    for t in totals:
        assert int(t["absent_out"]) <= int(t["absent_in"]), t


def test_an_index_built_with_another_k_is_refused():
    import ctypes as C
    reads = np.frombuffer(bytes(ac.cut()) + b"\n", np.uint8)
    recs = np.zeros(1, np2io.ALIGN_REC_DTYPE)
    with np2io.MapIndex([ac.CONTIG], k=19, w=19, stream=True) as ix:
        L = np2io._bind()
        o, ao = np2io.map_opts(k=21), np2io.align_opts()
        rc = L.np2_map_align_bytes(ix._h, reads.ctypes.data, len(reads), 1, C.byref(o), C.byref(ao), None, recs.ctypes.data, None, None)
        assert rc == -1 and b"k = 19" in L.np2_io_last_error()
        with pytest.raises(api.Np2Error) as e:
            ix.align([bytes(ac.cut())], band=2000)
        assert e.value.code == -1 and "band" in str(e.value)
        hits, recs, cigar, off = ix.align([bytes(ac.cut())])  # the handle still works
        assert ac.cigar_text(cigar, off) == ["600M"]
