"""The reads door of the resident SAM on the device (np2_sam_from_reads, np2_sam_from_read_bytes, cli --from_reads) against its
defining sentence: the handle holds what np2_sam_open holds after reading the SAM np2_map_align_files writes for the same call.
Every array of both handles is compared with np.array_equal on the edge cases of align_cases and mappolish_cases, again with piece,
group and traceback-budget boundaries inside and between reads, around a wavefront of reads and on recycled memory; a 100-read
subset of the committed bundle down to the bytes of the sorted BAM and its index; and the whole bundle through the command line.

(The file's name sorts it behind test_gpu_bai_forms.py and test_gpu_dirty_memory.py on purpose: the docstring of
tests/test_gpu_map_align.py has the reason.)"""
import contextlib
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases as ac
import mappolish_cases as pc
from nextpolish2_amd import Polisher, api
from nextpolish2_amd import io as np2io
from test_map_cpu import ASM, BAM, bundle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
BUNDLE = os.path.dirname(BAM)
STAT_FIELDS = ("lines", "records", "unmapped", "kept", "cigar_words", "seq_bytes")


@contextlib.contextmanager
def env(**kw):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in kw.items():
            mp.setenv(k, str(v))
        yield


_POL = []


def pol():
    """one table-less context for the file's handles (the command line's front ends use the same kind)"""
    if not _POL:
        _POL.append(Polisher([], device=0))
    return _POL[0]


def write_fasta(path, names, reads, comment=""):
    path.write_text("".join(f">{n}{comment}\n{bytes(r).decode()}\n" for n, r in zip(names, reads)))
    return path


def held(sam):
    """everything a handle holds that a reader can see: the four arrays, the names, the references, the counts"""
    st = sam.stats()
    return sam.export(pol()), sam.export_names(pol()), sam.refs(), {f: st[f] for f in STAT_FIELDS}


def same_handles(a, b):
    return (pc.same_arrays(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1]) and a[2] == b[2] and
            a[3] == b[3])


def both_doors(ix, tmp_path, names, reads, tie, kw, hooks=None):
    """-> (the reads door's handle from the files, the text door's from the SAM map_align_files writes, the mapper's stats of the
    reads door's call)"""
    fa = write_fasta(tmp_path / "reads.fa", names, reads)
    sam_path = tmp_path / f"out.{tie}.sam"
    np2io.map_align_files(ix, [fa], sam_path, **kw)
    with env(**(hooks or {})):
        a = np2io.Sam.from_reads(pol(), ix, [fa], tie=tie, keep_names=True, **kw)
        mst, ast = np2io.map_last_stats(), np2io.align_last_stats()
    b = np2io.Sam(pol(), [sam_path], tie=tie, keep_names=True)
    ha, hb = held(a), held(b)
    st = a.stats()
    assert st["parse_ms"] == 0 and st["pack_ms"] >= 0 and ast["write_ms"] == 0
    a.close(), b.close()
    return ha, hb, mst


def check_case(name, tmp_path, hooks=None, ties=np2io.SAM_TIES):
    contigs, reads, _, _, case_env = pc.case(name)
    kw = pc.call_kw(name)
    names = pc.names_of(name)
    out = []
    with env(**case_env):
        with np2io.MapIndex(contigs, k=kw.pop("k", 19), w=kw.pop("w", 19), stream=True) as ix:
            for tie in ties:
                ha, hb, mst = both_doors(ix, tmp_path, names, reads, tie, kw, hooks)
                assert same_handles(ha, hb), (name, tie, ha[3], hb[3])
                exp = pc.want(name, tie)  # ... and the model of the text door says the same
                assert pc.same_arrays(ha[0], exp) and ha[3] == {f: exp[4][f] for f in STAT_FIELDS}, (name, tie)
                assert mst["reads"] == len(reads)
                # the reads in memory, numbered: the same arrays, the names 1, 2, ...
                with env(**(hooks or {})):
                    c = np2io.Sam.from_reads(pol(), ix, reads, tie=tie, keep_names=True, **kw)
                hc = held(c)
                c.close()
                assert pc.same_arrays(hc[0], ha[0]) and hc[3] == ha[3] and np.array_equal(hc[1][1] & 255, np.array(
                    [len(str(int(n[1:]) + 1)) for n in kept_names(ha[1])], np.uint64))
                out.append((ha, mst))
    return out


def kept_names(names_ref):
    nm, ref = names_ref
    return [bytes(nm[int(r) >> 8:(int(r) >> 8) + (int(r) & 255)]).decode() for r in ref]


# ---- 5. parity, the core test ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.all_cases()))
def test_reads_door_equals_text_door(name, tmp_path):
    res = check_case(name, tmp_path)
    if name in ("cells_overflow", "unmapped_between"):  # the dropped reads
        assert res[0][0][3]["unmapped"] == 1 and res[0][0][3]["kept"] == 2
    if name == "none_maps":  # an empty handle reads as a contig without reads
        contigs, reads = pc.case(name)[:2]
        with np2io.MapIndex(contigs, stream=True) as ix:
            sam = np2io.Sam.from_reads(pol(), ix, reads)
            assert sam.stats()["kept"] == 0 and sam.export(pol())[0].shape == (0,)
            p = np2io.export_contig(pol(), np2io.contig_from_sam(pol(), sam, "1", contigs[0]), np.frombuffer(contigs[0], np.uint8))
            assert len(p.reads) == 1  # (the contig itself)
            sam.close()


# ---- 6. boundaries change nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pure_gaps_snv", "overhang", "seq_offsets", "cells_overflow"])
@pytest.mark.parametrize("hooks", [dict(NP2_MAP_TEST_PIECE="256"), dict(NP2_MAP_TEST_BUDGET="130"), dict(NP2_ALIGN_TEST_BUDGET="2000"),
                                   dict(NP2_MAP_TEST_PIECE="64", NP2_MAP_TEST_BUDGET="130", NP2_ALIGN_TEST_BUDGET="1")],
                         ids=["piece", "anchors", "traceback", "all"])
def test_piece_group_and_traceback_boundaries_change_nothing(name, hooks, tmp_path):
    (whole, wst), = check_case(name, tmp_path, ties=("strand",))
    (cut, st), = check_case(name, tmp_path, hooks=hooks, ties=("strand",))
    assert same_handles(whole, cut)
    n_reads = len(pc.case(name)[1])
    if "NP2_MAP_TEST_PIECE" in hooks:
        assert st["pieces"] > n_reads  # pieces inside reads
    if "NP2_MAP_TEST_BUDGET" in hooks or "NP2_ALIGN_TEST_BUDGET" in hooks:
        assert wst["groups"] < n_reads and st["groups"] > wst["groups"]
    if "NP2_ALIGN_TEST_BUDGET" in hooks and len(hooks) > 1:
        assert st["groups"] >= n_reads  # one read a group


# ---- 7. read counts around a wavefront -------------------------------------------------------------------------------------------
def pool_reads(n):
    """reads of several cases against the one contig, both strands, odd and even, mapped and not"""
    reads = []
    for name in ("pure_gaps_snv", "odd_even_both_strands", "overhang", "unmapped_between", "iupac_stray", "seq_offsets"):
        contigs, rd, o, ao, _ = pc.case(name)
        assert contigs == [ac.CONTIG] and not o and not ao
        reads += rd
    return [reads[i % len(reads)] for i in range(n)], len(reads), reads.index(ac.case("unmapped_between")[1][1])


def pool_parity(n_reads, tmp_path, tie="strand", hooks=None):
    reads, n_pool, unmapped = pool_reads(n_reads)
    names = ["q%d" % i for i in range(n_reads)]
    with np2io.MapIndex([ac.CONTIG], stream=True) as ix:
        ha, hb, _ = both_doors(ix, tmp_path, names, reads, tie, {}, hooks)
    assert same_handles(ha, hb) and ha[3]["records"] == n_reads
    assert ha[3]["kept"] == sum(1 for i in range(n_reads) if i % n_pool != unmapped)  # (the pool's one read that maps nowhere)
    return ha


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65])
def test_read_counts_around_a_wavefront(n_reads, tmp_path):
    pool_parity(n_reads, tmp_path)


# ---- 8. recycled memory changes nothing ------------------------------------------------------------------------------------------
def smaller_half():
    size = lambda name: sum(len(r) for r in pc.case(name)[1])
    names = sorted(pc.all_cases(), key=lambda n: (size(n), n))
    return names[:len(names) // 2]


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_dirty_memory_changes_nothing(byte, tmp_path):
    """a pad word or an odd read's last nibble that is not written shows here"""
    with api.alloc_poison(byte):
        for name in smaller_half() + ["odd_even_both_strands", "seq_offsets"]:
            check_case(name, tmp_path, ties=("strand",))
        pool_parity(40, tmp_path, tie="input", hooks=dict(NP2_MAP_TEST_PIECE="2048", NP2_MAP_TEST_BUDGET="300", NP2_ALIGN_TEST_BUDGET="5000"))


# ---- names ----------------------------------------------------------------------------------------------------------------------
def test_names_of_254_bytes_are_taken_and_longer_or_empty_ones_refused(tmp_path):
    reads = [bytes(ac.cut()), bytes(ac.cut(100, 500)), bytes(ac.rand(400, 77))]
    long_name = "n" * 254
    with np2io.MapIndex([ac.CONTIG], stream=True) as ix:
        ha, hb, _ = both_doors(ix, tmp_path, ["a", long_name, ""], reads, "strand", {})  # (the unmapped read's name is not looked at)
        assert same_handles(ha, hb) and sorted(kept_names(ha[1])) == ["a", long_name]
        for bad in ("n" * 255, ""):
            with pytest.raises(api.Np2Error) as e:
                np2io.Sam.from_reads(pol(), ix, reads, keep_names=True, names=["a", bad, "c"])
            assert e.value.code == -1 and "read 2: QNAME is empty or longer than 254 bytes" in str(e.value)
            if bad:  # the same from a file, and the text door's own message (a file's record without a name is named by its number)
                fa = write_fasta(tmp_path / "bad.fa", ["a", bad, "c"], reads)
                with pytest.raises(api.Np2Error) as e:
                    np2io.Sam.from_reads(pol(), ix, [fa], keep_names=True)
                assert e.value.code == -1 and "read 2: QNAME is empty or longer than 254 bytes" in str(e.value)
                np2io.map_align_files(ix, [fa], tmp_path / "bad.sam")
                with pytest.raises(api.Np2Error) as e:
                    np2io.Sam(pol(), [tmp_path / "bad.sam"], keep_names=True)
                assert e.value.code == -1 and "QNAME is empty or longer than 254 bytes" in str(e.value)
            sam = np2io.Sam.from_reads(pol(), ix, reads, names=["a", bad, "c"])  # without the names nobody looks
            assert sam.stats()["kept"] == 2
            sam.close()
        sam = np2io.Sam.from_reads(pol(), ix, reads, keep_names=True, names=["a", "b", "c"])  # the index and the context still serve
        assert sorted(kept_names(sam.export_names(pol()))) == ["a", "b"]
        sam.close()


# ---- 9. the committed bundle: the first 30, 40 middle and the last 30 of its 574 reads ------------------------------------------
SUBSET = list(range(30)) + list(range(267, 307)) + list(range(544, 574))


def test_bundle_subset_down_to_the_sorted_bam(tmp_path):
    b = bundle()
    reads, names = [b.reads[i] for i in SUBSET], [b.names[i] for i in SUBSET]
    fa = write_fasta(tmp_path / "hifi.fa", names, reads, comment=" some comment")
    with np2io.MapIndex(ASM) as ix:
        mst = np2io.map_align_files(ix, [fa], tmp_path / "out.sam")
        assert (mst["reads"], mst["mapped"]) == (100, 100)
        for tie in np2io.SAM_TIES:
            a = np2io.Sam.from_reads(pol(), ix, [fa], tie=tie, keep_names=True)
            t = np2io.Sam(pol(), [tmp_path / "out.sam"], tie=tie, keep_names=True)
            assert same_handles(held(a), held(t)) and a.stats()["kept"] == 100
            a.write_bam(pol(), tmp_path / f"a.{tie}.bam")
            t.write_bam(pol(), tmp_path / f"t.{tie}.bam")
            for ext in (".bam", ".bam.bai"):
                assert (tmp_path / f"a.{tie}{ext}").read_bytes() == (tmp_path / f"t.{tie}{ext}").read_bytes(), (tie, ext)
            assert a.bam_stream(pol()) == t.bam_stream(pol())
            a.close(), t.close()
        with env(NP2_MAP_TEST_PIECE="4096", NP2_MAP_TEST_BUDGET="20000", NP2_ALIGN_TEST_BUDGET="100000"):
            a = np2io.Sam.from_reads(pol(), ix, [fa, fa], keep_names=True)  # two files, many groups
            assert np2io.map_last_stats()["groups"] > 40
        np2io.map_align_files(ix, [fa, fa], tmp_path / "twice.sam")
        t = np2io.Sam(pol(), [tmp_path / "twice.sam"], keep_names=True)
        assert same_handles(held(a), held(t)) and a.stats()["kept"] == 200
        a.close(), t.close()


# ---- 10. the whole bundle through the command line -------------------------------------------------------------------------------
def run(module, *args):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd." + module] + [str(a) for a in args], capture_output=True, text=True, env=ENV,
                          timeout=600, stdin=subprocess.DEVNULL)


def test_whole_bundle_from_reads_equals_map_a_then_cli(tmp_path):
    b = bundle()
    fa = tmp_path / "hifi.fa.gz"
    with gzip.open(fa, "wt") as f:
        f.write("".join(f">{n}\n{r.decode()}\n" for n, r in zip(b.names, b.reads)))
    yaks = [os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")]
    r = run("map", ASM, fa, "-a", "-o", tmp_path / "map.sam")
    assert r.returncode == 0, r.stderr[-3000:]
    for tie in np2io.SAM_TIES:
        extra = ["--sorted_bam", tmp_path / "x.bam"] if tie == "strand" else []
        r = run("cli", "--from_reads", fa, ASM, *yaks, "-L", "10000", "--sam_tie", tie, "-o", tmp_path / f"a.{tie}.fa", *extra)
        assert r.returncode == 0, r.stderr[-3000:]
        r = run("cli", tmp_path / "map.sam", ASM, *yaks, "-L", "10000", "--sam_tie", tie, "-o", tmp_path / f"b.{tie}.fa")
        assert r.returncode == 0, r.stderr[-3000:]
        out = (tmp_path / f"a.{tie}.fa").read_bytes()
        assert out == (tmp_path / f"b.{tie}.fa").read_bytes(), tie
        assert [ln[1:].split()[0] for ln in out.decode().splitlines() if ln.startswith(">")] == b.tnames
    r = run("samsort", tmp_path / "map.sam", "-o", tmp_path / "y.bam")
    assert r.returncode == 0, r.stderr[-3000:]
    for ext in (".bam", ".bam.bai"):
        assert (tmp_path / ("x" + ext)).read_bytes() == (tmp_path / ("y" + ext)).read_bytes(), ext


# ---- 11. refusals leave the index and the context usable --------------------------------------------------------------------------
def test_refusals_leave_the_index_and_the_context_usable():
    import ctypes as C
    reads = [bytes(ac.cut())]
    L = np2io._bind()
    with np2io.MapIndex([ac.CONTIG], stream=True) as ix:
        s = np.frombuffer(reads[0] + b"\n", np.uint8)
        o, ao, so, h = np2io.map_opts(), np2io.align_opts(), np2io.np2_sam_opts_t(1), C.c_void_p()
        rc = L.np2_sam_from_read_bytes(pol()._h, ix._h, s.ctypes.data, len(s), 1, None, C.byref(o), C.byref(ao), C.byref(so),
                                       np2io.NP2_SAM_KEEP_ALL, C.byref(h))
        assert rc == -4 and not h.value and b"samsort --full" in L.np2_io_last_error() and b"map -a -o map.sam.gz" in L.np2_io_last_error()
        rc = L.np2_sam_from_read_bytes(pol()._h, ix._h, s.ctypes.data, len(s), 1, None, C.byref(o), C.byref(ao), C.byref(so), 8, C.byref(h))
        assert rc == -1 and b"unknown flag" in L.np2_io_last_error()
        with pytest.raises(api.Np2Error) as e:  # option errors are the aligner's, and come first
            np2io.Sam.from_reads(pol(), ix, reads, band=2000)
        assert e.value.code == -1 and "band" in str(e.value)
        with pytest.raises(api.Np2Error) as e:
            np2io.Sam.from_reads(pol(), ix, [os.path.join(BUNDLE, "no_such_reads.fa")])
        assert e.value.code == -1 and "cannot open" in str(e.value)
        sam = np2io.Sam.from_reads(pol(), ix, reads)  # the same index and context still serve a good call
        assert sam.stats()["kept"] == 1 and sam.export(pol())[0]["l_seq"].tolist() == [600]
        sam.close()


def test_an_index_on_another_device_than_the_context_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("an index on another device than the context needs two devices")
    reads = [bytes(ac.cut())]
    other = Polisher([], device=1)
    with np2io.MapIndex([ac.CONTIG], stream=True) as ix:
        with pytest.raises(api.Np2Error) as e:
            np2io.Sam.from_reads(other, ix, reads)
        assert e.value.code == -1 and "another device" in str(e.value)
        sam = np2io.Sam.from_reads(pol(), ix, reads)  # the same index still serves a good call
        assert sam.stats()["kept"] == 1
        sam.close()
    other.close()


def test_an_index_with_a_repeated_name_is_refused():
    with np2io.MapIndex([ac.CONTIG, pc.CONTIG2], stream=True, names=["c", "c"]) as ix:
        with pytest.raises(api.Np2Error) as e:
            np2io.Sam.from_reads(pol(), ix, [bytes(ac.cut())])
        assert e.value.code == -1 and "given twice" in str(e.value)
