"""The mapper without a GPU (include/np2_io.h: np2_map_*): the numpy model of the rule (tests/map_model.py) on the known answers
of the committed bundle and of a synthetic assembly with an exact repeat, the host mapper np2_map_host (which runs the rule's
one text, csrc/np2_map_core.hpp) against the model field for field on the edge cases of tests/map_cases.py and on the bundle,
the same text as a stand-alone program with and without the host sanitizers, the refusals with their statuses and messages,
and the ABI list."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_cases as mc
import map_model as mm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from nextpolish2_amd import map as np2map

HERE = os.path.dirname(os.path.abspath(__file__))
ASM = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
BAM = os.path.join(HERE, "golden", "ref_bundle", "hifi.map.sort.bam")
E_ARG, E_UNSUPPORTED = -1, -4


# ---- shared, computed once: the bundle and the synthetic case through the model -----------------------------------------------
class Bundle:
    def __init__(self):
        self.contigs = mm.split_stream(np2io.seqfile_stream(ASM))
        self.tnames, _ = np2io.seqfile_reads(ASM)
        self.refs, self.recs, self.reads, self.names, self.ends = mm.bundle_reads(BAM)
        self.index = mm.Index(self.contigs)
        self.hits, self.chains, self.tot = mm.map_reads(self.index, self.reads)
        self.paf = mm.paf(self.names, self.hits, self.tnames, [len(c) for c in self.contigs])


class Synthetic:
    def __init__(self):
        self.contigs, self.cases = mm.synthetic()
        self.reads = [c["read"] for c in self.cases]
        self.index = mm.Index(self.contigs)
        self.hits, self.chains, self.tot = mm.map_reads(self.index, self.reads)


_SHARED = {}


def bundle():
    if "bundle" not in _SHARED:
        _SHARED["bundle"] = Bundle()
    return _SHARED["bundle"]


def synthetic():
    if "synthetic" not in _SHARED:
        _SHARED["synthetic"] = Synthetic()
    return _SHARED["synthetic"]


# ---- 1. the model's known answers --------------------------------------------------------------------------------------------
def test_model_bundle_known_answer():
    b = bundle()
    assert len(b.reads) == 574 and b.index.n_minimizers == 10008
    assert b.tot["mapped"] == 574 and b.tot["unmapped"] == 0
    o = mm.opts()
    start_slack = end_slack = 0
    for h, rc, end in zip(b.hits, b.recs, b.ends):
        assert h["rev"] == (1 if rc["flag"] & 16 else 0) and h["tid"] == rc["tid"]
        assert rc["pos"] <= h["ts"] < h["te"] <= end
        start_slack, end_slack = max(start_slack, h["ts"] - rc["pos"]), max(end_slack, end - h["te"])
    assert (start_slack, end_slack) == (65, 80)
    assert min(h["n"] for h in b.hits) == 12
    assert max(len(mm.anchors(b.index, r, o)[2]) for r in b.reads) == 2050
    assert min(h["mapq"] for h in b.hits) == 32 and sum(h["mapq"] == 60 for h in b.hits) == 125


def test_model_synthetic_known_answer():
    s = synthetic()
    w = 19
    kinds = {"clear": 0, "inside": 0, "into": 0}
    for c, h in zip(s.cases, s.hits):
        assert h is not None and h["tid"] == c["tid"] and h["rev"] == int(c["rev"])
        kinds[c["kind"]] += 1
        lead, trail = (h["qlen"] - h["qe"], h["qs"]) if c["rev"] else (h["qs"], h["qlen"] - h["qe"])
        if c["kind"] == "clear":
            assert h["ts"] - lead == c["origin"] and lead < w and trail < w
            assert h["s2"] == 0 and h["mapq"] == 60
        elif c["kind"] == "inside":
            assert h["s1"] == h["s2"] and h["mapq"] == 0
            assert 6000 <= h["ts"] < h["te"] <= 9000  # the first copy
        else:
            assert 0 < h["mapq"] < 60 and h["ts"] - lead == c["origin"]
    assert kinds == {"clear": 48, "inside": 4, "into": 2}


def test_model_cases_reach_the_edges_they_are_built_for():
    hits = mc.expected("read_length")[0]
    assert [h is not None for h in hits] == [True, False, True] * 3 and all(h["n"] == 1 for h in hits if h)
    for name in ("bandwidth", "max_gap"):  # the gap at the limit is chained across, one base more is not
        contigs, reads, _ = mc.case(name)
        hits = mc.expected(name)[0]
        assert hits[0]["te"] - hits[0]["ts"] == len(contigs[0]) and hits[2]["te"] - hits[2]["ts"] == len(contigs[0])
        assert hits[1]["te"] - hits[1]["ts"] == 300 and hits[3]["te"] - hits[3]["ts"] == 300
    # a predecessor exactly `lookback` back is taken, and one more place of look-back changes the result
    assert mc.expected("lookback_2")[3]["at_lookback"] > 0 and mc.expected("lookback_3")[3]["at_lookback"] > 0
    assert mc.expected("lookback_2")[0] != mc.expected("lookback_3")[0] != mc.expected("lookback_64")[0]
    assert mc.expected("equal_hashes")[3]["ties"] > 0 and mc.expected("k20_palindrome")[3]["ties"] > 0
    tot = mc.expected("occ_cut")[2]
    assert tot["dropped_occ"] > 0 and mc.expected("occ_cut")[0][0] is not None and mc.expected("occ_cut")[0][1] is None
    tot = mc.expected("unmapped")[2]
    assert tot["unmapped"] == 5 and tot["mapped"] == 3
    # the palindrome is met: a k-mer with fw == rv inside a window
    ok, h, _ = mm.kmers(mc.case("k20_palindrome")[0][0], 20)
    assert np.count_nonzero(h[ok] == mm._INF) >= 3


# ---- 2. np2_map_host against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_host_mapper_equals_the_model(name):
    contigs, reads, o = mc.case(name)
    hits, chains, tot, _ = mc.expected(name)
    gh, gc, go = np2io.map_host(contigs, reads, chains=True, **o)
    mc.check(gh, gc, go, hits, chains, reads)
    st = np2io.map_last_stats()
    assert {f: st[f] for f in tot} == tot and st["reads"] == len(reads)
    assert np.array_equal(np2io.map_host(contigs, reads, **o), gh)  # (without the chains)


def test_host_mapper_equals_the_model_on_the_bundle_and_the_synthetic_case():
    for s in (bundle(), synthetic()):
        gh, gc, go = np2io.map_host(s.contigs, s.reads, chains=True)
        mc.check(gh, gc, go, s.hits, s.chains, s.reads)
        st = np2io.map_last_stats()
        assert {f: st[f] for f in s.tot} == s.tot and st["index_minimizers"] == s.index.n_minimizers


# ---- 3. the rule's text as a stand-alone program ------------------------------------------------------------------------------
def core_output(name):
    contigs, reads, o = mc.case(name)
    hits, chains, tot, _ = mc.expected(name)
    ix = mm.Index(contigs, o.get("k", 19), o.get("w", 19))
    lines = ["%d %d %d %d" % (tot["minimizers"], tot["anchors"], tot["dropped_occ"], ix.n_minimizers)]
    for rd, h, c in zip(reads, hits, chains):
        lines.append(" ".join(str(h[f]) for f in mm.HIT_FIELDS) if h else "-1 %d 0 0 0 0 0 0 0 0 0 0 0" % len(rd))
        lines.append(" ".join("%d:%d" % (r, q) for r, q in c))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_core_program_matches_the_model(tmp_path, flags):
    exe = str(tmp_path / "map_core_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "tools", "map_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("read_length", "broken_runs", "k20_palindrome", "k11", "k28", "w1", "w64", "equal_hashes", "occ_cut", "max_gap",
                 "lookback_3", "unmapped"):
        contigs, reads, o = mc.case(name)
        o = mm.opts(**o)
        (tmp_path / "asm").write_bytes(b"".join(c + b"\n" for c in contigs))
        (tmp_path / "reads").write_bytes(b"".join(c + b"\n" for c in reads))
        r = subprocess.run([exe, str(tmp_path / "asm"), str(tmp_path / "reads")] + [str(o[f]) for f in mm.DEFAULTS], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-3000:])
        assert r.stdout == core_output(name), name
    r = subprocess.run([exe, str(tmp_path / "asm"), str(tmp_path / "reads"), "29", "19", "200", "64", "10000", "500", "3", "40"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stderr.startswith("unsupported: k")


# ---- 4. refusals, before any device call ---------------------------------------------------------------------------------------
def test_refusals_come_back_as_statuses_with_their_messages(tmp_path):
    asm, reads = b"ACGT" * 30 + b"\n", b"ACGT" * 20 + b"\n"
    for kw, code, word in ((dict(k=10), E_UNSUPPORTED, "k"), (dict(k=29), E_UNSUPPORTED, "k"), (dict(w=0), E_UNSUPPORTED, "w"),
                           (dict(w=65), E_UNSUPPORTED, "w"), (dict(lookback=0), E_UNSUPPORTED, "lookback"),
                           (dict(lookback=65), E_UNSUPPORTED, "lookback"), (dict(max_occ=0), E_ARG, "max_occ"),
                           (dict(max_gap=0), E_ARG, "max_gap"), (dict(bandwidth=1 << 21), E_ARG, "bandwidth"),
                           (dict(min_cnt=1 << 31), E_ARG, "min_cnt")):
        with pytest.raises(api.Np2Error) as e:
            np2io.map_host(asm, reads, **kw)
        assert e.value.code == code and word in str(e.value), kw
        if "k" in kw or "w" in kw:  # the index build checks them too, before it touches a device
            with pytest.raises(api.Np2Error) as e:
                np2io.MapIndex(asm, stream=True, **kw)
            assert e.value.code == code and word in str(e.value), kw
            with pytest.raises(api.Np2Error) as e:
                np2io.MapIndex(ASM, **kw)
            assert e.value.code == code
    with pytest.raises(api.Np2Error) as e:
        np2io.map_host(asm[:-1], reads)
    assert e.value.code == E_ARG and "newline" in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        np2io.map_host(asm, reads[:-1])
    assert e.value.code == E_ARG and "newline" in str(e.value)
    with pytest.raises(TypeError):
        np2io.map_opts(kay=3)

    L = np2io._bind()
    o = np2io.map_opts()
    a = np.frombuffer(asm, np.uint8)
    r = np.frombuffer(reads, np.uint8)
    hits = np.zeros(1, np2io.MAP_HIT_DTYPE)
    pc, off = C.c_void_p(), np.zeros(2, np.uint64)
    assert L.np2_map_host(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, None, hits.ctypes.data, None, None) == E_ARG
    assert b"opts" in L.np2_io_last_error()
    assert L.np2_map_host(a.ctypes.data, len(a), r.ctypes.data, len(r), 2, C.byref(o), hits.ctypes.data, None, None) == E_ARG
    assert b"n_reads" in L.np2_io_last_error()
    assert L.np2_map_host(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, C.byref(o), None, None, None) == E_ARG
    assert L.np2_map_host(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, C.byref(o), hits.ctypes.data, C.byref(pc), None) == E_ARG
    assert b"chain" in L.np2_io_last_error()
    assert L.np2_map_host(None, 4, r.ctypes.data, len(r), 1, C.byref(o), hits.ctypes.data, None, None) == E_ARG
    h = C.c_void_p()
    assert L.np2_map_index_bytes(0, a.ctypes.data, len(a), None, C.byref(o), None) == E_ARG
    assert L.np2_map_index_files(0, None, 0, C.byref(o), C.byref(h)) == E_ARG and h.value is None
    assert L.np2_map_bytes(None, r.ctypes.data, len(r), 1, C.byref(o), hits.ctypes.data, None, None) == E_ARG
    assert b"index" in L.np2_io_last_error()
    assert L.np2_map_files(None, None, 0, C.byref(o), b"x", None) == E_ARG
    assert L.np2_map_last_stats(None) == E_ARG
    L.np2_map_index_free(None)
    # the thread's next call works
    assert int(np2io.map_host(asm, reads, min_cnt=1, min_score=1)[0]["qlen"]) == 80


def test_abi_symbols_are_listed():
    L = api.lib()
    for s in ("np2_map_index_bytes", "np2_map_index_files", "np2_map_index_free", "np2_map_index_info", "np2_map_index_seq", "np2_map_bytes",
              "np2_map_files", "np2_map_host", "np2_map_last_stats"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)


# ---- 5. the module's device-free helpers ----------------------------------------------------------------------------------------
def test_command_line_helpers():
    a = np2map.build_parser().parse_args(["asm.fa", "r1.fa", "r2.fq.gz", "-o", "x.paf.gz", "-k", "21", "--max_occ", "50"])
    assert (a.asm, a.reads, a.out, a.k, a.w, a.max_occ, a.min_score) == ("asm.fa", ["r1.fa", "r2.fq.gz"], "x.paf.gz", 21, 19, 50, 40)
    st = dict(reads=3, mapped=2, unmapped=1, minimizers=40, anchors=55, dropped_occ=1, index_minimizers=10008, pieces=1, groups=1,
              sketch_ms=0.5, seed_ms=0.25, sort_ms=1.0, chain_ms=2.0, read_ms=4.0, write_ms=0.125)
    head, row = np2map.stats_row(st, 3.125).splitlines()
    assert head.split("\t") == list(np2map.STATS_HEADER)
    assert row.split("\t") == ["3", "2", "1", "40", "55", "1", "10008", "1", "1", "3.125", "0.500", "0.250", "1.000", "2.000", "4.000", "0.125"]
    hit = dict(tid=0, qlen=100, qs=2, qe=98, rev=1, ts=10, te=107, matches=60, block=97, mapq=60, n=5, s1=70, s2=0)
    assert mm.paf_line("r/1", hit, "ctg", 5000) == "r/1\t100\t2\t98\t-\tctg\t5000\t10\t107\t60\t97\t60\ttp:A:P\tcm:i:5\ts1:i:70\ts2:i:0\n"
