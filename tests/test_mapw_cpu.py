"""The weighted mapper (winnowmap -W; include/np2_io.h: np2_map_*, "Weights") without a GPU: the numpy model of the weighted
window order (tests/mapw_model.py) on the edges of tests/mapw_cases.py and on the tandem-array known answer, the host mapper
under weights (np2_map_host_w, np2_map_align_host_w: the rule's one text, csrc/np2_map_core.hpp) against the model field for
field, the same text as a stand-alone program with and without the host sanitizers, the list file's rule, the refusals with
their statuses and messages, the ABI list and the command lines' argument rules."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import align_model as am
import map_cases as mc
import map_model as mm
import mapw_cases as wc
import mapw_model as wm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from nextpolish2_amd import map as np2map
from test_map_cpu import ASM, BAM, bundle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV = dict(os.environ, PYTHONPATH=ROOT)
YAKS = [os.path.join(HERE, "golden", "ref_bundle", f) for f in ("k21.yak", "k31.yak")]
E_ARG, E_UNSUPPORTED = -1, -4
BUNDLE_K, BUNDLE_MIN_COUNT = 15, 1  # the bundle's list: 15-mers met more than once in its 100 kb assembly


class WeightedBundle:
    """the committed bundle's reads against its assembly under a --rep min_count=1 style list, through the model"""

    def __init__(self):
        b = bundle()
        self.contigs, self.reads, self.names, self.tnames = b.contigs, b.reads, b.names, b.tnames
        self.L = wc.listed_of(self.contigs, BUNDLE_K, BUNDLE_MIN_COUNT)
        self.index = wm.Index(self.contigs, BUNDLE_K, 19, self.L)
        self.hits, self.chains, self.tot = wm.map_reads(self.index, self.reads, self.L)
        self.paf = mm.paf(self.names, self.hits, self.tnames, [len(c) for c in self.contigs])


_SHARED = {}


def weighted_bundle():
    if "b" not in _SHARED:
        _SHARED["b"] = WeightedBundle()
    return _SHARED["b"]


def weights_of(name):
    c = wc.case(name)
    return np2io.MapWeights(c["L"], k=c["o"]["k"])


# ---- 1. the model: edges and known answers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_model_case_reaches_the_edge_it_is_built_for(name):
    wc.EDGES[name](wc.case(name))
    k = wc.case(name)["o"]["k"]
    assert all(v <= wm.revcomp_index(v, k) for v in wc.case(name)["L"])  # canonical indices


def test_model_key_by_hand():
    k, M = 11, (1 << 22) - 1
    for h in (0, 1, 12345, M // 2, M - 1, M, M - (1 << 19), M - 700000):
        y = M - h
        for _ in range(3):
            y = (y * y) >> 22
        assert int(wm.key_of(np.array([h], np.uint64), np.array([True]), k)[0]) == M - y
        assert int(wm.key_of(np.array([h], np.uint64), np.array([False]), k)[0]) == h
    assert int(wm.key_of(np.array([0], np.uint64), np.array([True]), k)[0]) == 7  # y = M: each squaring loses a little under M
    assert int(wm.key_of(np.array([M - (1 << 19)], np.uint64), np.array([True]), k)[0]) == M  # y8 == 0
    h = np.arange(0, M, 997, dtype=np.uint64)
    key = wm.key_of(h, np.ones(len(h), bool), k)
    assert (key >= h).all() and (np.diff(key.astype(np.int64)) >= 0).all()  # a listed k-mer never gains; the order is kept


def test_model_w1_and_the_empty_set_change_nothing():
    c = wc.case("w1")
    (h1, c1, t1, n1), (h0, c0, t0, n0) = wc.expected("w1"), wc.expected("w1", False)
    assert h1 == h0 and t1 == t0 and n1 == n0 and all(np.array_equal(a, b) for a, b in zip(c1, c0))
    assert wm.Index(c["contigs"], 15, 1, []).n_minimizers == mm.Index(c["contigs"], 15, 1).n_minimizers == n1


def test_model_tandem_array_known_answer():
    c = wc.case("tandem")
    plain, weighted = wc.expected("tandem", False)[0], wc.expected("tandem")[0]
    for hits in (plain, weighted):  # every read maps to its origin either way
        for i, (h, at) in enumerate(zip(hits, c["origins"])):
            assert h is not None and h["rev"] == i % 2 and at <= h["ts"] < h["te"] <= at + 3000
    q30 = tuple(sum(h["mapq"] >= 30 for h in hits) for hits in (plain, weighted))
    q60 = tuple(sum(h["mapq"] == 60 for h in hits) for hits in (plain, weighted))
    assert q30 == wc.TANDEM_MAPQ30 and q30[1] > q30[0]
    assert q60 == wc.TANDEM_MAPQ60 and q60[1] > q60[0]
    for max_occ in (50,):  # the same under a lower occurrence cut
        kw = dict(max_occ=max_occ)
        p = wm.map_reads(wm.Index(c["contigs"], 15, 19, []), c["reads"], [], **kw)[0]
        w = wm.map_reads(wm.Index(c["contigs"], 15, 19, c["L"]), c["reads"], c["L"], **kw)[0]
        assert sum(h["mapq"] == 60 for h in w) > sum(h["mapq"] == 60 for h in p)


def test_model_bundle_under_weights():
    b = weighted_bundle()
    assert len(b.L) > 0 and b.tot["mapped"] == 574
    assert b.index.n_minimizers != mm.Index(b.contigs, BUNDLE_K, 19).n_minimizers  # the weights move minimizers


# ---- 2. np2_map_host_w and np2_map_align_host_w against the model -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_host_mapper_equals_the_model(name):
    c = wc.case(name)
    hits, chains, tot, n_index = wc.expected(name)
    with weights_of(name) as W:
        assert (W.k, W.n_listed) == (c["o"]["k"], len(c["L"]))
        gh, gc, go = np2io.map_host(c["contigs"], c["reads"], chains=True, weights=W, **c["o"])
        st = np2io.map_last_stats()
        mc.check(gh, gc, go, hits, chains, c["reads"])
        assert {f: st[f] for f in tot} == tot and st["reads"] == len(c["reads"]) and st["index_minimizers"] == n_index
        assert np.array_equal(np2io.map_host(c["contigs"], c["reads"], weights=W, **c["o"]), gh)  # (without the chains)


@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_host_aligner_under_weights_equals_the_model(name):
    c = wc.case(name)
    hits, chains, tot, _ = wc.expected(name)
    _, recs, cigars, cnt = am.align_mapped(c["contigs"], c["reads"], hits, chains, c["o"]["k"])
    with weights_of(name) as W:
        gh, gr, gc, go = np2io.map_align_host(c["contigs"], c["reads"], weights=W, **c["o"])
    mc.check(gh, None, None, hits, chains, c["reads"])
    have = np.array([[int(r[f]) for f in am.REC_FIELDS] for r in gr], np.int64).reshape(len(recs), len(am.REC_FIELDS))
    assert np.array_equal(have, am.recs_array(recs))
    words, off = am.cigar_words(cigars)
    assert np.array_equal(go, off) and np.array_equal(gc, words)
    st = np2io.align_last_stats()
    assert {f: st[f] for f in cnt} == cnt


def test_host_mapper_equals_the_model_on_the_bundle():
    b = weighted_bundle()
    with np2io.MapWeights(b.L, k=BUNDLE_K) as W:
        gh, gc, go = np2io.map_host(b.contigs, b.reads, chains=True, weights=W, k=BUNDLE_K)
    mc.check(gh, gc, go, b.hits, b.chains, b.reads)
    st = np2io.map_last_stats()
    assert {f: st[f] for f in b.tot} == b.tot and st["index_minimizers"] == b.index.n_minimizers


def test_the_empty_set_and_null_are_the_plain_calls():
    contigs, cases = mm.synthetic()
    reads = [c["read"] for c in cases]
    want = np2io.map_host(contigs, reads, chains=True)
    with np2io.MapWeights([], k=15) as W:  # (kw = 0: it fits the default k = 19)
        assert (W.k, W.n_listed) == (0, 0)
        got = np2io.map_host(contigs, reads, chains=True, weights=W)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        a, b = np2io.map_align_host(contigs, reads, weights=W), np2io.map_align_host(contigs, reads)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    L = np2io._bind()
    o = np2io.map_opts()
    s, n = np2io._stream_of(contigs)
    r, nr = np2io._stream_of(reads)
    hits = np.zeros(nr, np2io.MAP_HIT_DTYPE)
    assert L.np2_map_host_w(s.ctypes.data, len(s), r.ctypes.data, len(r), nr, C.byref(o), None, hits.ctypes.data, None, None) == 0
    assert np.array_equal(hits, want[0])


def test_the_weights_of_a_case_w1_change_no_hit():
    c = wc.case("w1")
    with weights_of("w1") as W:
        a = np2io.map_host(c["contigs"], c["reads"], chains=True, weights=W, **c["o"])
    b = np2io.map_host(c["contigs"], c["reads"], chains=True, **c["o"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 3. the rule's text as a stand-alone program ------------------------------------------------------------------------------
def model_words(seq, k, L):
    """the words of a sequence's first 64 bytes as np2map::push / push_w define them"""
    ok, v, h, strand = wm.kmers_v(seq, k)
    M = (1 << (2 * k)) - 1
    Ls = set(L)
    out = []
    for i in range(min(64, len(seq))):
        if not ok[i]:
            out.append((1 << 64) - 1)
        elif h[i] == mm._INF:
            out.append((1 << 64) - 2)
        else:
            hi = int(h[i])
            key = int(wm.key_of(np.array([hi], np.uint64), np.array([int(v[i]) in Ls]), k)[0])
            out.append((key << (2 * k + 1) | hi << 1 | int(strand[i])) if L else (hi << 1 | int(strand[i])))
    assert all(x <= M << (2 * k + 1) | M << 1 | 1 for x in out if x < (1 << 64) - 2)
    return " ".join("%x" % x for x in out)


def core_output(name, weighted=True):
    c = wc.case(name)
    hits, chains, tot, n_index = wc.expected(name, weighted)
    k, w = c["o"]["k"], c["o"]["w"]
    L = c["L"] if weighted else []
    ix = wm.Index(c["contigs"], k, w, L)
    lines = ["%d %d %d %d" % (tot["minimizers"], tot["anchors"], tot["dropped_occ"], n_index)]
    lines += ["%d %d %d %d" % (h, t, p, s) for h, t, p, s in zip(ix.h.tolist(), ix.tid.tolist(), ix.pos.tolist(), ix.strand.tolist())]
    lines.append(model_words(c["contigs"][0], k, L))
    for rd, h, ch in zip(c["reads"], hits, chains):
        lines.append(" ".join(str(h[f]) for f in mm.HIT_FIELDS) if h else "-1 %d 0 0 0 0 0 0 0 0 0 0 0" % len(rd))
        lines.append(" ".join("%d:%d" % (r, q) for r, q in ch))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_core_program_matches_the_model(tmp_path, flags):
    exe = str(tmp_path / "mapw_core_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "tools", "mapw_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for name, weighted in [(n, True) for n in sorted(wc.CASES) if n != "tandem"] + [("tile_edges", False)]:
        c = wc.case(name)
        o = mm.opts(**c["o"])
        (tmp_path / "asm").write_bytes(b"".join(x + b"\n" for x in c["contigs"]))
        (tmp_path / "reads").write_bytes(b"".join(x + b"\n" for x in c["reads"]))
        (tmp_path / "list").write_text("".join("%d\n" % v for v in c["L"]) if weighted else "")
        r = subprocess.run([exe, str(tmp_path / "asm"), str(tmp_path / "reads"), str(tmp_path / "list")] + [str(o[f]) for f in mm.DEFAULTS],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-3000:])
        assert r.stdout == core_output(name, weighted), name
    r = subprocess.run([exe, str(tmp_path / "asm"), str(tmp_path / "reads"), str(tmp_path / "list"), "16", "19", "200", "64", "10000", "500", "3",
                        "40"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0  # (the last list written is empty: k = 16 maps unweighted)
    (tmp_path / "list").write_text("5\n")
    r = subprocess.run([exe, str(tmp_path / "asm"), str(tmp_path / "reads"), str(tmp_path / "list"), "16", "19", "200", "64", "10000", "500", "3",
                        "40"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stderr.startswith("unsupported: weights")


# ---- 4. the list file ----------------------------------------------------------------------------------------------------------
def test_list_file_forms(tmp_path):
    name = "one_unlisted_k15_w19"
    c = wc.case(name)
    k, L = c["o"]["k"], c["L"]
    texts = {f: wc.list_text(name, f) for f in ("fw", "rc", "both")}
    fw = texts["fw"].split("\n")[:-1]
    texts["counts_crlf"] = "".join(f"{x}\t{i + 7}\r\n" for i, x in enumerate(fw))
    texts["lower_u"] = "".join(x.lower().replace("t", "u" if i % 2 else "U") + "\n" for i, x in enumerate(fw))
    texts["twice_no_last_newline"] = (texts["fw"] + texts["fw"])[:-1]
    texts["mixed"] = fw[0] + "\n" + fw[1] + "\tsome words, N included\n" + "".join(x + "\r\n" for x in fw[2:])
    hits = wc.expected(name)[0]
    for form, text in texts.items():
        p = tmp_path / (form + ".txt")
        p.write_bytes(text.encode())
        assert wm.parse_list(text.encode()) == (k, L), form
        with np2io.MapWeights(p) as W:
            assert (W.k, W.n_listed) == (k, len(L)), form
            gh = np2io.map_host(c["contigs"], c["reads"], weights=W, **c["o"])
        mc.check(gh, None, None, hits, None, c["reads"])
        assert np2map.list_k(p) == k
    gz = tmp_path / "list.txt.gz"
    with gzip.open(gz, "wb") as f:
        f.write(texts["counts_crlf"].encode())
    with np2io.MapWeights(gz) as W:
        assert (W.k, W.n_listed) == (k, len(L))
    assert np2map.list_k(gz) == k and wm.parse_list(gz.read_bytes()) == (k, L)
    empty = tmp_path / "empty.txt"
    empty.write_bytes(b"")
    with np2io.MapWeights(empty) as W:
        assert (W.k, W.n_listed) == (0, 0)
    assert np2map.list_k(empty) == 0 and wm.parse_list(b"") == (0, [])


def test_list_file_refusals_name_the_line(tmp_path):
    good = "ACGTACGTACGTACG"
    for text, line, word in ((f"{good}\n{good}\nACGTACGTNCGTACG\n", 3, "letter"), (f"{good}\r\n{good[:-1]}\r\n{good}\n", 2, "letters"),
                             (f"{good}\n{good}A\t3\n", 2, "letters"), (f"{good}\n\n{good}\n", 2, "letters"),
                             (f"{good}\n{good[:7]}\r{good[7:]}\n", 2, "letter"), (f"AC-T\n", 1, "letter")):
        p = tmp_path / "bad.txt"
        p.write_bytes(text.encode())
        with pytest.raises(api.Np2Error) as e:
            np2io.MapWeights(p)
        assert e.value.code == E_ARG and f"line {line}:" in str(e.value) and word in str(e.value), (text, str(e.value))
        with pytest.raises(ValueError) as e2:
            wm.parse_list(text.encode())
        assert f"line {line}:" in str(e2.value)
    with pytest.raises(api.Np2Error) as e:
        np2io.MapWeights(tmp_path / "missing.txt")
    assert e.value.code == E_ARG and "cannot open" in str(e.value)
    (tmp_path / "k16.txt").write_text("ACGTACGTACGTACGT\n")
    with pytest.raises(api.Np2Error) as e:
        np2io.MapWeights(tmp_path / "k16.txt")
    assert e.value.code == E_UNSUPPORTED and "bitmap" in str(e.value)


# ---- 5. refusals, before any device call ---------------------------------------------------------------------------------------
def test_refusals_come_back_as_statuses_with_their_messages():
    asm, reads = b"ACGT" * 30 + b"\n", b"ACGT" * 20 + b"\n"
    with np2io.MapWeights([5, 9, 5], k=15) as W:  # duplicates allowed
        assert (W.k, W.n_listed) == (15, 2)
        for kw in (dict(), dict(k=11), dict(k=16)):  # the options' k is not the list's
            for call in (lambda: np2io.map_host(asm, reads, weights=W, **kw), lambda: np2io.map_align_host(asm, reads, weights=W, **kw),
                         lambda: np2io.MapIndex(asm, stream=True, weights=W, **kw), lambda: np2io.MapIndex(ASM, weights=W, **kw)):
                with pytest.raises(api.Np2Error) as e:
                    call()
                assert e.value.code == E_ARG and "15" in str(e.value) and str(kw.get("k", 19)) in str(e.value), kw
        with pytest.raises(api.Np2Error) as e:  # the options are checked first, as in the plain calls
            np2io.map_host(asm, reads, weights=W, k=10)
        assert e.value.code == E_UNSUPPORTED
    M15 = (1 << 30) - 1
    for k, idx, code, word in ((16, [5], E_UNSUPPORTED, "bitmap"), (10, [5], E_UNSUPPORTED, "11 <= k <= 15"), (15, [M15 + 1], E_ARG, "beyond"),
                               (11, [1 << 22], E_ARG, "beyond"), (15, [M15], E_ARG, "canonical"),
                               (15, [3, wm.revcomp_index(wm.index_of("ACGTACGTACGTACC"), 15)], E_ARG, "index[1]")):
        with pytest.raises(api.Np2Error) as e:
            np2io.MapWeights(idx, k=k)
        assert e.value.code == code and word in str(e.value), (k, idx, str(e.value))
    with np2io.MapWeights([], k=16) as W:  # an empty set has no k
        assert (W.k, W.n_listed) == (0, 0)
    with pytest.raises(TypeError):
        np2io.MapWeights([1, 2])
    with pytest.raises(TypeError):
        np2io.map_host(asm, reads, weights=[1, 2])

    L = np2io._bind()
    h, v = C.c_void_p(), np.array([5], np.uint32)
    assert L.np2_map_weights_from_indices(15, v.ctypes.data, 1, None) == E_ARG and b"out" in L.np2_io_last_error()
    assert L.np2_map_weights_from_indices(15, None, 1, C.byref(h)) == E_ARG and h.value is None
    assert L.np2_map_weights_from_file(None, C.byref(h)) == E_ARG and b"path" in L.np2_io_last_error()
    assert L.np2_map_weights_from_file(b"x", None) == E_ARG
    assert L.np2_map_weights_info(None, None, None) == E_ARG
    assert L.np2_map_index_weights(None, None, None) == E_ARG and b"index" in L.np2_io_last_error()
    L.np2_map_weights_free(None)
    o = np2io.map_opts(k=15)
    a, r = np.frombuffer(asm, np.uint8), np.frombuffer(reads, np.uint8)
    hits = np.zeros(1, np2io.MAP_HIT_DTYPE)
    assert L.np2_map_weights_from_indices(15, v.ctypes.data, 1, C.byref(h)) == 0
    try:
        assert L.np2_map_host_w(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, None, h, hits.ctypes.data, None, None) == E_ARG
        assert L.np2_map_host_w(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, C.byref(o), h, None, None, None) == E_ARG
        assert L.np2_map_host_w(a.ctypes.data, len(a), r.ctypes.data, len(r), 2, C.byref(o), h, hits.ctypes.data, None, None) == E_ARG
        assert b"n_reads" in L.np2_io_last_error()
        assert L.np2_map_index_bytes_w(0, a.ctypes.data, len(a), None, C.byref(o), h, None) == E_ARG
        ix = C.c_void_p()
        assert L.np2_map_index_files_w(0, None, 0, C.byref(o), h, C.byref(ix)) == E_ARG and ix.value is None
        ao = np2io.align_opts()
        recs = np.zeros(1, np2io.ALIGN_REC_DTYPE)
        assert L.np2_map_align_host_w(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, C.byref(o), C.byref(ao), h, None, None, None, None) == E_ARG
        assert b"recs" in L.np2_io_last_error()
        assert L.np2_map_align_host_w(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, C.byref(o), None, h, None, recs.ctypes.data, None, None) == E_ARG
        # the thread's next call works
        assert L.np2_map_host_w(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, C.byref(o), h, hits.ctypes.data, None, None) == 0
        assert int(hits[0]["qlen"]) == 80
    finally:
        L.np2_map_weights_free(h)


def test_abi_symbols_are_listed():
    L = api.lib()
    for s in ("np2_map_weights_from_indices", "np2_map_weights_from_file", "np2_map_weights_info", "np2_map_weights_free",
              "np2_map_index_bytes_w", "np2_map_index_files_w", "np2_map_index_weights", "np2_map_host_w", "np2_map_align_host_w"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)


# ---- 6. the command lines' argument rules (no device: every one ends before the library loads) ------------------------------------
def run(module, *args):
    return subprocess.run([sys.executable, "-m", module] + [str(a) for a in args], capture_output=True, text=True, env=ENV, timeout=600)


def test_map_command_line_argument_rules(tmp_path):
    P = np2map.build_parser()
    a = P.parse_args(["asm.fa", "r.fa"])
    assert (a.k, a.w, a.weights, a.rep) == (None, 19, None, None)
    a = P.parse_args(["asm.fa", "r.fa", "-W", "list.txt", "-w", "50"])
    assert (a.k, a.w, a.weights, a.rep) == (None, 50, "list.txt", None)
    assert P.parse_args(["asm.fa", "r.fa", "--rep"]).rep == dict(distinct=0.9998)
    assert P.parse_args(["asm.fa", "--rep", "min_count=10", "r.fa"]).rep == dict(min_count=10)
    assert P.parse_args(["asm.fa", "r.fa", "--rep", "distinct=0.5"]).rep == dict(distinct=0.5)
    assert np2map.resolve_k(None, 0, 19) == (19, None) and np2map.resolve_k(None, 15, 19) == (15, None)
    assert np2map.resolve_k(15, 15, 19) == (15, None) and np2map.resolve_k(21, 0, 19) == (21, None)
    k, bad = np2map.resolve_k(19, 15, 19)
    assert "19" in bad and "15" in bad
    lst = tmp_path / "k15.txt"
    lst.write_text("ACGTACGTACGTACG\t12\n")
    r = run("nextpolish2_amd.map", ASM, "reads.fa", "-W", lst, "--rep")
    assert r.returncode == 2 and "not allowed with" in r.stderr
    r = run("nextpolish2_amd.map", ASM, "reads.fa", "--rep", "count=3")
    assert r.returncode == 2 and "min_count=N" in r.stderr
    r = run("nextpolish2_amd.map", ASM, "reads.fa", "--rep", "distinct=1.5")
    assert r.returncode == 2
    r = run("nextpolish2_amd.map", ASM, "reads.fa", "-W", lst, "-k", "19")
    assert r.returncode != 0 and "contradicts" in r.stderr and "15" in r.stderr and "Traceback" not in r.stderr
    r = run("nextpolish2_amd.map", ASM, "reads.fa", "-W", tmp_path / "missing.txt")
    assert r.returncode != 0 and "-W" in r.stderr and "Traceback" not in r.stderr
    head, row = np2map.stats_row(dict.fromkeys(np2map.STATS_HEADER, 1), 2.0, (15, 171)).splitlines()
    assert head.split("\t") == list(np2map.STATS_HEADER) + ["weights_k", "weights_listed"] and row.split("\t")[-2:] == ["15", "171"]


def test_polish_command_line_argument_rules(tmp_path):
    lst = tmp_path / "k15.txt"
    lst.write_text("ACGTACGTACGTACG\n")
    r = run("nextpolish2_amd.cli", BAM, ASM, *YAKS, "--map_weights", "auto")
    assert r.returncode == 2 and "--map_weights goes with --from_reads" in r.stderr
    r = run("nextpolish2_amd.cli", "--from_reads", ASM, ASM, *YAKS, "--map_weights", lst, "--map_opts", "k=19,w=50")
    assert r.returncode != 0 and "contradicts" in r.stderr and "--map_opts k=19" in r.stderr and "Traceback" not in r.stderr
    r = run("nextpolish2_amd.cli", "--from_reads", ASM, ASM, *YAKS, "--map_weights", tmp_path / "missing.txt")
    assert r.returncode != 0 and "--map_weights" in r.stderr and "Traceback" not in r.stderr
