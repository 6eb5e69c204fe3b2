"""The repetitive k-mer list without a GPU: the numpy model of the rule (tests/rep_model.py) on hand-derived streams and on
the committed assembly, the per-lane core as a one-lane host program (csrc/np2_rep_core.hpp through
tests/tools/rep_core_test.cpp) against the model, the entry points' argument checks (which come before any device call) and
the module's text helpers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import rep_model as rm
from nextpolish2_amd import api, repkmers
from nextpolish2_amd import io as np2io

HERE = os.path.dirname(os.path.abspath(__file__))
ASM = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
E_ARG, E_UNSUPPORTED = -1, -4

# (stream, k, expected {index: count}), every count derived by hand
#   k = 3: ACG = 0b000110 = 6, its reverse complement CGT = 27 -> 6
#   k = 2: AA = 0 (TT = 15); AC = 1 (GT = 11); CG = 6 is its own reverse complement
#   k = 4: ACGT = 27 and GTAC = 177 are their own reverse complements; CGTA = 108, its reverse complement TACG = 198
HAND = {
    "separator_inside": (b"AC\nGT", 3, {}),
    "separator_between": (b"ACG\nCGT", 3, {6: 2}),
    "lower_case_and_u": (b"acgu", 3, {6: 2}),
    "n_ends_the_run": (b"AANAA", 2, {0: 2}),
    "high_byte_ends_the_run": (b"AA\xc1AA\xe1AA", 2, {0: 3}),
    "palindrome_k2": (b"ACGT", 2, {1: 2, 6: 1}),
    "palindrome_k4": (b"ACGTACGT", 4, {27: 2, 108: 2, 177: 1}),
    "shorter_than_k": (b"ACG", 4, {}),
    "empty": (b"", 2, {}),
}


@pytest.fixture(scope="module")
def asm_stream():
    return np2io.seqfile_stream(ASM)


@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rep") / "rep_core_test")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "tools", "rep_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


# ---- 1. the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_model_counts_hand_derived_streams(name):
    stream, k, exp = HAND[name]
    index, count, st = rm.rep(stream, k, min_count=0)
    assert dict(zip(index.tolist(), count.tolist())) == exp
    assert st["kmers"] == sum(exp.values()) and st["distinct"] == len(exp) and st["threshold"] == 0
    assert st["max_count"] == max(exp.values(), default=0) and st["listed"] == len(exp)


def test_model_threshold_rule_by_hand():
    stream, k, _ = HAND["palindrome_k4"]  # counts 2, 2, 1: D = 3
    # f = 0: target 0, the smallest occurring count, 1; the two k-mers counted twice are listed
    index, count, st = rm.rep(stream, k, distinct=0.0)
    assert st["threshold"] == 1 and index.tolist() == [27, 108] and count.tolist() == [2, 2] and st["listed_occurrences"] == 4
    # f = 0.5: target (int)1.5 = 1, cum(1) = 1 reaches it
    assert rm.rep(stream, k, distinct=0.5)[2]["threshold"] == 1
    # f = 0.9998: target (int)2.9994 = 2, cum(1) = 1 < 2 <= cum(2) = 3
    assert rm.rep(stream, k, distinct=0.9998)[2]["threshold"] == 2
    # f = 1: target 3 = D: the largest count, nothing above it
    index, count, st = rm.rep(stream, k, distinct=1.0)
    assert st["threshold"] == 2 and len(index) == 0 and st["listed"] == 0 and st["listed_occurrences"] == 0
    # greater-than N
    index, count, st = rm.rep(stream, k, min_count=1)
    assert st["threshold"] == 1 and index.tolist() == [27, 108]
    # D = 0: threshold 0 and an empty list
    for f in (0.0, 0.9998, 1.0):
        index, count, st = rm.rep(b"AC\nGT", 3, distinct=f)
        assert st == {"kmers": 0, "distinct": 0, "listed": 0, "listed_occurrences": 0, "threshold": 0, "max_count": 0} and len(index) == 0


# k, f -> k-mers, distinct, threshold, listed, occurrences listed, max count
KNOWN = [
    (15, 0.9998, 99986, 95225, 4, 8, 153, 109),
    (15, 0.99, 99986, 95225, 2, 202, 843, 109),
    (11, 0.9998, 99990, 86813, 9, 16, 360, 147),
    (8, 0.9998, 99993, 24658, 66, 5, 577, 203),
    (8, 0.5, 99993, 24658, 3, 9443, 73208, 203),
    (16, 0.9998, 99985, 95463, 4, 6, 126, 52),
    (2, 0.5, 99999, 10, 9642, 5, 71189, 24269),
]


def known_stats(row):
    return dict(zip(("kmers", "distinct", "threshold", "listed", "listed_occurrences", "max_count"), row[2:]))


@pytest.mark.parametrize("row", KNOWN, ids=lambda r: f"k{r[0]}_f{r[1]}")
def test_model_reproduces_the_known_answers_on_the_committed_assembly(asm_stream, row):
    assert rm.rep(asm_stream, row[0], distinct=row[1])[2] == known_stats(row)


def test_model_poly_a_and_min_count_on_the_committed_assembly(asm_stream):
    index, count, st = rm.rep(asm_stream, 15, min_count=1)
    assert st["listed"] == 4322 and st["listed_occurrences"] == 9083 and st["threshold"] == 1
    assert index[0] == 0 and count[0] == 13  # poly-A


# ---- 2. the per-lane core as a host program ----------------------------------------------------------------------------------
def run_core(exe, path, k, distinct=None, min_count=None):
    how = ["min_count", str(min_count)] if min_count is not None else ["distinct", repr(float(distinct))]
    r = subprocess.run([exe, path, str(k)] + how, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    head = [int(x) for x in lines[0].split()]
    rows = [ln.split("\t") for ln in lines[1:]]
    st = dict(zip(("kmers", "distinct", "threshold", "listed", "listed_occurrences", "max_count"), head))
    return [int(x[0]) for x in rows], [int(x[1]) for x in rows], [x[2] for x in rows], st


def same_as_model(exe, path, stream, k, **kw):
    gi, gc, gt, gst = run_core(exe, path, k, **kw)
    mi, mc, mst = rm.rep(stream, k, **kw)
    assert gst == mst and gi == mi.tolist() and gc == mc.tolist()
    assert "".join(f"{t}\t{c}\n" for t, c in zip(gt, gc)) == rm.text(mi, mc, k)


def test_core_matches_the_model_on_the_hand_derived_streams(core_exe, tmp_path):
    for name, (stream, k, exp) in HAND.items():
        p = tmp_path / name
        p.write_bytes(stream)
        gi, gc, _, gst = run_core(core_exe, str(p), k, min_count=0)
        assert dict(zip(gi, gc)) == exp and gst["kmers"] == sum(exp.values()), name
        for f in (0.0, 0.5, 0.9998, 1.0):
            same_as_model(core_exe, str(p), stream, k, distinct=f)


def test_core_matches_the_model_on_the_committed_assembly(core_exe, tmp_path, asm_stream):
    p = tmp_path / "asm.stream"
    p.write_bytes(asm_stream)
    for row in KNOWN:
        same_as_model(core_exe, str(p), asm_stream, row[0], distinct=row[1])
        assert run_core(core_exe, str(p), row[0], distinct=row[1])[3] == known_stats(row)
    same_as_model(core_exe, str(p), asm_stream, 15, min_count=1)


def test_core_selects_across_the_two_levels(core_exe, tmp_path):
    """counts of 70 000 and 70 001 share their high half: the program's two-level selection (the driver's) must agree with
    the one-level rule wherever the threshold lands"""
    stream = b"\n".join([b"A" * 70001, b"C" * 70002, b"ACAC"])  # k = 2: AA 70 000, CC 70 001, AC 2, CA 1 (CA = 4, TG = 14)
    p = tmp_path / "runs"
    p.write_bytes(stream)
    index, count, _ = rm.rep(stream, 2, min_count=0)
    assert dict(zip(index.tolist(), count.tolist())) == {0: 70000, 5: 70001, 1: 2, 4: 1}
    for f, thr in ((0.0, 1), (0.5, 2), (0.75, 70000), (1.0, 70001)):
        same_as_model(core_exe, str(p), stream, 2, distinct=f)
        assert rm.rep(stream, 2, distinct=f)[2]["threshold"] == thr


# ---- 3. argument checks that need no device ----------------------------------------------------------------------------------
def test_bad_arguments_come_back_as_status_before_any_device_call(tmp_path):
    for k in (1, 17, 0):
        with pytest.raises(api.Np2Error) as e:
            api.rep_bytes(b"ACGT", k=k)
        assert e.value.code == E_UNSUPPORTED and f"k = {k}" in str(e.value)
        with pytest.raises(api.Np2Error) as e:
            api.rep_files([ASM], str(tmp_path / "out.txt"), k=k)
        assert e.value.code == E_UNSUPPORTED and f"k = {k}" in str(e.value)
    for f in (-0.1, 1.5, math.nan):
        with pytest.raises(api.Np2Error) as e:
            api.rep_bytes(b"ACGT", distinct=f)
        assert e.value.code == E_ARG and "distinct" in str(e.value)
    missing = str(tmp_path / "missing.fa")
    with pytest.raises(api.Np2Error) as e:
        api.rep_files([ASM, missing], str(tmp_path / "out.txt"))
    assert e.value.code == E_ARG and "cannot open" in str(e.value) and missing in str(e.value)
    assert not os.path.exists(tmp_path / "out.txt")
    with pytest.raises(api.Np2Error) as e:
        api.rep_files([ASM], None)
    assert e.value.code == E_ARG and "out_path" in str(e.value)

    L = api.lib()
    o, st = api.np2_rep_opts_t(15, 0, 0, 0.9998), api.np2_rep_stats_t()
    pi, pc, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    buf = np.frombuffer(b"ACGT", dtype=np.uint8)
    assert L.np2_rep_bytes(0, buf.ctypes.data, 4, None, C.byref(pi), C.byref(pc), C.byref(n), C.byref(st)) == E_ARG
    assert b"opts" in L.np2_io_last_error()
    assert L.np2_rep_bytes(0, buf.ctypes.data, 4, C.byref(o), None, C.byref(pc), C.byref(n), C.byref(st)) == E_ARG
    assert b"NULL" in L.np2_io_last_error()
    assert L.np2_rep_bytes(0, None, 4, C.byref(o), C.byref(pi), C.byref(pc), C.byref(n), C.byref(st)) == E_ARG
    assert L.np2_rep_files(0, None, 0, C.byref(o), b"x", 0, C.byref(st)) == E_ARG
    # the thread's next call works
    assert len(np2io.seqfile_stream(ASM)) == 100001


# ---- 4. the module's device-free helpers -------------------------------------------------------------------------------------
def test_index_and_text_round_trip():
    rng = np.random.default_rng(5)
    for k in (2, 15, 16):
        top = 4 ** k
        for v in [0, 1, top - 1, top // 2] + rng.integers(0, top, 50).tolist():
            t = repkmers.kmer_text(v, k)
            assert len(t) == k and set(t) <= set("ACGT") and repkmers.kmer_index(t) == v and repkmers.kmer_index(t.lower()) == v
            rc = repkmers.revcomp_index(v, k)
            assert repkmers.kmer_text(rc, k) == t[::-1].translate(str.maketrans("ACGT", "TGCA"))
            assert repkmers.revcomp_index(rc, k) == v
    assert repkmers.kmer_text(0, 15) == "A" * 15 and repkmers.kmer_text(27, 4) == "ACGT" and repkmers.kmer_index("ACGU") == 27


def test_list_lines_and_stats_row():
    index, count = np.array([6, 27, 108], np.uint32), np.array([5, 70001, 2], np.uint32)
    assert repkmers.list_lines(index, count, 4) == ["AACG\t5\n", "ACGT\t70001\n", "CGTA\t2\n"]
    # --both: the reverse complement follows, except after ACGT, which is its own
    assert repkmers.list_lines(index, count, 4, both=True) == ["AACG\t5\n", "CGTT\t5\n", "ACGT\t70001\n", "CGTA\t2\n", "TACG\t2\n"]
    assert "".join(repkmers.list_lines(index, count, 4, both=True)) == rm.text(index, count, 4, both=True)
    st = {"kmers": 99986, "distinct": 95225, "listed": 8, "listed_occurrences": 153, "threshold": 4, "max_count": 109,
          "count_ms": 0.25, "select_ms": 1.5, "emit_ms": 0.125}
    head, row = repkmers.stats_row(15, st).splitlines()
    assert head.split("\t") == list(repkmers.STATS_HEADER)
    assert row.split("\t") == ["15", "99986", "95225", "4", "8", "153", "109", "0.250", "1.500", "0.125"]
