"""The aligner's opt-in outputs without a GPU (include/np2_io.h: np2_map_align_*, "Tags"): the host twin np2_align_tags_host (the
rule's one text, csrc/np2_aligntags_core.hpp, walked by one caller) against the Python model of tests/aligntags_model.py on the
hand-built and the seeded random records; np2_map_align_host_x on every aligner edge case (tests/align_cases.py): untouched
records without a flag, = / X that collapse back to M, MD and cs equal to the model on the model's CIGAR, the reference rebuilt
from SEQ + CIGAR + MD, NM = X + I + D; the same text as a stand-alone program under the host sanitizers; the refusals of the doors
and of the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases as ac
import align_model as am
import aligntags_model as tm
import map_model as mm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from nextpolish2_amd import map as np2map

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV = dict(os.environ, PYTHONPATH=ROOT)
FLAG_SETS = [dict(md=True, cs=True, eqx=True), dict(md=True, cs=False, eqx=False), dict(md=False, cs=True, eqx=False),
             dict(md=False, cs=False, eqx=True)]


def check_tags(got, records, flags):
    md, cs, eqx = got
    want_md, want_cs, want_eqx = tm.expected(records)
    assert (md is None) == (not flags["md"]) and (cs is None) == (not flags["cs"]) and (eqx is None) == (not flags["eqx"])
    if flags["md"]:
        assert md == want_md
    if flags["cs"]:
        assert cs == want_cs
    if flags["eqx"]:
        assert len(eqx) == len(want_eqx)
        for g, w, rec in zip(eqx, want_eqx, records):
            assert np.array_equal(g, w), (tm.cigar_of(g), tm.cigar_of(w), rec[2])


# ---- 1. the model on literal answers ----------------------------------------------------------------------------------------------
def test_model_on_literal_answers():
    assert tm.tags(b"ACGTACGT", b"ACGTACGT", [("M", 8)]) == (b"8", b":8", [("=", 8)])
    assert tm.tags(b"ACGTAC", b"ACGGT", [("M", 3), ("D", 2), ("M", 1), ("S", 1)])[:2] == (b"3^TA0C0", b":3-ta*cg")
    h = tm.hand_cases()
    t, q, c = h["d_then_sub"]
    assert tm.tags(t, q, c)[0] == b"10^AC0T9"
    t, q, c = h["subs_130"]
    md, cs, split = tm.tags(t, q, c)
    assert md == b"".join(b"0" + bytes([b]) for b in t) + b"0" and split == [("X", 130)] and len(cs) == 3 * 130
    t, q, c = h["i_between"]
    assert tm.tags(t, q, c) == (b"90", b":40+" + q[40:43].lower() + b":50", [("=", 40), ("I", 3), ("=", 50)])
    t, q, c = h["count_9999"]
    assert tm.tags(t, q, c)[0] == b"0" + t[:1] + b"9999" + t[-1:] + b"0"
    t, q, c = h["n_against_n"]
    assert tm.tags(t, q, c)[1] == b":5*nn:60*" + t[66:67].lower() + b"n:3"
    t, q, c = h["odd_reference_bytes"]
    assert tm.tags(t, q, c)[0] == b"2R61N0N4^RNNN10"
    assert tm.tags(b"acgT", b"ACGt", [("M", 4)]) == (b"4", b":4", [("=", 4)])
    assert tm.tags(b"", b"", []) == (b"", b"", [])
    # the inverse: SEQ + CIGAR + MD give the aligned reference back
    for name, (t, q, c) in h.items():
        if c:
            md, _, split = tm.tags(t, q, c)
            n_t = sum(n for op, n in c if op in "MD")
            assert tm.rebuild_reference(q, split, md) == bytes(tm.L(b) for b in t[:n_t]) == tm.rebuild_reference(q, c, md), name
            assert tm.collapse(split) == tm.collapse(c)


# ---- 2. the host twin against the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAG_SETS, ids=["all", "md", "cs", "eqx"])
def test_host_twin_equals_the_model_on_hand_cases(flags):
    h = tm.hand_cases()
    records = [h[name] for name in h]
    ref, reads, t_off, q_off, cigars = tm.pack(records)
    check_tags(np2io.align_tags_host(ref, reads, t_off, q_off, cigars, **flags), records, flags)
    for name in h:  # and each alone, at offset 0 with nothing behind it
        ref, reads, t_off, q_off, cigars = tm.pack([h[name]], pad=0)
        check_tags(np2io.align_tags_host(ref, reads, t_off, q_off, cigars, **flags), [h[name]], flags)


def test_host_twin_equals_the_model_on_random_records():
    records = tm.random_records()
    assert len(records) == 200 and max(n for _, _, c in records for _, n in c) == 300
    ref, reads, t_off, q_off, cigars = tm.pack(records)
    flags = FLAG_SETS[0]
    check_tags(np2io.align_tags_host(ref, reads, t_off, q_off, cigars, **flags), records, flags)
    assert np2io.align_tags_host(b"", b"", [], [], [], **flags) == ([], [], [])


# ---- 3. np2_map_align_host_x on the aligner's edge cases ---------------------------------------------------------------------------
def cigars_of(words, off):
    return [tm.cigar_of(words[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]


def aligned(read, rev):
    return mm.revcomp(read) if rev else bytes(read)


def check_case_outputs(name, plain, full):
    """plain: (hits, recs, cigar, off) without a flag; full: the six of a call with md, cs and eqx"""
    contigs, reads, _, _, _ = ac.case(name)
    ph, pr, pc, po = plain
    fh, fr, fc, fo, md, cs = full
    assert np.array_equal(ph, fh)
    for f in am.REC_FIELDS:
        if f != "n_cigar":
            assert np.array_equal(pr[f], fr[f]), f
    base, split = cigars_of(pc, po), cigars_of(fc, fo)
    assert [tm.collapse(c) for c in split] == base and all(op in "=XIDS" for c in split for op, _ in c)
    assert [len(c) for c in split] == [int(v) for v in fr["n_cigar"]]
    for i, (rec, cg) in enumerate(zip(pr, base)):
        if int(rec["tid"]) < 0:
            assert md[i] == b"" and cs[i] == b"" and not split[i]
            continue
        t = contigs[int(rec["tid"])][int(rec["pos"]):]
        q = aligned(reads[i], int(rec["flag"]) & 16)
        want = tm.tags(t, q, cg)
        assert (md[i], cs[i], split[i]) == want, (name, i)
        assert tm.rebuild_reference(q, split[i], md[i]) == bytes(tm.L(b) for b in contigs[int(rec["tid"])][int(rec["pos"]):int(rec["end"])])
        assert int(rec["nm"]) == tm.nm_of(split[i])


def host_x(name, **flags):
    contigs, reads, _, _, env = ac.case(name)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return np2io.map_align_host_x(contigs, reads, **flags, **ac.call_kw(name))


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_host_x_on_the_aligner_cases(name):
    contigs, reads, _, _, env = ac.case(name)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        plain = np2io.map_align_host(contigs, reads, **ac.call_kw(name))
    none = host_x(name)
    assert none[4] is None and none[5] is None and all(np.array_equal(a, b) for a, b in zip(plain, none[:4]))
    full = host_x(name, md=True, cs=True, eqx=True)
    check_case_outputs(name, plain, full)
    st = np2io.align_last_tag_stats()
    assert st["tags_ms"] == 0 and st["md_bytes"] == sum(map(len, full[4])) and st["cs_bytes"] == sum(map(len, full[5]))
    only_md = host_x(name, md=True)
    assert only_md[4] == full[4] and only_md[5] is None and np.array_equal(only_md[2], plain[2])


# ---- 4. the stand-alone program under the host sanitizers --------------------------------------------------------------------------
@pytest.mark.parametrize("cxx_flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_core_program_matches_the_model(tmp_path, cxx_flags):
    exe = str(tmp_path / "aligntags_core_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + cxx_flags + ["-o", exe, os.path.join(HERE, "tools", "aligntags_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    h = tm.hand_cases()
    records = [h[name] for name in h] + tm.random_records(20, seed=3)
    with open(tmp_path / "records", "wb") as f:  # per record three lines: t, q (hex, so that any byte goes through), the CIGAR text
        for t, q, c in records:
            f.write(t.hex().encode() + b"\n" + q.hex().encode() + b"\n" + ("".join(f"{n}{op}" for op, n in c) or "*").encode() + b"\n")
    for lanes in ("1", "64", "7"):
        r = subprocess.run([exe, str(tmp_path / "records"), lanes], capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-3000:]
        lines = r.stdout.split(b"\n")
        assert len(lines) == 3 * len(records) + 1
        for i, (t, q, c) in enumerate(records):
            md, cs, split = tm.tags(t, q, c)
            assert lines[3 * i] == md and lines[3 * i + 1] == cs, (lanes, i)
            assert lines[3 * i + 2] == ("".join(f"{n}{op}" for op, n in split) or "*").encode(), (lanes, i)


# ---- 5. refusals, before any walk --------------------------------------------------------------------------------------------------
def test_door_refusals():
    ref, reads = b"ACGTACGT", b"ACGTACGT"
    ok = dict(ref=ref, reads=reads, t_off=[0], q_off=[0], cigars=[tm.words([("M", 8)])])
    assert np2io.align_tags_host(**ok) == ([b"8"], [b":8"], [ok["cigars"][0] | 7])
    for change, text in ((dict(cigars=[tm.words([("M", 9)])]), "beyond the reference buffer"),
                         (dict(cigars=[tm.words([("M", 8), ("I", 1)])]), "beyond the read buffer"),
                         (dict(t_off=[1]), "beyond the reference buffer"), (dict(q_off=[9]), "beyond the read buffer"),
                         (dict(cigars=[tm.words([("M", 4), ("N", 2), ("M", 2)])]), "not M, I, D or S"),
                         (dict(cigars=[tm.words([("=", 8)])]), "not M, I, D or S")):
        with pytest.raises(api.Np2Error) as e:
            np2io.align_tags_host(**dict(ok, **change))
        assert e.value.code == -1 and text in str(e.value), str(e.value)
    L = np2io._bind()
    r8, off = np.frombuffer(ref, np.uint8), np.zeros(2, np.uint64)
    zero, coff, w = np.zeros(1, np.uint64), np.array([0, 1], np.uint64), tm.words([("M", 8)])
    pm, px, pe = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def raw(flags, md=True, md_off=True):
        return L.np2_align_tags_host(r8.ctypes.data, 8, r8.ctypes.data, 8, 1, zero.ctypes.data, zero.ctypes.data, w.ctypes.data, coff.ctypes.data, flags,
                                     C.byref(pm) if md else None, off.ctypes.data if md_off else None, None, None, None, None)
    assert raw(16) == -1 and b"unknown flag bits" in L.np2_io_last_error()
    assert raw(1) == -1 and b"unknown flag bits" in L.np2_io_last_error()  # (NP2_ALN_QUAL is no output of the walk)
    assert raw(2, md_off=False) == -1 and b"md and md_off go together" in L.np2_io_last_error()
    assert raw(2, md=False, md_off=False) == -1 and b"NP2_ALN_MD without" in L.np2_io_last_error()
    assert raw(4) == -1 and b"NP2_ALN_CS without" in L.np2_io_last_error()
    assert raw(2) == 0 and C.string_at(pm.value, int(off[1])) == b"8"
    L.np2_free(pm)
    with pytest.raises(api.Np2Error) as e:  # the device door checks the same before its first device call
        np2io.align_tags_device(**dict(ok, cigars=[tm.words([("M", 9)])]))
    assert "beyond the reference buffer" in str(e.value)
    asm, rd = b"ACGT" * 30 + b"\n", b"ACGT" * 20 + b"\n"
    a, r = np.frombuffer(asm, np.uint8), np.frombuffer(rd, np.uint8)
    recs, o, ao = np.zeros(1, np2io.ALIGN_REC_DTYPE), np2io.map_opts(), np2io.align_opts()
    rc = L.np2_map_align_host_x(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, C.byref(o), C.byref(ao), None, 32, None, recs.ctypes.data, None, None,
                                None, None, None, None)
    assert rc == -1 and b"unknown flag bits" in L.np2_io_last_error()


def test_abi_symbols_are_listed():
    for s in ("np2_map_align_bytes_x", "np2_map_align_files_x", "np2_map_align_host_x", "np2_align_tags_device", "np2_align_tags_host",
              "np2_map_align_last_tag_stats"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(np2io._bind(), s)


def run_map(*args):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd.map"] + [str(a) for a in args], capture_output=True, text=True, env=ENV, timeout=600)


@pytest.mark.parametrize("flag", ["--qual", "--MD", "--cs", "--eqx"])
def test_command_line_refuses_a_tag_flag_without_a(flag, tmp_path):
    (tmp_path / "a.fa").write_text(">c\nACGT\n")
    r = run_map(tmp_path / "a.fa", tmp_path / "a.fa", flag)
    assert r.returncode == 2 and f"{flag} needs -a" in r.stderr


def test_command_line_helpers():
    row = np2map.tag_stats_row(dict(md_bytes=5, cs_bytes=7, eqx_words=3, qual_reads=2, tags_ms=0.25))
    assert row == "md_bytes\tcs_bytes\teqx_words\tqual_reads\ttags_ms\n5\t7\t3\t2\t0.250\n"
    a = np2map.build_parser().parse_args(["asm.fa", "r.fq", "-a", "--qual", "--MD", "--cs", "--eqx"])
    assert (a.qual, a.md, a.cs, a.eqx) == (True, True, True, True)
    a = np2map.build_parser().parse_args(["asm.fa", "r.fq", "-a"])
    assert (a.qual, a.md, a.cs, a.eqx) == (False, False, False, False)
