"""The aligner without a GPU (include/np2_io.h: np2_map_align_*): the host aligner np2_map_align_host (which runs the rule's one
text, csrc/np2_align_core.hpp) against the Python model of tests/align_model.py field for field on the edge cases of
tests/align_cases.py; the same text as a stand-alone program with and without the host sanitizers; checks that do not go through
the model (lengths, spans, NM and AS recomputed, no gap movable, the SAM text through tests/sam_model.py, planted truths as
literal CIGARs); the banded scores against a plain full-matrix affine DP; the refusals, the ABI list and the command line's
device-free helpers.

The stand-alone program's `finish` mode runs the rule's last pass on hand-made alignments as well: the stops of left-alignment
one by one, beside the cases that reach them through the mapper's chains."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_cases as ac
import align_model as am
import map_model as mm
import sam_model as sm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from nextpolish2_amd import map as np2map

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_UNSUPPORTED = -1, -4
K = 19


def host(name):
    contigs, reads, _, _, env = ac.case(name)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        got = np2io.map_align_host(contigs, reads, **ac.call_kw(name))
        return got, np2io.align_last_stats()


def cigars_of(got):
    _, recs, words, off = got
    return [[(am.OPS[int(w) & 15], int(w) >> 4) for w in words[int(a):int(b)]] for a, b in zip(off[:-1], off[1:])]


# ---- 1. the model reaches the edges the cases are built for -------------------------------------------------------------------
def test_model_cases_reach_the_edges_they_are_built_for():
    cnt = lambda name: ac.expected(name)[3]
    cig = lambda name: [ac.cigar_str(c) for c in ac.expected(name)[2]]
    assert cnt("all_equal")["cores"] == cnt("all_equal")["pure_gap"] == cnt("all_equal")["snv"] == 0 and cnt("all_equal")["equal"] == 71
    assert cig("pure_gaps_snv") == ["300M3I300M", "298M4D298M", "600M", "300M3I300M", "298M4D298M"]
    assert (cnt("pure_gaps_snv")["pure_gap"], cnt("pure_gaps_snv")["snv"], cnt("pure_gaps_snv")["cores"]) == (4, 1, 0)
    # band widths: what the cells hold beyond the end extensions' (n + 1) (2 band + 1) is (ql + 1) * W of the cores
    def core_cells(name):
        contigs, reads, _, ao, _ = ac.case(name)
        hits, chains, _ = mm.map_reads(mm.Index(contigs), reads)
        ends = 0
        for rd, ch in zip(reads, chains):
            pins = am.pins_of(ch, K)
            ends += (pins[0][1] - K + 1 + 1 + len(rd) - 1 - pins[-1][1] + 1) * (2 * ao["band"] + 1)
        return cnt(name)["cells"] - ends
    assert core_cells("band_63") == 7 * 63 and core_cells("band_64") == 7 * 64
    assert core_cells("band_65") == 7 * 65 + 7 * 66 and core_cells("band_129") == 7 * 129 + 7 * 130
    # the path on the band's outermost diagonal is found; with one diagonal less the banded optimum is another alignment
    assert cig("band_touch") == cig("band_wide") == ["298M2I12M2D288M"] and cig("band_short") == ["600M"]
    assert ac.expected("band_short")[1][0]["as"] < ac.expected("band_touch")[1][0]["as"]
    assert cnt("core_rows_1_2")["cores"] == 3 and cig("core_rows_1_2") == ["300M2D298M", "300M1D299M", "300M2D298M"]
    # anchors less than k apart on two diagonals: the later one is no pin
    contigs, reads, *_ = ac.case("tandem")
    hits, chains, _ = mm.map_reads(mm.Index(contigs), reads)
    n_skipped = 0
    for ch in chains:
        skipped = [(a, b) for a, b in zip(ch[:-1].tolist(), ch[1:].tolist()) if b[0] - a[0] < K and b[0] - a[0] != b[1] - a[1]]
        assert all(tuple(b) not in am.pins_of(ch, K) for _, b in skipped)
        n_skipped += len(skipped)
    assert n_skipped >= 2
    assert all(h["n"] == 1 for h in ac.expected("one_pin")[0] if h) and cnt("one_pin")["pins"] == 6 and cnt("one_pin")["segments"] == 0
    assert cig("end_bonus_equal") == ["600M", "600M"] and cig("end_bonus_less") == ["597M3S", "3S597M"][:1] * 2
    assert cig("ext_max")[0] == "9S585M6S"  # a head of 12 and a tail of 9 matching bases, three considered
    assert all(r["pos"] == 0 for r in ac.expected("head_no_reference")[1]) and cig("head_no_reference") == ["40S500M", "40S500M", "300M"]
    assert cig("overhang") == ["300S400M", "500M300S", "300S400M", "500M300S"]
    # left-alignment through a pin: the gap ends up inside the columns of a pin of the chain
    contigs, reads, *_ = ac.case("homopolymer")
    hits, chains, _ = mm.map_reads(mm.Index(contigs), reads)
    assert cig("homopolymer") == ["300M1D299M", "300M1I300M"] * 2
    assert any(r - K + 1 < 800 <= r for ch in chains for r, q in am.pins_of(ch, K))
    # two gaps that meet and merge, and a gap that runs to the alignment's first column: what left-alignment was given and left
    for name, first in (("gaps_merge", False), ("first_column", True)):
        contigs, reads, o, ao, _ = ac.case(name)
        seen, plain = [], am.left_align

        def spy(runs, *a):
            before = [tuple(x) for x in runs]
            plain(runs, *a)
            seen.append((before, [tuple(x) for x in runs]))
        am.left_align = spy
        try:
            am.align_reads(contigs, reads, map_kw=o, **ao)
        finally:
            am.left_align = plain
        assert len(seen) == len(reads)
        for before, after in seen:
            gaps = lambda runs: [x for x in runs if x[0] in "ID"]
            if first:
                assert before[0][0] == "M" and before[0][1] > 1 and after[0] == ("M", 1) and after[1][0] == "I"
            else:
                assert [L for _, L in gaps(before)] == [7, 7] and [L for _, L in gaps(after)] == [14]
                assert sum(op == "M" for op, _ in before) >= 3  # (pins between the two)
    assert cig("gaps_merge") == ["300M14D496M", "300M14I510M"] * 2 and cig("first_column")[:2] == ["1M7I334M", "1M14I334M"]
    assert cnt("n_bases")["snv"] == 1 and [r["nm"] for r in ac.expected("n_bases")[1]] == [1, 2, 2]
    assert [r["nm"] for r in ac.expected("lower_case")[1]] == [2, 0, 2]
    assert [r["tid"] for r in ac.expected("cells_overflow")[1]] == [0, -1, 0] and cnt("cells_overflow")["overflow"] == 1
    assert [r["tid"] for r in ac.expected("unmapped_between")[1]] == [0, -1, 0] and cnt("unmapped_between")["overflow"] == 0


# ---- 2. np2_map_align_host against the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_host_aligner_equals_the_model(name):
    got, st = host(name)
    ac.check(got, name)
    cnt, tot = ac.expected(name)[3], ac.expected(name)[4]
    assert {f: st[f] for f in cnt} == cnt
    mst = np2io.map_last_stats()
    assert {f: mst[f] for f in tot} == tot


# ---- 3. checks that do not go through the model ---------------------------------------------------------------------------------
def columns(contig, read, rec, cigar):
    """-> (reference codes, read codes on the record's strand)"""
    T, Q = am.codes(contig), am.codes(read)
    return T, am.rc_codes(Q) if rec["flag"] & 16 else Q


def movable(T, Q, rec, cigar):
    """a gap that could move one column left under the rule's condition"""
    r, q = int(rec["pos"]), 0
    for i, (op, L) in enumerate(cigar):
        if op in "ID" and i > 0 and cigar[i - 1][0] == "M":
            only_one_left = (i - 1 == (1 if cigar[0][0] == "S" else 0)) and cigar[i - 1][1] == 1
            last = T[r + L - 1] if op == "D" else Q[q + L - 1]
            if not only_one_left and am.same(T[r - 1], Q[q - 1]) and last == T[r - 1]:
                return (i, op, L)
        r += L if op in "MD" else 0
        q += L if op in "MIS" else 0
    return None


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_records_hold_without_the_model(name, core_program, tmp_path):
    contigs, reads, mo, ao, _ = ac.case(name)
    o = am.opts(**ao)
    got, _ = host(name)
    hits, recs, words, off = got
    tnames = [str(i + 1) for i in range(len(contigs))]
    # the SAM text as the library's writer (sam_header, sam_line of np2_align_cpu.hpp) formats it, through the stand-alone program
    (tmp_path / "asm").write_bytes(b"".join(c + b"\n" for c in contigs))
    (tmp_path / "reads").write_bytes(b"".join(c + b"\n" for c in reads))
    mo = mm.opts(**mo)
    r = subprocess.run([core_program, str(tmp_path / "asm"), str(tmp_path / "reads")] + [str(mo[f]) for f in mm.DEFAULTS] +
                       [str(o[f]) for f in am.DEFAULTS] + ["sam"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-3000:]
    text = r.stdout
    lines = sm.split_lines(text)
    refs, n_head = sm.parse_header(lines)
    assert refs == list(zip(tnames, [len(c) for c in contigs])) and n_head == len(contigs) + 2
    tid_of = {n.encode(): i for i, n in enumerate(tnames)}
    for rd, rec, cg, line in zip(reads, recs, cigars_of(got), lines[n_head:]):
        p = sm.parse_line(line, tid_of)
        if rec["tid"] < 0:
            assert rec["flag"] == 4 and not cg and p["tid"] == -1 and p["flag"] == 4 and p["cigar"] == [] and p["seq"] == rd.decode()
            continue
        T, Q = columns(contigs[rec["tid"]], rd, rec, cg)
        assert sum(L for op, L in cg if op in "MIS") == len(rd)
        assert 0 <= rec["pos"] < rec["end"] <= len(T) and rec["end"] - rec["pos"] == sum(L for op, L in cg if op in "MD")
        assert all(op in "MIDS" for op, _ in cg) and all(a[0] != b[0] for a, b in zip(cg[:-1], cg[1:]))
        assert all(op != "S" or i in (0, len(cg) - 1) for i, (op, _) in enumerate(cg))
        nm = score = 0
        r, q = int(rec["pos"]), 0
        for op, L in cg:
            if op == "M":
                mis = sum(not am.same(T[r + c], Q[q + c]) for c in range(L))
                nm, score = nm + mis, score + (L - mis) * o["match"] - mis * o["mismatch"]
            elif op in "ID":
                nm, score = nm + L, score - o["gap_open"] - L * o["gap_ext"]
            r += L if op in "MD" else 0
            q += L if op in "MIS" else 0
        assert (nm, score) == (rec["nm"], rec["as"])
        assert movable(T, Q, rec, cg) is None
        seq = mm.revcomp(rd) if rec["flag"] & 16 else rd
        assert (p["tid"], p["pos"], p["flag"], p["mapq"], p["cigar"], p["seq"]) == (rec["tid"], rec["pos"], rec["flag"], rec["mapq"], cg, seq.decode())


def full_affine(T, Q, o):
    """the score of the best global alignment: three full tables, no band"""
    NEG = -10 ** 9
    go, ge = o["gap_open"], o["gap_ext"]
    H = [[NEG] * (len(T) + 1) for _ in range(len(Q) + 1)]
    E = [[NEG] * (len(T) + 1) for _ in range(len(Q) + 1)]
    F = [[NEG] * (len(T) + 1) for _ in range(len(Q) + 1)]
    H[0][0] = 0
    for i in range(len(Q) + 1):
        for j in range(len(T) + 1):
            if i == j == 0:
                continue
            if j:
                E[i][j] = max(E[i][j - 1], H[i][j - 1] - go) - ge
            if i:
                F[i][j] = max(F[i - 1][j], H[i - 1][j] - go) - ge
            d = H[i - 1][j - 1] + (o["match"] if am.same(T[j - 1], Q[i - 1]) else -o["mismatch"]) if i and j else NEG
            H[i][j] = max(d, E[i][j], F[i][j])
    return H[len(Q)][len(T)]


def segments_of_cases(names):
    """the bases between consecutive pins of the cases' reads that are not equal: (reference, read) as bytes of ACGTN"""
    out = []
    for name in names:
        contigs, reads, o, ao, _ = ac.case(name)
        assert "band" not in ao or ao["band"] == 32
        hits, chains, _ = mm.map_reads(mm.Index(contigs), reads, **o)
        for rd, h, ch in zip(reads, hits, chains):
            if h is None:
                continue
            T, Q = contigs[h["tid"]].upper(), (mm.revcomp(rd) if h["rev"] else rd).upper()
            pins = am.pins_of(ch, K)
            for (pr, pq), (r, q) in zip(pins[:-1], pins[1:]):
                st, sq = T[pr + 1:r - K + 1], Q[pq + 1:q - K + 1]
                if st != sq:
                    out.append((st, sq))
    return out


@pytest.fixture(scope="module")
def core_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align_core") / "align_core_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-o", exe, os.path.join(HERE, "tools", "align_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_banded_scores_equal_a_full_matrix(core_program, tmp_path):
    """The C++ recurrence (classify and dp_slot of the core text, through the stand-alone program's `core` mode, which is what
    the host library runs) against a plain full-matrix affine DP written here, not against the model: every core of the cases
    whose shorter side is <= band, where the band holds the whole matrix, and seeded random pairs of length 1 .. 40 under a band of
    40; under the default scores and under the extremes of tests/alignchain_cases.py.

    The kernels share classify, gap_of, h_of, choose_end and the walk with this text, but not the matrix loop: k_align_dp has its
    own (a prefix maximum over the lanes for E, carries between the blocks of 64 lanes, the previous row in LDS).  It is held
    to dp_slot cell by cell in tests/test_gpu_map_alignchain.py."""
    import alignchain_cases as cc
    rng = np.random.default_rng(5)
    letters = b"ACGTN"
    pairs = [tuple(bytes(letters[i] for i in rng.integers(0, 4 if rng.random() < 0.9 else 5, int(rng.integers(1, 41)))) for _ in range(2))
             for _ in range(400)]
    segs = segments_of_cases(("band_65", "core_rows_1_2", "lower_case", "unmapped_between", "pure_gaps_snv", "n_bases", "cells_overflow"))
    n_cores = {}
    runs = [("random", pairs, 40, None), ("cases", segs, 32, None)]
    runs += [(sc, pairs, 40, cc.scoring(sc)) for sc in cc.OPTSETS] + [(sc + "/cases", segs, 32, cc.scoring(sc)) for sc in cc.OPTSETS]
    for label, todo, band, scores in runs:
        o = am.opts(**(scores or {}))
        (tmp_path / "pairs").write_bytes(b"".join(t + b" " + q + b"\n" for t, q in todo))
        r = subprocess.run([core_program, "core", str(tmp_path / "pairs"), str(band)] + [str(v) for v in (scores or {}).values()],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(todo)
        n_cores[label] = 0
        for (t, q), line in zip(todo, lines):
            kind, over, pre, suf, tl, ql, score = (int(x) for x in line.split())
            T, Q = am.codes(t), am.codes(q)
            assert not over and (tl, ql) == (len(T) - pre - suf, len(Q) - pre - suf)
            assert all(am.same(a, b) for a, b in zip(T[:pre], Q[:pre])) and all(am.same(T[len(T) - 1 - i], Q[len(Q) - 1 - i]) for i in range(suf))
            if kind != 3:  # no matrix: equal, one gap, or one mismatch
                assert (kind == 0 and tl == ql and suf == 0 and pre == len(T)) or (kind == 1 and min(tl, ql) == 0 < max(tl, ql)) or \
                       (kind == 2 and tl == ql == 1)
                continue
            if min(tl, ql) > band:
                continue
            n_cores[label] += 1
            assert score == full_affine(T[pre:len(T) - suf], Q[pre:len(Q) - suf], o), (t, q)
    assert n_cores["random"] > 350 and n_cores["cases"] >= 8
    assert all(n_cores[sc] == n_cores["random"] and n_cores[sc + "/cases"] == n_cores["cases"] for sc in cc.OPTSETS)


def test_planted_truths_as_literal_cigars():
    contig = bytes(ac.rand(3000, 21))
    c = bytearray(contig)
    c[1300:1308] = b"TTTTTTTT"
    c[1299], c[1308] = ord("A"), ord("C")
    contig = bytes(c)
    base = contig[1000:1600]
    subst = bytearray(base)
    subst[250] = ac.other(subst[250])
    hdel = base[:304] + base[305:]  # a base out of the homopolymer's middle
    hins = base[:304] + b"T" + base[304:]
    big = base[:200] + base[250:]
    left, right = bytes(ac.rand(300, 22)) + contig[:300], contig[-300:] + bytes(ac.rand(300, 23))
    reads = [bytes(subst), hdel, hins, big, left, right]
    reads += [mm.revcomp(r) for r in reads]
    want = ["600M", "300M1D299M", "300M1I300M", "200M50D350M", "300S300M", "300M300S"]
    hits, recs, words, off = np2io.map_align_host([contig], reads)
    assert ac.cigar_text(words, off) == want * 2
    assert [int(r["pos"]) for r in recs] == [1000, 1000, 1000, 1000, 0, 2700] * 2
    assert [int(r["nm"]) for r in recs] == [1, 1, 1, 50, 0, 0] * 2 and [int(r["flag"]) for r in recs] == [0] * 6 + [16] * 6
    assert [int(r["as"]) for r in recs] == [595, 591, 592, 444, 300, 300] * 2


# ---- 4. the rule's text as a stand-alone program --------------------------------------------------------------------------------
def core_output(name):
    hits, recs, cigars, cnt, _ = ac.expected(name)
    lines = [" ".join(str(cnt[f]) for f in am.COUNT_FIELDS)]
    for rec, cg in zip(recs, cigars):
        lines.append(" ".join(str(rec[f]) for f in am.REC_FIELDS) + " " + (ac.cigar_str(cg) or "*"))
    return "\n".join(lines) + "\n"


def finish_model(T, Q, t_start, raw):
    """the model's last pass on a hand-made alignment: ends, left-alignment, NM, AS -> the program's line"""
    runs = [[op, int(n)] for n, op in sm._CIGAR_OP.findall(raw.encode())]
    runs = [[op.decode(), n] for op, n in runs]
    Tc, Qc = am.codes(T.encode()), am.codes(Q.encode())
    clip5 = runs.pop(0)[1] if runs[0][0] == "S" else 0
    clip3 = runs.pop()[1] if runs[-1][0] == "S" else 0
    am.left_align(runs, Tc, Qc, t_start, clip5)
    o = am.opts()
    nm = score = 0
    r, q = t_start, clip5
    for op, L in runs:
        if op == "M":
            mis = sum(not am.same(Tc[r + c], Qc[q + c]) for c in range(L))
            nm, score = nm + mis, score + (L - mis) * o["match"] - mis * o["mismatch"]
            r, q = r + L, q + L
        else:
            nm, score = nm + L, score - o["gap_open"] - L * o["gap_ext"]
            r, q = r + (L if op == "D" else 0), q + (L if op == "I" else 0)
    cg = ([("S", clip5)] if clip5 else []) + [tuple(x) for x in runs] + ([("S", clip3)] if clip3 else [])
    return f"{t_start} {r} {nm} {score} {ac.cigar_str(cg)}\n"


FINISH = [
    # (reference, read, t_start, raw ops, what the rule gives) -- a deletion in a run that reaches the alignment's first column
    ("AAAAAAAAGCTTGCA", "AAAAAAGCTTGCA", 0, "6M2D7M", "0 15 2 3 1M2D12M\n"),
    ("CAAAAAAAAGCTTGCA", "AAAAAAGCTTGCA", 1, "6M2D7M", "1 16 2 3 1M2D12M\n"),
    ("GGAAAAAAGCTTGCA", "TTTGGAAAAAAAAGCTTGCA", 0, "3S8M2I7M", "0 15 2 5 3S2M2I13M\n"),
    # two deletions in one run, an M run between them: they meet and the merged gap moves on
    ("GCAAAAAAAAAATCG", "GCAAAAAATCG", 0, "4M2D2M2D5M", "0 15 4 -3 2M4D9M\n"),
    # two gaps of different kinds stop at each other
    ("GCAAAAAATCGGA", "GCAAAAAAATCGGA", 0, "5M2I3M1D4M", None),
    # a mismatch column and an N stop a gap
    ("GCATAAAATCG", "GCATAAATCG", 0, "7M1D3M", "0 11 1 2 4M1D6M\n"),
    ("GCANAAAATCG", "GCANAAATCG", 0, "7M1D3M", "0 11 2 -3 4M1D6M\n"),
]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_core_program_matches_the_model(tmp_path, flags):
    exe = str(tmp_path / "align_core_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "tools", "align_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in sorted(ac.CASES):
        contigs, reads, o, ao, _ = ac.case(name)
        o, ao = mm.opts(**o), am.opts(**ao)
        (tmp_path / "asm").write_bytes(b"".join(c + b"\n" for c in contigs))
        (tmp_path / "reads").write_bytes(b"".join(c + b"\n" for c in reads))
        r = subprocess.run([exe, str(tmp_path / "asm"), str(tmp_path / "reads")] + [str(o[f]) for f in mm.DEFAULTS] + [str(ao[f]) for f in am.DEFAULTS],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-3000:])
        assert r.stdout == core_output(name), name
    for T, Q, t_start, raw, want in FINISH:
        r = subprocess.run([exe, "finish", T, Q, str(t_start), raw], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (raw, r.stderr[-3000:])
        assert r.stdout == finish_model(T, Q, t_start, raw), raw
        if want is not None:
            assert r.stdout == want, raw
    argv = [exe, str(tmp_path / "asm"), str(tmp_path / "reads")] + [str(mm.DEFAULTS[f]) for f in mm.DEFAULTS] + ["1", "4", "6", "0", "32", "5", "2048", "100"]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stderr.startswith("argument: gap_ext")


# ---- 5. refusals, before any device call -----------------------------------------------------------------------------------------
def test_refusals_come_back_as_statuses_with_their_messages():
    asm, reads = b"ACGT" * 30 + b"\n", b"ACGT" * 20 + b"\n"
    for kw, word in ((dict(match=0), "match"), (dict(match=16), "match"), (dict(mismatch=32), "mismatch"), (dict(gap_open=256), "gap_open"),
                     (dict(gap_ext=0), "gap_ext"), (dict(gap_ext=16), "gap_ext"), (dict(band=1024), "band"), (dict(end_bonus=(1 << 16) + 1), "end_bonus"),
                     (dict(ext_max=0), "ext_max"), (dict(max_cells=0), "max_cells"), (dict(max_cells=(1 << 24) + 1), "max_cells")):
        with pytest.raises(api.Np2Error) as e:
            np2io.map_align_host(asm, reads, **kw)
        assert e.value.code == E_ARG and word in str(e.value), kw
    with pytest.raises(api.Np2Error) as e:
        np2io.map_align_host(asm, reads, k=29)
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(TypeError):
        np2io.align_opts(bandd=3)
    L = np2io._bind()
    o, ao = np2io.map_opts(), np2io.align_opts()
    a, r = np.frombuffer(asm, np.uint8), np.frombuffer(reads, np.uint8)
    recs = np.zeros(1, np2io.ALIGN_REC_DTYPE)
    pc, off = C.c_void_p(), np.zeros(2, np.uint64)
    call = lambda *x: L.np2_map_align_host(a.ctypes.data, len(a), r.ctypes.data, len(r), *x)
    assert call(1, C.byref(o), None, None, recs.ctypes.data, None, None) == E_ARG and b"align_opts" in L.np2_io_last_error()
    assert call(1, None, C.byref(ao), None, recs.ctypes.data, None, None) == E_ARG and b"opts" in L.np2_io_last_error()
    assert call(1, C.byref(o), C.byref(ao), None, None, None, None) == E_ARG and b"recs" in L.np2_io_last_error()
    assert call(2, C.byref(o), C.byref(ao), None, recs.ctypes.data, None, None) == E_ARG and b"n_reads" in L.np2_io_last_error()
    assert call(1, C.byref(o), C.byref(ao), None, recs.ctypes.data, C.byref(pc), None) == E_ARG and b"cigar" in L.np2_io_last_error()
    assert call(1, C.byref(o), C.byref(ao), None, recs.ctypes.data, None, off.ctypes.data) == E_ARG and b"cigar" in L.np2_io_last_error()
    assert L.np2_map_align_bytes(None, r.ctypes.data, len(r), 1, C.byref(o), C.byref(ao), None, recs.ctypes.data, None, None) == E_ARG
    assert b"index" in L.np2_io_last_error()
    assert L.np2_map_align_files(None, None, 0, C.byref(o), C.byref(ao), b"x", None) == E_ARG
    assert L.np2_map_align_last_stats(None) == E_ARG
    assert call(1, C.byref(o), C.byref(ao), None, recs.ctypes.data, None, None) == 0  # the thread's next call works; hits may be NULL
    assert int(recs[0]["flag"]) in (0, 4)


def test_abi_symbols_are_listed():
    L = api.lib()
    for s in ("np2_map_align_bytes", "np2_map_align_files", "np2_map_align_host", "np2_map_align_last_stats"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)


def test_command_line_helpers():
    a = np2map.build_parser().parse_args(["asm.fa", "r1.fa", "-a", "-o", "x.sam.gz", "-B", "5", "--band", "16", "--max_cells", "1000"])
    assert (a.sam, a.out, a.match, a.mismatch, a.gap_open, a.gap_ext, a.band, a.end_bonus, a.ext_max, a.max_cells) == \
        (True, "x.sam.gz", 1, 5, 6, 2, 16, 5, 2048, 1000)
    a = np2map.build_parser().parse_args(["asm.fa", "r1.fa"])
    assert a.sam is False and a.out is None
    st = dict(pins=5, segments=4, equal=2, pure_gap=1, snv=0, cores=1, cells=455, clipped_bases=3, overflow=0, pins_ms=0.5, classify_ms=0.25,
              dp_ms=1.0, assemble_ms=2.0, write_ms=0.125)
    head, row = np2map.align_stats_row(st).splitlines()
    assert head.split("\t") == list(np2map.ALIGN_STATS_HEADER) and len(np2map.STATS_HEADER) == 16
    assert row.split("\t") == ["5", "4", "2", "1", "0", "1", "455", "3", "0", "0.500", "0.250", "1.000", "2.000", "0.125"]
    hit = dict(n=5, s1=70, s2=0)
    rec = dict(tid=0, flag=16, pos=9, mapq=60, nm=1, **{"as": 7})
    assert am.sam_line("r/1", b"ACGTn", hit, rec, [("S", 1), ("M", 4)], ["ctg"]) == \
        "r/1\t16\tctg\t10\t60\t1S4M\t*\t0\t0\tnACGT\t*\tNM:i:1\tAS:i:7\tcm:i:5\ts1:i:70\ts2:i:0\n"
    assert am.sam_line("r/2", b"ACG", None, am.UNALIGNED, [], ["ctg"]) == "r/2\t4\t*\t0\t0\t*\t*\t0\t0\tACG\t*\n"
