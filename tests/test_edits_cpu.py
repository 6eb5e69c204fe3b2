"""The edit report without a device: the plain model of tests/edits_model.py on hand-derived cases and on the reference's
test bundle polished by the CPU oracle (the known answer), the one-lane host program of the kernels' rule
(csrc/np2_edits_core.hpp through tests/tools/edits_core_test.cpp, built with the host sanitizers) against the model, the VCF
writer's anchoring, and the command line's argument checks."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import edits_cases as Cs
import edits_model as M
from nextpolish2_amd import Opts, edits
from nextpolish2_amd import io as np2io

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUNDLE = os.path.join(HERE, "golden", "ref_bundle")
ASM = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
BAM = os.path.join(BUNDLE, "hifi.map.sort.bam")

# the known answer on the bundle (oracle, default options): (ref_pos, out_off, REF, ALT, kind) after the shift.  Before
# left-alignment the four insertions lie at the same contig positions: the suffix-first trimming already put each at the
# left end of its run, and the base before it differs.
BUNDLE_EDITS = [(63156, 63156, b"", b"T", "INS"), (76368, 76369, b"", b"T", "INS"), (79624, 79626, b"", b"A", "INS"),
                (81108, 81111, b"", b"T", "INS")]
BUNDLE_TOTALS = dict(has_span=1, first=0, last=99999, raw_runs=2128, same_runs=2124, n_kind=[0, 0, 4, 0, 0], bases_inserted=4,
                     bases_deleted=0, outside=0)


# ---- 1. the model on hand-derived cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(Cs.HAND))
def test_model_on_hand_derived_cases(name):
    ref, (bases, pos), recs, totals, vcf = Cs.HAND[name]
    got, tot = M.edits(ref, bases, pos)
    assert got == recs
    assert all(tot[k] == v for k, v in totals.items()), tot
    assert sum(tot["n_kind"]) == len(recs) == tot["raw_runs"] - tot["same_runs"]
    if tot["has_span"]:  # the round trip, and the totals' identity
        assert M.apply(ref, got, tot["first"], tot["last"]).upper() == bases.upper()
        assert len(bases) == tot["last"] - tot["first"] + 1 + tot["bases_inserted"] - tot["bases_deleted"]
    # the VCF writer's anchoring
    assert [edits.anchor(ref, r["ref_pos"], r["ref"], r["alt"], r["kind"]) for r in got] == vcf
    for r, (p, a, b) in zip(got, vcf):
        f = edits.vcf_line("ctg", ref, r).split(b"\t")
        assert f[:5] == [b"ctg", b"%d" % p, b".", a, b] and a[:1] and b[:1]  # (neither REF nor ALT is ever empty)
        assert f[7] == b"KIND=%s;OUT=%d;VERDICT=same\n" % (r["kind"].encode(), r["out_off"])


def test_model_refuses_what_the_entry_point_refuses():
    with pytest.raises(ValueError, match="decrease"):
        M.edits(b"ACGT", b"AC", [1, 0])
    with pytest.raises(ValueError, match="length"):
        M.edits(b"ACGT", b"A", [4])


def test_vcf_lines_and_summary():
    ref = b"GCAAAAATCG"
    line = edits.vcf_line("c", ref, dict(ref_pos=2, out_off=2, ref=b"", alt=b"A", kind="INS"), [21, 31], [(20, 5, 21, 0), (30, 2, 31, 2)])
    assert line == b"c\t2\t.\tC\tCA\t.\t.\tKIND=INS;OUT=2;K21=5/20,0/21;K31=2/30,2/31;VERDICT=better\n"
    assert edits.verdict([(1, 0, 1, 0)]) == "same" and edits.verdict([(1, 0, 1, 1), (1, 1, 1, 1)]) == "worse" and edits.verdict([]) == "same"
    head = edits.vcf_header([("a", 10), ("b", 7)], [21])
    assert head[0] == b"##fileformat=VCFv4.2\n" and head[2:4] == [b"##contig=<ID=a,length=10>\n", b"##contig=<ID=b,length=7>\n"]
    assert head[-1] == b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" and sum(b"ID=K21," in h for h in head) == 1
    rep = edits.EditsReport([21])
    rep.add_unpolished("short", 12)
    assert rep.summary_lines() == ["\t".join(edits.SUMMARY_HEADER) + "\n", "short\t12" + "\t0" * 17 + "\n"]
    assert rep.vcf_lines() == edits.vcf_header([("short", 12)], [21])


def test_out_pos_text_reader(tmp_path):
    p = tmp_path / "o.tsv"
    p.write_bytes(b"a\tA\t0\na\tC\t0\na\tg\t2\nb\tT\t5\n")
    got = edits.read_out_pos(str(p))
    assert list(got) == ["a", "b"] and got["a"][0].tobytes() == b"ACg" and got["a"][1].tolist() == [0, 0, 2] and got["b"][1].dtype == np.uint32
    p.write_bytes(b"a\tA\t0\nb\tC\t0\na\tG\t1\n")
    with pytest.raises(ValueError, match="two pieces"):
        edits.read_out_pos(str(p))
    p.write_bytes(b"a\tAC\t0\n")
    with pytest.raises(ValueError, match="line 1"):
        edits.read_out_pos(str(p))


# ---- 2. the kernels' rule as a one-lane host program, under the host sanitizers ------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("edits") / "edits_core_test")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(HERE, "tools", "edits_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def core_text(exe, tmp, ref, bases, pos):
    case = os.path.join(str(tmp), "case.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<II", len(ref), len(bases)) + bytes(ref) + bytes(bases) + np.asarray(pos, dtype="<u4").tobytes())
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def model_text(ref, bases, pos):
    recs, t = M.edits(ref, bases, pos)
    out = "".join("E %d %d %d %d %d %s %s\n" % (r["ref_pos"], len(r["ref"]), r["out_off"], len(r["alt"]), M.KINDS.index(r["kind"]),
                                                   r["ref"].decode() or ".", r["alt"].decode() or ".") for r in recs)
    return out + "T %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (t["has_span"], t["first"], t["last"], t["raw_runs"], t["same_runs"], *t["n_kind"],
                                                                   t["bases_inserted"], t["bases_deleted"], t["outside"])


def test_core_on_the_hand_cases(core_exe, tmp_path):
    for name, (ref, (bases, pos), _, _, _) in sorted(Cs.HAND.items()):
        assert core_text(core_exe, tmp_path, ref, bases, pos) == model_text(ref, bases, pos), name
    assert core_text(core_exe, tmp_path, b"ACGT", b"AC", [1, 0]) == "ERR 2\n"
    assert core_text(core_exe, tmp_path, b"ACGT", b"AC", [3, 4]) == "ERR 1\n"


def test_core_against_the_model_on_seeded_edits(core_exe, tmp_path):
    n_recs = 0
    for seed in range(45):
        L = [0, 1, 2, 63, 64, 65, 300, 1000, 8193][seed % 9]
        alphabet = (b"ACGTacgtN", b"ACGT", b"AC")[seed // 9 % 3]  # (two letters: homopolymers and repeats to shift through)
        span = None if seed < 27 or L < 3 else (L // 3, L - 2)
        ref, bases, pos = Cs.random_case(seed, L, rate=0.05, span=span, alphabet=alphabet)
        text = model_text(ref, bases, pos)
        assert core_text(core_exe, tmp_path, ref, bases, pos) == text, seed
        n_recs += text.count("E ")
    assert n_recs > 1000


# ---- 3. the bundle through the oracle ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def polished_bundle():
    from oracle import np2_oracle as orc
    from nextpolish2_amd.bamio import records_to_arrays
    from test_ref_bundle import bundle
    name, ref, recs, yaks = bundle()
    arr, cig, seq4, asc, asc_off = records_to_arrays(recs)
    pu = orc.front_end(ref, arr, cig, asc, asc_off, np2io.FrontOpts())
    b, p = orc.Oracle(yaks).polish(pu, Opts())
    return name, ref, b.tobytes(), np.asarray(p), yaks


def test_bundle_known_answer_and_round_trip(polished_bundle, core_exe, tmp_path):
    name, ref, bases, pos, _ = polished_bundle
    recs, tot = M.edits(ref, bases, pos)
    assert [(r["ref_pos"], r["out_off"], r["ref"], r["alt"], r["kind"]) for r in recs] == BUNDLE_EDITS
    assert tot == BUNDLE_TOTALS
    assert len(ref) == 100000 and len(bases) == 100004 and (np.diff(pos.astype(np.int64)) >= 0).all()
    assert min(b[0] - a[0] for a, b in zip(BUNDLE_EDITS, BUNDLE_EDITS[1:])) == 1484
    assert M.apply(ref, recs, tot["first"], tot["last"]) == bases  # byte for byte
    assert core_text(core_exe, tmp_path, ref, bases, pos) == model_text(ref, bases, pos)
    assert [edits.anchor(ref, r["ref_pos"], r["ref"], r["alt"], r["kind"])[0] for r in recs] == [63156, 76368, 79624, 81108]


def test_bundle_support_identity(polished_bundle):
    """the edits are at least k apart and the span is the whole contig: what the edits' windows lose in absent k-mers is
    what np2_qv loses between the committed input and output (32 -> 0 for k21, 82 -> 10 for k31)"""
    _, ref, bases, pos, yaks = polished_bundle
    recs, _ = M.edits(ref, bases, pos)
    for y, (drop_in, drop_out) in zip(yaks, ((32, 0), (82, 10))):
        t = M.Table(y)
        sup = [M.support(ref, bases, r, t) for r in recs]
        assert sum(s[1] for s in sup) - sum(s[3] for s in sup) == drop_in - drop_out
        assert [(s[0], s[2]) for s in sup] == [(y.k - 1, y.k)] * 4  # an insertion of one base: k - 1 k-mers span the join, k the base


# ---- 4. the interface ---------------------------------------------------------------------------------------------------------
def test_abi_declares_the_three_entries():
    from nextpolish2_amd import api
    L = api.lib()
    for s in ("np2_edits_buffers", "np2_edits_last", "np2_edits_free"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s)
    assert api.EDIT_DTYPE.itemsize == 20 and api.EDIT_KINDS == M.KINDS


def test_cli_rejects_edits_where_they_cannot_work(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    vcf, out = str(tmp_path / "e.vcf"), str(tmp_path / "o.fa")
    base = [sys.executable, "-m", "nextpolish2_amd.cli", BAM, ASM, os.path.join(BUNDLE, "k21.yak"), "-o", out]
    r = subprocess.run(base + ["--edits", vcf, "--out_pos"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--out_pos" in r.stderr and "--edits" in r.stderr and not os.path.exists(out)
    r = subprocess.run(base + ["--edits_summary", vcf, "--edits_min_count", "5000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--edits_min_count" in r.stderr and not os.path.exists(out)
    r = subprocess.run(base + ["--edits", vcf], capture_output=True, text=True, timeout=600,
                       env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 2 and "torchrun" in r.stderr and not os.path.exists(out) and not os.path.exists(vcf)
