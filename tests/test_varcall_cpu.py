"""The variant caller without a device: the rule (csrc/np2_varcall_core.hpp) as a stand-alone host program under the address
and undefined-behaviour sanitizers, the model of tests/varcall_model.py pinned to hand-derived answers and to the known answer
of the reference's test bundle, the host twin np2_varcall_host held to the model byte for byte, its refusals, the ABI, and the
argument handling of the nextpolish2_amd.varcall module.  tests/test_gpu_varcall.py compares the device against that model."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import varcall_model as vm
from nextpolish2_amd import api, varcall

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUNDLE_BAM = os.path.join(HERE, "golden", "ref_bundle", "hifi.map.sort.bam")
ASM = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
E_ARG = -1
ALL = dict(min_depth=1, min_alt=1, hom_pm=1000, het_pm=0)  # every allele with a read is called


# ---- 1. the core ----------------------------------------------------------------------------------------------------------------
def test_core_program_under_sanitizers(tmp_path):
    """codes, admission, the event rule, both left shifts on a hand-written contig, the key's order, the call tests at
    c * 1000 == pm * d and one below, ties, SEQ outside its buffer, L = 0"""
    exe = str(tmp_path / "varcall_core_test")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "tools", "varcall_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stderr == ""  # (a sanitizer report goes there)


# ---- 2. the model, pinned, and the host twin held to it ---------------------------------------------------------------------
def twin(ref, recs, cigar, seq4, **opts):
    """model and np2_varcall_host on one input: equal byte for byte -> the model"""
    m = vm.model(ref, recs, cigar, seq4, **opts)
    calls, st, cov, alt = api.varcall_host(ref, recs, cigar, seq4, want_counts=True, **opts)
    assert np.array_equal(cov, m["cov"]) and np.array_equal(alt, m["alt"])
    assert {k: st[k] for k in vm.STAT_KEYS} == m["stats"] and st["kernel_ms"] == 0
    assert calls.dtype.itemsize == vm.CALL_DTYPE.itemsize == 32 and calls.tobytes() == m["calls"].tobytes()
    return m


def calls_of(m):
    return [(int(c["pos"]), vm.KINDS[c["kind"]], int(c["len"]), int(c["bases"]) if c["kind"] == vm.INS else int(c["alt_code"]), int(c["count"]),
             int(c["depth"]), int(c["gt"])) for c in m["calls"]]


#      0         1         2         3
#      0123456789012345678901234567890123456789
REF = b"GATCGATTACAAAAAAGCTCGTGTGTGTCAGGCATTCAGA"


def read_of(pos, ops, ins=""):
    out, p = [], pos
    for op, n in ops:
        if op == "M":
            out.append(REF[p:p + n].decode())
            p += n
        elif op in "IS":
            out.append(ins[:n])
        elif op == "D":
            p += n
    return "".join(out)


def rec(pos, ops, ins="", flag=0, mapq=60):
    return (pos, flag, mapq, ops, read_of(pos, ops, ins))


def test_model_hand_derived_pileup_and_snv():
    # three reads over 0..9: one with C -> G at 3, one soft-clipped (an odd query start) with an N at 5
    recs = [rec(0, [("M", 10)]), (0, 0, 60, [("M", 10)], "GATGGATTAC"), (2, 0, 60, [("S", 3), ("M", 6)], "CCC" + "TCGNTT")]
    m = twin(REF, *vm.records(recs), **ALL)
    assert m["cov"][:11].tolist() == [2, 2, 3, 3, 3, 3, 3, 3, 2, 2, 0]
    assert m["alt"][3].tolist() == [0, 0, 1, 0] and int(m["alt"].sum()) == 1  # (the read N adds nothing)
    assert calls_of(m) == [(3, "SNV", 1, 2, 1, 3, 1)]
    assert m["stats"]["callable"] == 10 and m["stats"]["snv_het"] == 1
    # a lower-case reference is the same reference; a reference N has no counts and no call
    low = REF[:3] + b"n" + REF[4:].lower()
    m2 = twin(low, *vm.records(recs), **ALL)
    assert not m2["alt"].any() and len(m2["calls"]) == 0 and m2["stats"]["callable"] == 9


def test_model_hand_derived_left_shifts():
    recs = [rec(2, [("M", 8 + k), ("I", 1), ("M", 20)], "A") for k in range(1, 7)]   # one more A in 10..15, at six offsets
    recs.append(rec(12, [("M", 4), ("I", 1), ("M", 10)], "A"))                        # starts inside the run: stops at m - 1
    s = bytearray(read_of(2, [("M", 14), ("I", 1), ("M", 20)], "A").encode())
    s[11] = ord("C")
    recs.append((2, 0, 60, [("M", 14), ("I", 1), ("M", 20)], s.decode()))             # a read mismatch at 13 stops it
    recs += [rec(5, [("M", 17 + k), ("D", 2), ("M", 10)]) for k in (0, 2, 4)]          # a GT out of (GT)4, at three offsets
    m = twin(REF, *vm.records(recs), **ALL)
    assert m["alleles"] == {(9, 1, 1, 0): 6, (12, 1, 1, 0): 1, (13, 1, 1, 0): 1, (19, 0, 2, 0): 3}
    assert int(m["alt"].sum()) == 1 and m["alt"][13].tolist() == [0, 1, 0, 0]
    assert calls_of(m) == [(9, "INS", 1, 0, 6, 10, 1), (12, "INS", 1, 0, 1, 11, 1), (13, "SNV", 1, 1, 1, 11, 1), (13, "INS", 1, 0, 1, 11, 1),
                           (19, "DEL", 2, 0, 3, 11, 1)]
    # under the defaults (homozygous and heterozygous thresholds) only the six-read insertion and the deletion stay
    m = twin(REF, *vm.records(recs), het_pm=250)
    assert calls_of(m) == [(9, "INS", 1, 0, 6, 10, 1), (19, "DEL", 2, 0, 3, 11, 1)]
    assert len(twin(REF, *vm.records(recs), het_pm=800)["calls"]) == 0


def test_model_thresholds_ties_and_order():
    plain = lambda n: [rec(0, [("M", 40)])] * n
    snv = lambda p, b, n: [(0, 0, 60, [("M", 40)], REF[:p].decode() + b + REF[p + 1:].decode())] * n
    for c, gt in ((16, 2), (15, 1), (5, 1), (4, 0)):  # d = 20: hom from 16, het from 5
        m = twin(REF, *vm.records(snv(30, "T", c) + plain(20 - c)), het_pm=250)
        assert calls_of(m) == ([(30, "SNV", 1, 3, c, 20, gt)] if gt else [])
    for d, c, called in ((8, 8, True), (7, 7, False), (8, 3, True), (8, 2, False)):
        assert (len(twin(REF, *vm.records(snv(30, "T", c) + plain(d - c)), het_pm=250)["calls"]) == 1) == called
    m = twin(REF, *vm.records(snv(30, "T", 2) + snv(30, "C", 2) + plain(1)), **ALL)  # REF[30] is G: the tie goes to C
    assert calls_of(m) == [(30, "SNV", 1, 1, 2, 5, 1)]
    ins = lambda text, n: [rec(0, [("M", 31), ("I", len(text)), ("M", 9)], text)] * n
    m = twin(REF, *vm.records(ins("TC", 2) + ins("A", 2) + plain(1)), **ALL)        # equal counts: the smaller n
    assert calls_of(m) == [(30, "INS", 1, 0, 2, 5, 1)]
    m = twin(REF, *vm.records(ins("TC", 2) + ins("CC", 2) + ins("AA", 1) + plain(1)), **ALL)  # equal counts and n: the smaller bases
    assert calls_of(m) == [(30, "INS", 2, 0b0101, 2, 6, 1)]
    m = twin(REF, *vm.records(ins("TC", 3) + ins("CC", 2) + plain(1)), **ALL)       # the greater count
    assert calls_of(m) == [(30, "INS", 2, 0b1101, 3, 6, 1)]
    both = [rec(0, [("M", 31), ("D", 2), ("M", 7)])] * 2 + ins("T", 2) + snv(30, "A", 2)
    assert [c[:2] for c in calls_of(twin(REF, *vm.records(both), **ALL))] == [(30, "SNV"), (30, "DEL"), (30, "INS")]


def test_model_admission():
    ok = rec(0, [("M", 20), ("I", 1), ("M", 10)], "C")
    recs = [ok, ok[:1] + (0x100,) + ok[2:], ok[:1] + (0x800,) + ok[2:], ok[:1] + (0x400,) + ok[2:], ok[:1] + (0x200,) + ok[2:], ok[:1] + (4,) + ok[2:],
            ok[:2] + (4,) + ok[3:], ok[:2] + (5,) + ok[3:], (-1,) + ok[1:], (40,) + ok[1:], ok[:4] + (ok[4][:-1],), ok[:4] + (None,),
            rec(0, [("M", 10), ("N", 5), ("M", 10)]), (0, 0, 60, [], None), ok[:1] + (0x10,) + ok[2:]]
    m = twin(REF, *vm.records(recs), **ALL)
    st = m["stats"]
    assert (st["records_seen"], st["records_counted"], st["records_no_seq"], st["records_skipped"], st["events"]) == (15, 3, 2, 1, 3)
    assert twin(REF, *vm.records(recs), exclude_flags=0, min_mapq=0, **ALL)["stats"]["records_counted"] == 9
    none = vm.records([])
    m = twin(REF, *none, min_depth=0, min_alt=1, hom_pm=0, het_pm=0)
    assert len(m["calls"]) == 0 and m["stats"]["callable"] == 40
    m = twin(b"", *vm.records([ok]), **ALL)  # L = 0 gives nothing
    assert len(m["cov"]) == 0 and m["stats"]["records_counted"] == 0 and m["stats"]["records_seen"] == 1


def test_host_twin_on_random_records():
    rng = np.random.default_rng(20261021)
    L = 5003
    ref = bytearray(np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)[rng.choice(10, L, p=[.2225, .2225, .2225, .2225, .025, .025, .025, .025, .005, .005])].tobytes())
    ref[1000:1030] = b"A" * 30
    ref[2000:2040] = b"CA" * 20
    ref = bytes(ref)
    recs = []
    for pos in np.sort(rng.integers(-20, L + 20, 1500)):
        ops, q = [], 0
        for _ in range(int(rng.integers(1, 14))):
            ops.append(("MIDNSHP=X"[int(rng.choice(9, p=[.4, .15, .15, .01, .04, .02, .01, .12, .1]))], int(rng.integers(1, 40))))
        q = sum(n for o, n in ops if o in "MIS=X")
        s = "".join("ACGTN"[i] for i in rng.choice(5, q, p=[.245, .245, .245, .245, .02]))
        if rng.random() < 0.7:  # mostly the reference's own bases, so that shifts happen
            s, p, out = list(s), int(pos), 0
            for o, n in ops:
                if o in "M=X":
                    for j in range(n):
                        if 0 <= p + j < L and rng.random() < 0.95:
                            s[out + j] = chr(ref[p + j]).upper()
                if o in "MIS=X":
                    out += n
                if o in "MDN=X":
                    p += n
            s = "".join(s)
        recs += [(int(pos), int(rng.choice([0, 0, 0, 16, 4, 0x100])), int(rng.integers(0, 61)), ops, s if rng.random() < 0.97 else s[:-1])] * int(rng.integers(1, 4))
    arrays = vm.records(recs)
    m = twin(ref, *arrays, min_depth=2, min_alt=1, hom_pm=800, het_pm=250)
    assert m["stats"]["events"] > 300 and m["stats"]["alleles"] < m["stats"]["events"] and len(m["calls"]) > 100
    assert m["stats"]["records_no_seq"] > 5 and m["stats"]["records_skipped"] > 5
    twin(ref, *arrays, **ALL)
    twin(ref, *arrays, min_depth=4, min_alt=2, hom_pm=600, het_pm=600, max_indel=5, min_aligned_fra=0.5, exclude_flags=0x4, min_mapq=20)


@pytest.fixture(scope="module")
def bundle():
    refs, per = vm.read_bam(BUNDLE_BAM)
    text = gzip.open(ASM).read().split(b">")[1:]
    seqs = {t.split(b"\n", 1)[0].split()[0].decode(): t.split(b"\n", 1)[1].replace(b"\n", b"") for t in text}
    return refs[0][0], seqs[refs[0][0]], per[0]


def test_known_answer_on_the_bundle(bundle):
    name, ref, arrays = bundle
    m = twin(ref, *arrays, het_pm=250)  # the defaults with --het
    st = m["stats"]
    assert (st["records_seen"], st["records_counted"], st["callable"], st["events"], st["alleles"]) == (574, 574, 100000, 44283, 19093)
    assert (int(m["cov"].min()), int(m["cov"].max())) == (48, 80)
    assert [st[k] for k in vm.CALL_KEYS] == [518, 0, 202, 0, 118, 0]  # a diploid region: no homozygous call
    ins = {c[0] + 1: c for c in calls_of(m) if c[1] == "INS"}
    # the four one-base insertions --edits reports for this bundle: het INS at exactly those positions
    assert [("ACGT"[ins[p][3]],) + ins[p][4:] for p in (63156, 76368, 79624, 81108)] == [("T", 22, 70, 1), ("T", 27, 68, 1), ("A", 18, 57, 1), ("T", 20, 56, 1)]
    assert len(twin(ref, *arrays, het_pm=800)["calls"]) == 0  # het_pm = hom_pm, the command line's default
    # and the module's text is the model's
    assert varcall.vcf_header([(name, len(ref))]) + varcall.vcf_text(name, ref, m["calls"]) == vm.vcf_header_of([(name, len(ref))]) + vm.vcf_of(name, ref, m["calls"])
    assert varcall.summary_text([(name, st), ("other", st)]) == vm.summary_of([(name, st), ("other", st)])


def test_formatting_by_hand():
    calls = np.array([(3, 10, 9, 0, 0, vm.SNV, 2, 1, 2, 0), (5, 9, 3, 0, 0, vm.DEL, 1, 2, 0, 0), (5, 9, 8, 0, 0b1101, vm.INS, 2, 2, 0, 0)], dtype=vm.CALL_DTYPE)
    text = varcall.vcf_text("c", b"gatcgattac", calls)
    assert text == ("c\t4\t.\tC\tG\t.\tPASS\tKIND=SNV;DP=10;AC=9\tGT:DP:AD\t1/1:10:9\n"
                    "c\t6\t.\tATT\tA\t.\tPASS\tKIND=DEL;DP=9;AC=3\tGT:DP:AD\t0/1:9:3\n"
                    "c\t6\t.\tA\tATC\t.\tPASS\tKIND=INS;DP=9;AC=8\tGT:DP:AD\t1/1:9:8\n") == vm.vcf_of("c", b"gatcgattac", calls)
    head = varcall.vcf_header([("c", 10), ("d", 7)])
    assert head.startswith("##fileformat=VCFv4.2\n") and "##contig=<ID=c,length=10>\n##contig=<ID=d,length=7>\n" in head and head.endswith("\tFORMAT\tSAMPLE\n")
    st = dict(callable=2000000, snv_hom=3, ins_hom=1, del_hom=0, snv_het=5, ins_het=6, del_het=7)
    assert varcall.summary_text([("c", st)]) == vm.SUMMARY_HEADER + "c\t2000000\t3\t1\t0\t5\t6\t7\t2.000\ntotal\t2000000\t3\t1\t0\t5\t6\t7\t2.000\n"
    assert varcall.summary_text([]) == vm.SUMMARY_HEADER + "total\t0\t0\t0\t0\t0\t0\t0\t0.000\n" == vm.summary_of([])


# ---- 3. refusals and the ABI ----------------------------------------------------------------------------------------------------
def test_host_twin_refusals():
    L = api.lib()
    recs, cigar, seq4 = vm.records([rec(0, [("M", 10)]), rec(5, [("M", 10)])])
    ref = np.frombuffer(REF, dtype=np.uint8)

    def call(o=None, calls=True, ref_p=ref.ctypes.data, recs_p=recs.ctypes.data, cigar_p=cigar.ctypes.data, n_cig=len(cigar), seq_p=seq4.ctypes.data,
             seq_bytes=len(seq4), no_opts=False, n_pos=40):
        o = o or api.np2_varcall_opts_t(0.0, 8, 3, 800, 250, 28, 0xF04, 5)
        pc, n = C.c_void_p(), C.c_uint32()
        rc = L.np2_varcall_host(ref_p, n_pos, recs_p, len(recs), cigar_p, n_cig, seq_p, seq_bytes, None if no_opts else C.byref(o), C.byref(pc) if calls else None,
                                C.byref(n), None, None, None)
        assert not pc.value and n.value == 0
        return rc, (L.np2_io_last_error() or b"").decode()

    opts = lambda hom=800, het=250, max_indel=28, min_alt=3, fra=0.0: api.np2_varcall_opts_t(fra, 8, min_alt, hom, het, max_indel, 0xF04, 5)
    for kw, text in ((dict(o=opts(hom=1001)), "hom_pm"), (dict(o=opts(hom=500, het=501)), "het_pm"), (dict(o=opts(max_indel=0)), "max_indel"),
                     (dict(o=opts(max_indel=29)), "max_indel"), (dict(o=opts(min_alt=0)), "min_alt"), (dict(o=opts(fra=-0.5)), "min_aligned_fra"),
                     (dict(o=opts(fra=float("nan"))), "min_aligned_fra"), (dict(no_opts=True), "opts is NULL"), (dict(calls=False), "is NULL"),
                     (dict(ref_p=None), "is NULL"), (dict(recs_p=None), "is NULL"), (dict(cigar_p=None), "is NULL"), (dict(seq_p=None), "is NULL"),
                     (dict(n_cig=1), "CIGAR of record 1 outside the buffer"), (dict(seq_bytes=9), "SEQ of record 1 outside the buffer")):
        rc, msg = call(**kw)
        assert rc == E_ARG and text in msg, (kw, msg)
    assert call(n_pos=4294901761)[0] == -4  # NP2_E_UNSUPPORTED
    assert call()[0] == 0  # (and the arguments above are otherwise fine)
    with pytest.raises(api.Np2Error) as e:
        api.varcall_host(REF, recs, cigar, seq4, het_pm=900)
    assert e.value.code == E_ARG and "het_pm" in str(e.value)


def test_abi_symbols_and_struct_sizes():
    L = api.lib()
    for s in ("np2_varcall_from_records", "np2_varcall_from_bam", "np2_varcall_host"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)
    assert C.sizeof(api.np2_varcall_opts_t) == 32 and C.sizeof(api.np2_varcall_stats_t) == 136 and api.VARCALL_DTYPE.itemsize == 32
    assert api.VARCALL_DTYPE == vm.CALL_DTYPE and api.np2_varcall_stats_t.kernel_ms.offset == 104
    header = open(os.path.join(ROOT, "include", "np2_io.h")).read()
    assert "Equality with DeepVariant, bcftools or any" in header


# ---- 4. the module's arguments --------------------------------------------------------------------------------------------------
def test_defaults_and_het(tmp_path):
    out = str(tmp_path / "c.vcf")
    a = varcall.parse_args([BUNDLE_BAM, ASM, "-o", out])
    assert (a.min_depth, a.min_alt, a.hom_pm, a.het_pm, a.min_mapq, a.exclude_flags, a.min_fra, a.max_indel, a.summary) == (8, 3, 800, 800, 5, 0xF04, 0.0, 28, None)
    a = varcall.parse_args([BUNDLE_BAM, ASM, "-o", out, "--het"])
    assert (a.hom_pm, a.het_pm) == (800, 250)
    a = varcall.parse_args([BUNDLE_BAM, ASM, "-o", out, "--het", "--hom", "0.9", "--het_frac", "0.3", "-d", "10", "--min_alt", "4", "-q", "20",
                            "--exclude_flags", "0x904", "--min_fra", "0.5", "--max_indel", "20"])
    assert (a.hom_pm, a.het_pm, a.min_depth, a.min_alt, a.min_mapq, a.exclude_flags, a.min_fra, a.max_indel) == (900, 300, 10, 4, 20, 0x904, 0.5, 20)
    assert "not claimed" in " ".join(varcall.__doc__.split()) and "gVCF" in varcall.__doc__


def test_argument_errors_stop_before_the_library_loads(tmp_path):
    """run as a child: the process ends in the parser (exit 2, or the overwrite refusal) — this machine has no device, so a
    call that reached one would fail differently"""
    mod = [sys.executable, "-m", "nextpolish2_amd.varcall", BUNDLE_BAM, ASM]
    out = ["-o", str(tmp_path / "c.vcf")]
    for extra in (["--hom", "1.5"], ["--hom", "nan"], ["--het_frac", "-0.1"], ["--het", "--het_frac", "0.9"], ["-d", "-1"], ["--min_alt", "0"],
                  ["-q", "256"], ["--exclude_flags", "65536"], ["--min_fra", "1.5"], ["--max_indel", "29"], ["--max_indel", "0"]):
        r = subprocess.run(mod + out + extra, capture_output=True, text=True, timeout=600, env=ENV)
        assert r.returncode == 2 and r.stdout == "" and extra[-2] in r.stderr, (extra, r.stderr[-500:])
        with pytest.raises(SystemExit):
            varcall.parse_args([BUNDLE_BAM, ASM] + out + extra)
    r = subprocess.run(mod[:3] + [BUNDLE_BAM, str(tmp_path / "missing.fa")] + out, capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 2 and "cannot open" in r.stderr
    r = subprocess.run(mod, capture_output=True, text=True, timeout=600, env=ENV)  # -o is required
    assert r.returncode == 2
    there = tmp_path / "there.vcf"
    there.write_text("keep me\n")
    for args in (["-o", str(there)], out + ["--summary", str(there)]):
        r = subprocess.run(mod + args, capture_output=True, text=True, timeout=600, env=ENV)
        assert r.returncode != 0 and "already exists" in r.stderr and r.stdout == ""
    assert there.read_text() == "keep me\n" and not os.path.exists(out[1])
