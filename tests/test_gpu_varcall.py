"""The variant caller on the device (np2_varcall_from_records, np2_varcall_from_bam, the nextpolish2_amd.varcall module) against
the plain-Python model of tests/varcall_model.py, which tests/test_varcall_cpu.py pins to hand-derived answers: calls, cov, alt
and stats, value for value.  The record kernel walks a CIGAR 64 words and an M run 64 columns at a step, the call kernel
works on tiles of 8192 positions: the sizes below straddle both."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import varcall_model as vm
from nextpolish2_amd import Polisher, api
from nextpolish2_amd import io as np2io
from test_gpu_dirty_memory import POISON

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUNDLE_BAM = os.path.join(HERE, "golden", "ref_bundle", "hifi.map.sort.bam")
ASM = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
E_ARG = -1
TILE = 8192
LOW = dict(min_depth=2, min_alt=1, hom_pm=800, het_pm=250)  # thresholds a handful of reads reaches


@pytest.fixture(scope="module")
def pol():
    p = Polisher([])  # (no k-mer table: the caller needs the device only)
    yield p
    p.close()


def check(pol, ref, recs, cigar, seq4, **opts):
    m = vm.model(ref, recs, cigar, seq4, **opts)
    calls, st, cov, alt = api.varcall_from_records(pol, ref, recs, cigar, seq4, want_counts=True, **opts)
    assert np.array_equal(cov, m["cov"]), opts
    assert np.array_equal(alt, m["alt"]), opts
    assert {k: st[k] for k in vm.STAT_KEYS} == m["stats"], opts
    assert calls.dtype.itemsize == 32 and calls.tobytes() == m["calls"].tobytes(), (calls.tolist(), m["calls"].tolist())
    return m


def rand_ref(L, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, L)].tobytes()


def read_of(ref, pos, ops, rng=None, ins=None, err=0.0):
    """the SEQ a record with these CIGAR operations at `pos` has when it agrees with `ref` (beyond its end: A): insertions and
    clips take random bases or the texts of `ins` in turn; `err`: the rate of substituted bases in M runs"""
    rng = rng or np.random.default_rng(0)
    ins = list(ins or [])
    out, p = [], pos
    for op, n in ops:
        if op in "M=X":
            s = bytearray(ref[p:p + n].upper() + b"A" * max(0, p + n - max(len(ref), p)))
            s += b"A" * (n - len(s))
            for j in np.flatnonzero(rng.random(n) < err):
                s[j] = b"ACGT"[(b"ACGT".find(bytes([s[j]])) + 1 + int(rng.integers(0, 3))) % 4]
            out.append(bytes(s).decode())
            p += n
        elif op in "IS":
            out.append(ins.pop(0) if ins and op == "I" else "".join("ACGT"[i] for i in rng.integers(0, 4, n)))
        elif op in "DN":
            p += n
    return "".join(out)


def rec(ref, pos, ops, flag=0, mapq=60, **kw):
    return (pos, flag, mapq, ops, read_of(ref, pos, ops, **kw))


def long_cigar(n_ops):
    """n_ops operations M I M D ... of 1 to 3 bases"""
    return [("MIMD"[k % 4], 1 + k % 3) for k in range(n_ops)]


@pytest.mark.parametrize("L", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 1000003])
def test_lengths_and_cigars_against_the_model(pol, L):
    rng = np.random.default_rng(L)
    ref = rand_ref(L, L + 1)
    recs = []
    for m_run in (1, 63, 64, 65):  # M runs of these lengths, at the start, inside and overhanging the end
        for pos in (0, max(0, L - m_run), max(0, L - 1), int(rng.integers(0, L))):
            recs += [rec(ref, pos, [("M", m_run)], rng=rng, err=0.3)] * 2
            recs.append(rec(ref, pos, [("S", 3), ("M", m_run), ("I", 2), ("M", 5)], rng=rng, err=0.2))  # an odd query index: the low nibble first
    for n_ops in (1, 63, 64, 65, 129, 1000):
        for _ in range(3):
            pos = int(rng.integers(0, L))
            recs.append(rec(ref, pos, long_cigar(n_ops), rng=rng, err=0.1))
            recs.append(rec(ref, pos, [("=", 2)] + long_cigar(n_ops)[::-1] + [("X", 1)], rng=rng, err=0.1))
    if L > 100000:  # enough reads for calls in every block of the call kernel
        for p in rng.integers(0, L, 3000):
            n = int(rng.integers(200, 1500))
            recs.append(rec(ref, int(p), [("M", n // 2), ("I", 1), ("M", n - n // 2), ("D", 2), ("M", 30)], rng=rng, err=0.02))
    arrays = vm.records(recs)
    m = check(pol, ref, *arrays, **LOW)
    assert m["stats"]["records_counted"] == len(recs)
    m0 = check(pol, ref, *arrays, min_depth=1, min_alt=1, hom_pm=1000, het_pm=0)
    assert sum(m0["stats"][k] for k in vm.CALL_KEYS) >= 1 and (L < 64 or m["stats"]["events"] > 100)
    check(pol, ref, *arrays, min_depth=3, min_alt=2, hom_pm=500, het_pm=500, max_indel=1)
    calls, _, cov, alt = api.varcall_from_records(pol, ref, *arrays, **LOW)  # the per-base arrays stay on the device
    assert cov is None and alt is None and calls.tobytes() == m["calls"].tobytes()


def test_left_shift(pol):
    #      0         1         2         3
    #      0123456789012345678901234567890123456789
    ref = b"GATCGATTACAAAAAAGCTCGTGTGTGTCAGGCATTCAGA"
    L = len(ref)
    # one more A in the run 10..15, written at different offsets by different reads: all collapse onto anchor 9
    recs = [rec(ref, 2, [("M", 8 + k), ("I", 1), ("M", 20)], ins=["A"]) for k in range(1, 7)]
    # the same insertion in a read that starts inside the run: the shift stops at m - 1 (the run's first column stays)
    recs.append(rec(ref, 12, [("M", 4), ("I", 1), ("M", 10)], ins=["A"]))
    # ... and in a read with a mismatch inside the run: the shift stops there
    s = bytearray(read_of(ref, 2, [("M", 14), ("I", 1), ("M", 20)], ins=["A"]).encode())
    s[11] = ord("C")  # reference position 13
    recs.append((2, 0, 60, [("M", 14), ("I", 1), ("M", 20)], s.decode()))
    # a GT deleted from (GT)4 at 20..27, at three offsets: all collapse onto anchor 19
    for k in (0, 2, 4):
        recs.append(rec(ref, 5, [("M", 17 + k), ("D", 2), ("M", 10)]))
    arrays = vm.records(recs)
    m = check(pol, ref, *arrays, min_depth=1, min_alt=1, hom_pm=1000, het_pm=0)
    assert m["alleles"] == {(9, 1, 1, 0): 6, (12, 1, 1, 0): 1, (13, 1, 1, 0): 1, (19, 0, 2, 0): 3}
    assert m["stats"]["events"] == 11 and m["stats"]["alleles"] == 4
    assert not m["alt"][:13].any() and m["alt"][13].tolist() == [0, 1, 0, 0]


def test_indel_admission(pol):
    ref = bytearray(rand_ref(300, 5))
    ref[150] = ord("N")
    ref = bytes(ref)
    L = len(ref)
    big = lambda n, op: rec(ref, 10, [("M", 40), (op, n), ("M", 40)])
    recs = [big(28, "I"), big(29, "I"), big(28, "D"), big(29, "D")]
    recs.append(rec(ref, 20, [("M", 30), ("I", 3), ("M", 30)], ins=["ANC"]))              # an N in the insertion
    s = bytearray(read_of(ref, 60, [("M", 30), ("I", 2), ("M", 30)], ins=["TT"]).encode())
    s[29] = ord("N")                                                                        # an N in the read, at the anchor
    recs.append((60, 0, 60, [("M", 30), ("I", 2), ("M", 30)], s.decode()))
    recs.append(rec(ref, 140, [("M", 11), ("D", 2), ("M", 20)]))                            # anchored on the reference N
    recs.append(rec(ref, 140, [("M", 10), ("I", 2), ("M", 20)], ins=["GG"]))                # before the reference N
    recs.append(rec(ref, 30, [("S", 5), ("I", 2), ("M", 30), ("D", 2), ("S", 4)]))          # next to clips
    recs.append(rec(ref, 30, [("I", 2), ("M", 30), ("D", 2)]))                              # leading and trailing
    recs.append(rec(ref, 30, [("M", 20), ("I", 2), ("D", 3), ("M", 20)]))                   # adjacent I and D
    recs.append(rec(ref, 30, [("M", 20), ("D", 3), ("I", 2), ("M", 20)]))
    recs.append(rec(ref, 30, [("H", 5), ("M", 20), ("P", 1), ("D", 3), ("M", 20)]))         # a pad before the deletion
    recs.append(rec(ref, L - 10, [("M", 8), ("D", 2), ("M", 5)]))                           # a + n = L - 1: inside
    recs.append(rec(ref, L - 10, [("M", 8), ("D", 3), ("M", 5)]))                           # a + n = L: touches L
    recs.append(rec(ref, L - 10, [("M", 9), ("I", 1), ("M", 5)]))                           # a + 1 = L - 1: inside
    recs.append(rec(ref, L - 10, [("M", 10), ("I", 1), ("M", 5)]))                          # a + 1 = L
    recs.append(rec(ref, 100, [("=", 10), ("X", 1), ("=", 10), ("I", 1), ("X", 2), ("D", 1), ("=", 5)]))  # runs of =/X
    arrays = vm.records(recs)
    m = check(pol, ref, *arrays, min_depth=1, min_alt=1, hom_pm=1000, het_pm=0)
    lens = sorted((kd, n) for (_, kd, n, _) in m["alleles"])
    assert (1, 28) in lens and (0, 28) in lens and (1, 29) not in lens and (0, 29) not in lens
    assert m["stats"]["events"] == 2 + 1 + 2 + 2 + 2  # n = 28 twice, the read N, the reference N twice, inside L twice, =/X twice
    assert (150, 0, 2, 0) in m["alleles"]  # (no shift off a reference N)
    m5 = check(pol, ref, *arrays, min_depth=1, min_alt=1, hom_pm=1000, het_pm=0, max_indel=1)
    assert m5["stats"]["events"] == 3


def test_thresholds_and_ties(pol):
    ref = b"ACGTTGCATGCCATGGATCCAGTTGACCAT" * 4
    L = len(ref)
    plain = lambda n: [rec(ref, 0, [("M", L)])] * n
    snv = lambda p, b, n: [(0, 0, 60, [("M", L)], ref[:p].decode() + b + ref[p + 1:].decode())] * n
    # c * 1000 == pm * d exactly and one read below, for both thresholds (d = 20: hom at 16, het at 5)
    for c, gt in ((16, 2), (15, 1), (5, 1), (4, 0)):
        m = check(pol, ref, *vm.records(snv(40, "A", c) + plain(20 - c)), min_depth=8, min_alt=3, hom_pm=800, het_pm=250)
        assert [(x["pos"], x["gt"], x["count"], x["depth"]) for x in m["calls"]] == ([(40, gt, c, 20)] if gt else [])
    # d = min_depth and min_depth - 1; c = min_alt and min_alt - 1
    for d, c, called in ((8, 8, True), (7, 7, False), (8, 3, True), (8, 2, False)):
        m = check(pol, ref, *vm.records(snv(40, "A", c) + plain(d - c)), min_depth=8, min_alt=3, hom_pm=800, het_pm=250)
        assert (len(m["calls"]) == 1) == called
    # SNV ties go A < C < G < T (the reference base at 41 is C)
    assert ref[41:42] == b"C"
    m = check(pol, ref, *vm.records(snv(41, "T", 3) + snv(41, "G", 3) + plain(2)), **LOW)
    assert [(x["pos"], x["alt_code"], x["count"]) for x in m["calls"]] == [(41, 2, 3)]
    # allele ties: by count the greater, then the smaller n, then the smaller bases
    ins = lambda text, n: [rec(ref, 0, [("M", 51), ("I", len(text)), ("M", L - 51)], ins=[text])] * n
    for group, want in (((("GG", 3), ("C", 2)), (2, 0b1010, 3)), ((("GG", 2), ("C", 2)), (1, 1, 2)), ((("TC", 2), ("GC", 2), ("CT", 1)), (2, 0b1001, 2))):
        m = check(pol, ref, *vm.records(sum((ins(t, n) for t, n in group), []) + plain(1)), **LOW)
        assert [(x["pos"], x["kind"], x["len"], x["bases"], x["count"]) for x in m["calls"]] == [(50, vm.INS) + want]
    # an SNV, a DEL and an INS at one position come out in that order
    both = [rec(ref, 0, [("M", 61), ("D", 2), ("M", L - 63)])] * 3 + [rec(ref, 0, [("M", 61), ("I", 1), ("M", L - 61)], ins=["C"])] * 3
    m = check(pol, ref, *vm.records(snv(60, "C" if ref[60:61] != b"C" else "G", 3) + both + plain(1)), **LOW)
    assert [(x["pos"], x["kind"]) for x in m["calls"]] == [(60, vm.SNV), (60, vm.DEL), (60, vm.INS)]
    # het_pm = hom_pm: homozygous calls only
    m = check(pol, ref, *vm.records(snv(40, "A", 15) + plain(5)), min_depth=8, min_alt=3, hom_pm=800, het_pm=800)
    assert len(m["calls"]) == 0


def test_records_not_counted(pol):
    ref = rand_ref(500, 9)
    ok = rec(ref, 100, [("M", 50), ("I", 1), ("M", 50)], ins=["G"], err=0.1, rng=np.random.default_rng(1))
    recs = [ok] * 3
    for flag in (0x4, 0x100, 0x200, 0x400, 0x800):
        recs.append(ok[:1] + (flag,) + ok[2:])
    recs.append(ok[:2] + (4,) + ok[3:])                                   # mapq below 5
    recs.append((-1,) + ok[1:])                                           # pos < 0
    recs.append((500,) + ok[1:])                                          # pos >= L
    recs.append(ok[:4] + (ok[4][:-1],))                                   # l_seq one short
    recs.append(ok[:4] + (None,))                                         # SEQ *
    recs.append(rec(ref, 100, [("M", 20), ("N", 30), ("M", 20)]))         # an N operation
    recs.append((100, 0, 60, [], None))                                   # no CIGAR
    recs.append(ok[:1] + (0x10,) + ok[2:])                                # the reverse strand counts
    arrays = vm.records(recs)
    m = check(pol, ref, *arrays, **LOW)
    st = m["stats"]
    assert (st["records_seen"], st["records_counted"], st["records_no_seq"], st["records_skipped"]) == (len(recs), 4, 2, 1)
    assert int(m["cov"].max()) == 4
    m = check(pol, ref, *arrays, exclude_flags=0, min_mapq=0, **LOW)
    assert m["stats"]["records_counted"] == 10
    check(pol, ref, *arrays, min_aligned_fra=1.0, **LOW)


def test_no_records_and_no_positions(pol):
    none = vm.records([])
    for L in (1, 64, TILE, 2 * TILE + 1):
        m = check(pol, rand_ref(L, L), *none, min_depth=0, min_alt=1, hom_pm=0, het_pm=0)
        assert len(m["calls"]) == 0 and m["stats"]["callable"] == L
    calls, st, cov, alt = api.varcall_from_records(pol, b"", *vm.records([(0, 0, 60, [("M", 5)], "ACGTA")]), want_counts=True)  # L = 0 gives nothing
    assert len(calls) == 0 and len(cov) == 0 and alt.shape == (0, 4) and st["records_seen"] == 1 and st["records_counted"] == 0


# ---- from an indexed BAM, on both fetch paths ---------------------------------------------------------------------------------
def bundle():
    refs, per = vm.read_bam(BUNDLE_BAM)
    text = gzip.open(ASM).read().split(b">")[1:]
    seqs = {t.split(b"\n", 1)[0].split()[0].decode(): t.split(b"\n", 1)[1].replace(b"\n", b"") for t in text}
    return refs[0][0], seqs[refs[0][0]], per[0]


@pytest.fixture(scope="module")
def bundle_model():
    name, ref, arrays = bundle()
    return name, ref, vm.model(ref, *arrays, het_pm=250)


_CHILD = ("import json, sys\n"
          "sys.path.insert(0, %r)\n"
          "import numpy as np\n"
          "from nextpolish2_amd import Polisher, api, io as np2io\n"
          "pol = Polisher([])\n"
          "bam = np2io.Bam(sys.argv[1])\n"
          "ref = dict(np2io.read_fasta(sys.argv[2]))[bam.refs()[0][0]]\n"
          "calls, st, cov, alt = api.varcall_from_bam(pol, bam, bam.refs()[0][0], ref, het_pm=250, want_counts=True)\n"
          "np.savez(sys.argv[3], calls=calls, cov=cov, alt=alt)\n"
          "print('RESULT ' + json.dumps(st))\n" % ROOT)


@pytest.mark.parametrize("mode", ["gpu", "libdeflate"])
def test_bundle_bam_on_both_fetch_paths(tmp_path, bundle_model, mode):
    npz = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, BUNDLE_BAM, ASM, npz], capture_output=True, text=True,
                       env=dict(os.environ, NP2_INFLATE=mode, NP2_IO_PROFILE="1"), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert ("fetch_records_gpu" in r.stderr) == (mode == "gpu"), r.stderr[-2000:]  # (the path asked for really ran)
    st = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    _, _, m = bundle_model
    got = np.load(npz)
    assert {k: st[k] for k in vm.STAT_KEYS} == m["stats"]
    assert np.array_equal(got["cov"], m["cov"]) and np.array_equal(got["alt"], m["alt"]) and got["calls"].tobytes() == m["calls"].tobytes()
    # the known answer of the bundle (a diploid region: no homozygous call)
    assert (st["records_seen"], st["records_counted"], st["callable"], st["events"], st["alleles"]) == (574, 574, 100000, 44283, 19093)
    assert (int(got["cov"].min()), int(got["cov"].max())) == (48, 80)
    assert [st[k] for k in vm.CALL_KEYS] == [518, 0, 202, 0, 118, 0]
    # the four one-base insertions --edits reports for this bundle are het INS at exactly those positions
    ins = {int(c["pos"]) + 1: ("ACGT"[int(c["bases"])], int(c["count"]), int(c["depth"]), int(c["gt"])) for c in got["calls"] if c["kind"] == vm.INS and c["len"] == 1}
    assert [ins[p] for p in (63156, 76368, 79624, 81108)] == [("T", 22, 70, 1), ("T", 27, 68, 1), ("A", 18, 57, 1), ("T", 20, 56, 1)]


_POISON_CODE = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import numpy as np\n"
                "import test_gpu_varcall as t\n"
                "from nextpolish2_amd import Polisher, api\n"
                "byte, out = int(sys.argv[1]), sys.argv[2]\n"
                "try:\n"
                "    with api.alloc_poison(byte):\n"
                "        p = Polisher([])\n"
                "        for i, k in enumerate('ABA'):\n"
                "            ref, arrays = t.poison_inputs()[k]\n"
                "            calls, st, cov, alt = api.varcall_from_records(p, ref, *arrays, want_counts=True, **t.LOW)\n"
                "            np.savez('%%s.%%d.npz' %% (out, i), calls=calls, cov=cov, alt=alt, stats=np.array([st[k] for k in t.vm.STAT_KEYS]))\n"
                "        p.close()\n"
                "    assert api.alloc_poison_stats()[0] > 0\n"
                "except api.Np2Error as e:\n"
                "    print(e, file=sys.stderr)\n"
                "    sys.exit(3 if e.code == -2 else 1)\n" % (ROOT, HERE))


def poison_inputs():
    """a small contig A and a larger one B with many more events and calls"""
    out = {}
    for k, L, n in (("A", 3001, 60), ("B", 40009, 1500)):
        rng = np.random.default_rng(L)
        ref = rand_ref(L, L)
        recs = []
        for p in np.sort(rng.integers(0, L - 500, n)):
            recs.append(rec(ref, int(p), [("S", 3), ("M", 100), ("I", 2), ("M", 150), ("D", 3), ("M", 200)], rng=rng, err=0.03))
        out[k] = (ref, vm.records(recs))
    return out


@pytest.mark.parametrize("byte", POISON)
def test_on_poisoned_recycled_blocks(tmp_path, byte):
    """A, the larger B and A again on one context, every pool block filled with `byte` before it is handed out: both A results
    are the model's (the second runs in buffers sized and dirtied by B).  A process of its own: the hook's counters are the
    process's."""
    out = str(tmp_path / "w")
    r = subprocess.run([sys.executable, "-c", _POISON_CODE, str(byte), out], capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    if r.returncode == 3 or r.returncode < 0:
        pytest.exit(f"device error in the variant caller under poison {byte:#x}: {r.stderr.decode(errors='replace')[-2000:]}", returncode=3)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    inputs = poison_inputs()
    for i, k in enumerate("ABA"):
        ref, arrays = inputs[k]
        m = vm.model(ref, *arrays, **LOW)
        got = np.load(f"{out}.{i}.npz")
        assert np.array_equal(got["cov"], m["cov"]) and np.array_equal(got["alt"], m["alt"]), (k, byte)
        assert got["calls"].tobytes() == m["calls"].tobytes() and got["stats"].tolist() == [m["stats"][s] for s in vm.STAT_KEYS], (k, byte)
        assert len(m["calls"]) > 10


def test_module_end_to_end_on_the_bundle(tmp_path, bundle_model):
    name, ref, m = bundle_model
    vcf, vgz, tsv = (str(tmp_path / f) for f in ("calls.vcf", "calls.vcf.gz", "calls.tsv"))
    cmd = [sys.executable, "-m", "nextpolish2_amd.varcall", BUNDLE_BAM, ASM]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd + ["-o", vcf, "--summary", tsv, "--het"], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    want = vm.vcf_header_of([(name, len(ref))]) + vm.vcf_of(name, ref, m["calls"])
    assert open(vcf).read() == want and want.count("\n") == 10 + 838
    assert open(tsv).read() == vm.summary_of([(name, m["stats"])])
    assert "\t63156\t.\t" in want and "KIND=INS;DP=70;AC=22\tGT:DP:AD\t0/1:70:22\n" in want
    # the default is homozygous calls only (none in this diploid region); .gz is BGZF, gzip reads it
    r = subprocess.run(cmd + ["-o", vgz], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    raw = open(vgz, "rb").read()
    assert raw[:4] == b"\x1f\x8b\x08\x04" and raw[12:14] == b"BC"
    assert gzip.decompress(raw).decode() == vm.vcf_header_of([(name, len(ref))])
    r = subprocess.run(cmd + ["-o", vgz], capture_output=True, env=env, timeout=600)  # not overwritten
    assert r.returncode != 0 and b"already exists" in r.stderr


def test_argument_errors_leave_the_context_usable(pol):
    L = api.lib()
    ref = rand_ref(100, 1)
    recs, cigar, seq4 = vm.records([rec(ref, 5, [("M", 10)]), rec(ref, 8, [("M", 10)])])
    refa = np.frombuffer(ref, dtype=np.uint8)
    bam = np2io.Bam(BUNDLE_BAM)

    def opts(hom=800, het=250, max_indel=28, min_alt=3, fra=0.0):
        return api.np2_varcall_opts_t(fra, 8, min_alt, hom, het, max_indel, 0xF04, 5)

    def from_records(o=None, calls=True, ref_p=refa.ctypes.data, recs_p=recs.ctypes.data, cigar_p=cigar.ctypes.data, seq_p=seq4.ctypes.data, no_opts=False):
        o = o or opts()
        pc, n = C.c_void_p(), C.c_uint32()
        rc = L.np2_varcall_from_records(pol._h, ref_p, 100, recs_p, len(recs), cigar_p, seq_p, None if no_opts else C.byref(o),
                                        C.byref(pc) if calls else None, C.byref(n), None, None, None)
        assert rc != 0 and not pc.value and n.value == 0
        return rc

    def from_bam(o=None, name=b"x", bam_h=bam._h):
        pc, n = C.c_void_p(), C.c_uint32()
        rc = L.np2_varcall_from_bam(pol._h, bam_h, name, refa.ctypes.data, 100, C.byref(o or opts()), C.byref(pc), C.byref(n), None, None, None)
        assert rc != 0 and not pc.value and n.value == 0
        return rc

    cases = [(lambda: from_records(opts(hom=1001)), "hom_pm"), (lambda: from_records(opts(hom=500, het=501)), "het_pm"),
             (lambda: from_records(opts(max_indel=0)), "max_indel"), (lambda: from_records(opts(max_indel=29)), "max_indel"),
             (lambda: from_records(opts(min_alt=0)), "min_alt"), (lambda: from_records(opts(fra=1.5)), "min_aligned_fra"),
             (lambda: from_records(opts(fra=float("nan"))), "min_aligned_fra"), (lambda: from_records(no_opts=True), "opts is NULL"),
             (lambda: from_records(calls=False), "is NULL"), (lambda: from_records(ref_p=None), "ref is NULL"),
             (lambda: from_records(recs_p=None), "recs is NULL"), (lambda: from_records(cigar_p=None), "cigar is NULL"),
             (lambda: from_records(seq_p=None), "seq4 is NULL"), (lambda: from_bam(name=b"no_such_contig"), "contig not in the BAM header"),
             (lambda: from_bam(opts(het=900)), "het_pm"), (lambda: from_bam(bam_h=None), "is NULL")]
    for fn, text in cases:
        assert fn() == E_ARG
        assert text in L.np2_last_error(pol._h).decode(), text
        _, st, cov, _ = api.varcall_from_records(pol, ref, recs, cigar, seq4, want_counts=True)  # the context still answers
        assert st["records_counted"] == 2 and cov[4:19].tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 0]
    assert L.np2_varcall_from_records(None, None, 0, None, 0, None, None, None, None, None, None, None, None) == E_ARG
    assert L.np2_varcall_from_bam(None, None, None, None, 0, None, None, None, None, None, None) == E_ARG
    bam.close()
