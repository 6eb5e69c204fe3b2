"""The BAM writer on the device (np2_bamout.hip, np2_bamout_host.cpp: Sam.write_bam, Sam.bam_stream, the samsort module and
cli --sorted_bam) against its host twin and the plain-Python model of the rule (tests/bamout_model.py), byte for byte; the
written files through the project's own readers; and the whole path on recycled, poisoned memory."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bamout_model as bm
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.bamio import pileup_to_records, read_bam, write_bam, write_sam
from nextpolish2_amd.synth import Synth
from test_frontend_cpu import same_pileup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNDLE = os.path.join(ROOT, "tests", "golden", "ref_bundle")
ASM = os.path.join(ROOT, "tests", "golden", "ref_test_asm.fa.gz")
E_ARG, E_DEVICE, E_UNSUPPORTED = -1, -2, -4


def device_error(e, what):
    """nothing more may run on a device that has reported an error: the session ends here"""
    pytest.exit(f"device error in {what}: {e}", returncode=3)


def shuffled(recs, seed=3):
    return [recs[k] for k in np.random.default_rng(seed).permutation(len(recs))]


def sam_file(tmp_path, refs, recs, name="in.sam"):
    path = str(tmp_path / name)
    write_sam(path, refs, recs)
    return path


def device_files(pol, sam_path, tie, out, keep_stream=True):
    """-> (stream, bam bytes, bai bytes, stats, (export arrays + names)) of one SAM text through the device"""
    sam = np2io.Sam(pol, [sam_path], tie=tie, keep_names=True)
    try:
        S = sam.bam_stream(pol) if keep_stream else None
        st = sam.write_bam(pol, out)
        arrays = sam.export(pol) + sam.export_names(pol)
    finally:
        sam.close()
    return S, open(out, "rb").read(), open(out + ".bai", "rb").read(), st, arrays


@pytest.fixture(scope="module")
def pol():
    p = Polisher([])
    yield p
    p.close()


# ---- 1. the hand-built shapes: device == host twin == model -------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [None, 1])
@pytest.mark.parametrize("case,tie", [(c, "strand") for c in sorted(bm.CASES)] + [("bins", "input"), ("small", "input")])
def test_shapes_equal_the_host_twin_and_the_model(pol, tmp_path, monkeypatch, case, tie, batch):
    if batch is not None:
        monkeypatch.setenv("NP2_BGZF_TEST_BATCH", str(batch))
    refs, recs = bm.CASES[case]()
    given = shuffled(recs)
    want = bm.sort_records(given, tie)
    try:
        S, bam, bai, st, arrays = device_files(pol, sam_file(tmp_path, refs, given), tie, str(tmp_path / "dev.bam"))
    except Np2Error as e:
        if e.code == E_DEVICE:
            device_error(e, case)
        raise
    model_S, _ = bm.stream(refs, want)
    assert S == model_S, (case, len(S), len(model_S), next((i for i, (a, b) in enumerate(zip(S, model_S)) if a != b), None))
    twin_S, twin_st = np2io.bamout_host(*arrays, refs, path=str(tmp_path / "twin.bam"))
    assert twin_S == S
    assert bam == open(tmp_path / "twin.bam", "rb").read() and bai == open(tmp_path / "twin.bam.bai", "rb").read()
    assert bam == np2io.bgzf_deflate_host(model_S)
    bm.check_files(refs, want, bam, bai, case)
    counts = ("records", "stream_bytes", "file_bytes", "blocks", "bins", "chunks")
    assert {k: st[k] for k in counts} == {k: twin_st[k] for k in counts} and st["records"] == len(want)
    if case == "long" and batch == 1:
        assert st["blocks"] == 3


# ---- 2. refusals: no file, the context stays usable -----------------------------------------------------------------------------------
def test_refusals_leave_no_file_and_a_usable_context(pol, tmp_path):
    out = str(tmp_path / "refused.bam")
    for case, (refs, recs, status) in sorted(bm.REFUSED.items()):
        sam = np2io.Sam(pol, [sam_file(tmp_path, refs, recs, case + ".sam")], keep_names=True)
        for call in (lambda: sam.write_bam(pol, out), lambda: sam.bam_stream(pol)):
            with pytest.raises(Np2Error) as e:
                call()
            assert e.value.code == status, (case, str(e.value))
        assert ("c1" in str(e.value)) if case == "ln_too_large" else ("record" in str(e.value)), str(e.value)
        sam.close()
        assert not os.path.exists(out) and not os.path.exists(out + ".bai"), case
    # a 255-byte and an empty QNAME are refused when the names are kept, naming the line; without names they are not looked at
    refs, good = bm.case_small()
    for bad, line in ((b"n" * 255, 6), (b"", 7)):
        recs = good[:line - 5] + [bm.rec(0, 5, [("M", 4)], name=bad)] + good[4:]  # (four header lines: the first record is line 5)
        path = sam_file(tmp_path, refs, recs, "name%d.sam" % line)
        with pytest.raises(Np2Error, match="line %d: QNAME" % line) as e:
            np2io.Sam(pol, [path], keep_names=True)
        assert e.value.code == E_ARG
        np2io.Sam(pol, [path]).close()
    # a handle without names
    path = sam_file(tmp_path, refs, good, "good.sam")
    sam = np2io.Sam(pol, [path])
    for call in (lambda: sam.write_bam(pol, out), lambda: sam.bam_stream(pol), lambda: sam.export_names(pol)):
        with pytest.raises(Np2Error, match="NP2_SAM_KEEP_NAMES") as e:
            call()
        assert e.value.code == E_ARG
    sam.close()
    assert not os.path.exists(out) and not os.path.exists(out + ".bai")
    # a path that cannot be created leaves nothing either, and the context goes on
    sam = np2io.Sam(pol, [path], keep_names=True)
    with pytest.raises(Np2Error, match="cannot open"):
        sam.write_bam(pol, str(tmp_path / "no_such_dir" / "x.bam"))
    S, bam, bai, _, _ = device_files(pol, path, "strand", out)
    sam.close()
    bm.check_files(refs, bm.sort_records(good), bam, bai, "after the refusals")


# ---- 3. round trips through the project's own readers ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_refs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamout")
    s1 = Synth(30000, depth=20, seed=71, diploid=True, read_len_mean=5000.0, name="ctgA")
    s2 = Synth(20000, depth=15, seed=72, name="ctgB")
    recs = pileup_to_records(s1.pileup, tid=0, rng=np.random.default_rng(5), decorate=True) + \
        pileup_to_records(s2.pileup, tid=1, rng=np.random.default_rng(6), decorate=True)
    refs = [("ctgA", s1.pileup.L), ("ctgB", s2.pileup.L)]
    given = shuffled(recs, 8)
    for i, r in enumerate(given):
        r["name"] = b"read%d" % i
    sam = str(tmp / "shuffled.sam")
    write_sam(sam, refs, given)
    return (s1, s2), refs, given, sam, tmp


def run_module(module, args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd." + module] + args, capture_output=True, env=env, timeout=600, **kw)


@pytest.fixture(scope="module")
def samsorted(two_refs):
    _, refs, given, sam, tmp = two_refs
    out = str(tmp / "sorted.bam")
    r = run_module("samsort", [sam, "-o", out])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"[samsort]" in r.stderr
    bm.check_files(refs, bm.sort_records(given), open(out, "rb").read(), open(out + ".bai", "rb").read(), "samsort")
    return out


@pytest.mark.parametrize("mode", ["gpu", "host"])
def test_the_written_bam_gives_the_pileup_of_the_text(pol, two_refs, samsorted, monkeypatch, mode):
    synths, refs, _, sam_path, _ = two_refs
    monkeypatch.setenv("NP2_INFLATE", mode)  # (read at every fetch)
    sam, bam = np2io.Sam(pol, [sam_path]), np2io.Bam(samsorted)
    assert bam.refs() == refs
    for (name, _), s in zip(refs, synths):
        ref = s.pileup.ref
        want = np2io.export_contig(pol, np2io.contig_from_sam(pol, sam, name, ref.tobytes()), ref)
        got = np2io.export_contig(pol, np2io.contig_from_bam(pol, bam, name, ref.tobytes()), ref)
        assert len(want.reads) > 10 and same_pileup(got, want), (name, mode)
    sam.close(), bam.close()


@pytest.mark.parametrize("mode", ["gpu", "host"])
def test_use_secondary_finds_the_primary_by_the_written_names(pol, tmp_path, monkeypatch, mode):
    s = Synth(20000, depth=15, seed=72, name="ctgB")
    recs = pileup_to_records(s.pileup, tid=0, rng=np.random.default_rng(6))  # (undecorated: every secondary below has its primary)
    refs = [("ctgB", s.pileup.L)]
    for i, r in enumerate(recs):
        r["name"] = b"read%d" % i
    prim = [r for r in recs if not r.get("flag", 0) & 0x900 and 3000 < len(r["seq"]) < 9000][:5]
    assert len(prim) >= 2
    for p in prim:  # a secondary record without SEQ whose primary is in the file: the same alignment, so that it is admitted
        recs.append(dict(p, flag=p.get("flag", 0) & 16 | 0x100, seq=""))
    given = shuffled(recs, 4)
    want_order = bm.sort_records(given)
    write_bam(str(tmp_path / "model.bam"), refs, want_order)
    dev = str(tmp_path / "dev.bam")
    device_files(pol, sam_file(tmp_path, refs, given), "strand", dev, keep_stream=False)
    monkeypatch.setenv("NP2_INFLATE", mode)
    fo = np2io.FrontOpts(use_secondary=True)
    ref = s.pileup.ref
    piles = []
    for path in (str(tmp_path / "model.bam"), dev):
        bam = np2io.Bam(path)
        piles.append(np2io.export_contig(pol, np2io.contig_from_bam(pol, bam, "ctgB", ref.tobytes(), fo), ref))
        bam.close()
    assert same_pileup(piles[1], piles[0])
    bam = np2io.Bam(dev)  # ... and the secondary records are what makes the difference
    plain = np2io.export_contig(pol, np2io.contig_from_bam(pol, bam, "ctgB", ref.tobytes()), ref)
    bam.close()
    assert piles[1].n_reads > plain.n_reads


def test_lowdepth_on_the_written_bam(two_refs, samsorted):
    synths, refs, given, _, tmp = two_refs
    write_bam(str(tmp / "model.bam"), refs, bm.sort_records(given))
    fa = tmp / "genome.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s.pileup.ref.tobytes()) for (n, _), s in zip(refs, synths)))
    outs = []
    for bam in (str(tmp / "model.bam"), samsorted):
        bed = str(tmp / (os.path.basename(bam) + ".bed"))
        r = run_module("lowdepth", [bam, str(fa), "-d", "12", "-l", "500", "--bed", bed])
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        outs.append((r.stdout, open(bed, "rb").read()))
    assert outs[0] == outs[1] and outs[0][0].count(b">") >= 1


def test_cli_sorted_bam_from_a_stream(two_refs, samsorted):
    from test_oracle import yak_from_seqs
    synths, refs, _, sam, tmp = two_refs
    with gzip.open(tmp / "g.fa.gz", "wt") as f:
        for (nm, _), s in zip(refs, synths):
            f.write(f">{nm}\n{s.pileup.ref.tobytes().decode()}\n")
    haps = [synths[0].hap1.decode(), synths[0].hap2.decode(), synths[1].hap1.decode()]
    np2io.write_yak(str(tmp / "k21.yak"), yak_from_seqs(haps, 21))
    np2io.write_yak(str(tmp / "k31.yak"), yak_from_seqs(haps, 31))
    rest = [str(tmp / "g.fa.gz"), str(tmp / "k21.yak"), str(tmp / "k31.yak")]
    r = run_module("cli", ["-L", "10000", sam] + rest)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    want = r.stdout
    assert want.count(b">") == 2
    kept = str(tmp / "kept.bam")
    with open(sam, "rb") as text:  # the stream cannot be read twice: one pass polishes and keeps the mapping
        r = run_module("cli", ["-L", "10000", "-", "--sorted_bam", kept] + rest, stdin=text)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == want
    assert open(kept, "rb").read() == open(samsorted, "rb").read() and open(kept + ".bai", "rb").read() == open(samsorted + ".bai", "rb").read()
    r = run_module("cli", ["-L", "10000", samsorted, "--sorted_bam", str(tmp / "again.bam")] + rest)  # a BAM is sorted already
    assert r.returncode != 0 and b"--sorted_bam" in r.stderr and not os.path.exists(tmp / "again.bam")


def test_reference_bundle_through_the_written_bam(tmp_path):
    refs, recs = read_bam(os.path.join(BUNDLE, "hifi.map.sort.bam"))
    assert len(recs) == 574
    sam = sam_file(tmp_path, refs, recs, "bundle.sam")  # in file order
    out = str(tmp_path / "bundle.sort.bam")
    r = run_module("samsort", [sam, "-o", out, "--sam_tie", "input"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got_refs, got = read_bam(out)
    assert got_refs == refs and [(g["name"], g["pos"], g["flag"]) for g in got] == [(w["name"], w["pos"], w["flag"]) for w in recs]
    r = run_module("cli", ["-L", "1000", out, ASM, os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == gzip.open(os.path.join(BUNDLE, "expected.fa.gz"), "rb").read()


# ---- 4. recycled memory: the scheme of test_gpu_dirty_memory.py ------------------------------------------------------------------------
def poison_inputs():
    refs, a = bm.case_bins()
    _, b = bm.case_cuts()
    return refs, {"A": shuffled(a, 1), "B": shuffled(b + a[:12], 2)}


_POISON_CODE = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import test_gpu_bamout as t\n"
                "from nextpolish2_amd import Polisher, api\n"
                "byte, out = int(sys.argv[1]), sys.argv[2]\n"
                "try:\n"
                "    with api.alloc_poison(byte):\n"
                "        p = Polisher([])\n"
                "        for i, k in enumerate('ABA'):\n"
                "            S, _, _, _, _ = t.device_files(p, '%%s.%%s.sam' %% (out, k), 'strand', '%%s.%%d.bam' %% (out, i))\n"
                "            open('%%s.%%d.stream' %% (out, i), 'wb').write(S)\n"
                "        p.close()\n"
                "    assert api.alloc_poison_stats()[0] > 0\n"
                "except api.Np2Error as e:\n"
                "    print(e, file=sys.stderr)\n"
                "    sys.exit(3 if e.code == -2 else 1)\n" % (ROOT, os.path.join(ROOT, "tests")))


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_on_poisoned_recycled_blocks(tmp_path, byte):
    """a small input A, a larger B and A again on one context, every pool block filled with `byte` before it is handed out: the
    two A outputs are identical and equal to the model (the second runs in buffers sized and dirtied by B).  (A process of
    its own: the hook's counters are the process's, and tests/test_gpu_dirty_memory.py reads them.)"""
    refs, inputs = poison_inputs()
    out = str(tmp_path / "w")
    for k, v in inputs.items():
        write_sam(f"{out}.{k}.sam", refs, v)
    env = dict(os.environ, PYTHONPATH=ROOT, NP2_BGZF_TEST_BATCH="2", NP2_SAM_TEST_PIECE=str(1 << 16))
    r = subprocess.run([sys.executable, "-c", _POISON_CODE, str(byte), out], capture_output=True, env=env, timeout=300)
    if r.returncode == 3 or r.returncode < 0:
        device_error(r.stderr.decode(errors="replace")[-2000:], f"the BAM writer under poison {byte:#x}")
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    outs = []
    for i, k in enumerate("ABA"):
        S, bam, bai = (open(f"{out}.{i}.{e}", "rb").read() for e in ("stream", "bam", "bam.bai"))
        assert bm.check_files(refs, bm.sort_records(inputs[k]), bam, bai, (k, byte)) == S
        outs.append((S, bam, bai))
    assert outs[0] == outs[2]
