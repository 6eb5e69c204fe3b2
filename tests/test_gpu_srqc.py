"""The short-read quality filter on the device (np2_srqc_*, the *_qc counting entry points, python -m nextpolish2_amd.srqc,
the command lines' --sr_qc) against the plain-Python model of tests/srqc_model.py.  The reads are the model's seeded
generator (tests/test_srqc_cpu.py asserts what it exercises) plus its hand-written edge reads."""
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import srqc_model as sm
from nextpolish2_amd import Polisher, api
from nextpolish2_amd import io as np2io
from test_kcount_cpu import BUNDLE, FIXTURE, stream_hashes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "tests", "golden", "ref_test_asm.fa.gz")
BAM = os.path.join(BUNDLE, "hifi.map.sort.bam")
ENV = dict(os.environ, PYTHONPATH=ROOT)
KS = [21, 31]
E_UNSUPPORTED = -4


@functools.lru_cache(maxsize=None)
def gen_reads():
    return tuple(sm.generate())


@functools.lru_cache(maxsize=None)
def gen_clean_stream():
    return sm.clean_stream(gen_reads(), sm.opts())


def qc_of(o):
    return np2io.SrQc(**o)


def write_two_files(tmp_path, reads, tag="g"):
    """the reads as two FASTQ files, the second gzip"""
    half = len(reads) // 2
    a, b = tmp_path / f"{tag}a.fq", tmp_path / f"{tag}b.fq.gz"
    a.write_bytes(sm.fastq(reads[:half], b"a"))
    b.write_bytes(gzip.compress(sm.fastq(reads[half:], b"b"), 1))
    return [str(a), str(b)]


def same_yaks(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.k == e.k and np.array_equal(g.bucket_off, e.bucket_off) and np.array_equal(g.words, e.words), g.k


# ---- 1. np2_srqc_bytes against the model ----------------------------------------------------------------------------------------
VARIANTS = ([("recipe", sm.opts())] + [("only_" + "_".join(d), sm.opts(sm.NEUTRAL, **d)) for d in sm.SINGLES] +
            [(f"window{w}", sm.opts(cut_window=w)) for w in (1, 64, 1000)] + [(f"n{v}", sm.opts(n_base_limit=v)) for v in sm.N_LIMITS[1:]])


@pytest.mark.parametrize("name,o", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_stream_equals_the_model(name, o):
    reads = list(gen_reads()) + sm.edge_reads()
    seq, qual = sm.streams(reads)
    res, masked, totals = sm.run(reads, o)
    got_masked, got_reads, got_totals = np2io.srqc_bytes(seq, qual, qc_of(o))
    got = list(zip(got_reads["begin"].tolist(), got_reads["end"].tolist(), got_reads["cls"].tolist()))
    bad = [(i, g, e, len(reads[i][0])) for i, (g, e) in enumerate(zip(got, res)) if g != e]
    assert not bad, (len(bad), bad[:5])
    assert got_masked == masked
    assert got_totals == totals
    assert {k: v for k, v in np2io.srqc_last_stats().items() if k != "kernel_ms"} == totals


def test_stream_argument_errors():
    seq, qual = sm.streams(sm.edge_reads()[:6])
    L = np2io._bind()
    o = np2io.SrQc().c()
    import ctypes as C
    s, q = np.frombuffer(seq, np.uint8), np.frombuffer(qual, np.uint8)
    rc = L.np2_srqc_bytes(0, s.ctypes.data, q.ctypes.data, len(s), C.byref(o), None, None, 5, None)  # 6 separators
    assert rc == -1 and "n_reads" in L.np2_io_last_error().decode()
    o.cut_window = 1001
    rc = L.np2_srqc_bytes(0, s.ctypes.data, q.ctypes.data, len(s), C.byref(o), None, None, 6, None)
    assert rc == -1 and "cut_window" in L.np2_io_last_error().decode()
    assert np2io.srqc_bytes(b"", b"")[2] == dict.fromkeys(sm.STAT_NAMES, 0)


# ---- 2. word ownership ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [sm.opts(sm.NEUTRAL, qualified_q=20, unqualified_percent=40),
                               sm.opts(sm.NEUTRAL, qualified_q=20, unqualified_percent=40, trim_front=1, trim_tail=1)], ids=["whole", "trimmed"])
def test_neighbouring_reads_share_words(o):
    """reads of 1 .. 9 bases back to back in every rotation and at every offset of a word, pass and fail alternating: every
    separator falls on each of the four byte positions, and every word at a boundary is shared by a read that is rewritten
    and one that is not"""
    reads, k = [], 0
    for lead in range(4):
        if lead:
            reads.append((b"ACGT"[:lead - 1], b"I" * (lead - 1)))  # shifts what follows by `lead` bytes
        for rot in range(9):
            for j in range(9):
                n = 1 + (rot + j) % 9
                reads.append((b"ACGTACGTA"[:n], (b"I" if k % 2 == 0 else b"#") * n))
                k += 1
    seq, qual = sm.streams(reads)
    seps = np.flatnonzero(np.frombuffer(seq, np.uint8) == 10)
    assert {int(x) % 4 for x in seps} == {0, 1, 2, 3}
    res, masked, totals = sm.run(reads, o)
    assert totals["pass"] > 100 and totals["low_quality"] > 100
    got_masked, got_reads, got_totals = np2io.srqc_bytes(seq, qual, qc_of(o))
    assert got_masked == masked and got_totals == totals
    assert [tuple(r) for r in got_reads.tolist()] == res


# ---- 3. counting through the filter ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen_files(tmp_path_factory):
    return write_two_files(tmp_path_factory.mktemp("srqc"), list(gen_reads()))


@functools.lru_cache(maxsize=None)
def clean_yaks(min_count):
    return tuple(np2io.count_kmers(gen_clean_stream(), KS, min_count=min_count))


@pytest.mark.parametrize("min_count", [1, 2])
def test_counting_through_the_filter_equals_counting_the_clean_reads(gen_files, tmp_path, min_count):
    exp = clean_yaks(min_count)
    assert all(len(y.words) > 1000 for y in exp)
    same_yaks(np2io.count_kmers(gen_files, KS, min_count=min_count, qc=np2io.SrQc.recipe()), exp)
    assert {k: v for k, v in np2io.srqc_last_stats().items() if k != "kernel_ms"} == sm.run(gen_reads(), sm.opts())[2]
    outs = [str(tmp_path / f"k{k}.yak") for k in KS]
    np2io.count_kmers_to_files(gen_files, KS, outs, min_count=min_count, qc=np2io.SrQc.recipe())
    for out, y in zip(outs, exp):
        ref = str(tmp_path / f"ref{y.k}.yak")
        np2io.write_yak(ref, y)
        assert open(out, "rb").read() == open(ref, "rb").read()
    # unfiltered, the same files count differently: the option is not a no-op here
    assert len(np2io.count_kmers(gen_files, KS, min_count=min_count)[0].words) != len(exp[0].words)


@pytest.mark.parametrize("min_count", [1, 2])
def test_resident_tables_through_the_filter_answer_like_uploaded_ones(gen_files, min_count):
    pol = np2io.polisher_from_reads(gen_files, KS, min_count=min_count, qc=np2io.SrQc.recipe())
    ref = Polisher(list(clean_yaks(min_count)))
    rng = np.random.default_rng(1)
    raw = sm.streams(gen_reads())[0]
    for i, k in enumerate(KS):
        present = np.unique(stream_hashes(raw, k))  # of the unfiltered reads: some survive the filter, some do not
        absent = rng.integers(0, 1 << (2 * k), size=2000, dtype=np.uint64)
        hs = np.concatenate([present, absent])
        for mk in (1, 2, 5):
            got, exp = pol.lookup_hashes(i, hs, mk), ref.lookup_hashes(i, hs, mk)
            assert np.array_equal(got, exp), (k, mk)
        assert 0 < int((pol.lookup_hashes(i, present, 1) > 0).sum()) < len(present)


# ---- 4. piece boundaries --------------------------------------------------------------------------------------------------------
def _count_in_child(tmp_path, files, piece):
    out = tmp_path / f"p{piece}.npz"
    code = ("import numpy as np\nfrom nextpolish2_amd import io\n"
            f"ys = io.count_kmers({files!r}, {KS!r}, qc=io.SrQc.recipe())\n"
            "st = io.srqc_last_stats()\n"
            f"np.savez({str(out)!r}, **{{f'w{{i}}': y.words for i, y in enumerate(ys)}}, **{{f'o{{i}}': y.bucket_off for i, y in enumerate(ys)}}, "
            f"stats=np.array([st[k] for k in {sm.STAT_NAMES!r}], np.uint64))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, env=dict(ENV, NP2_KCOUNT_TEST_PIECE=str(piece)), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return np.load(out)


@pytest.mark.parametrize("piece", [5200, 8192, 65536])
def test_pieces_end_at_reads_and_change_nothing(gen_files, tmp_path, piece):
    got = _count_in_child(tmp_path, gen_files, piece)
    exp = clean_yaks(1)  # (test 3 pins the one-piece run to the same tables)
    for i, y in enumerate(exp):
        assert np.array_equal(got[f"w{i}"], y.words) and np.array_equal(got[f"o{i}"], y.bucket_off), (piece, y.k)
    totals = sm.run(gen_reads(), sm.opts())[2]
    assert got["stats"].tolist() == [totals[k] for k in sm.STAT_NAMES]


def test_a_read_longer_than_a_piece_is_refused_not_cut(gen_files, tmp_path):
    seq, qual = sm.streams(sm.edge_reads()[:20])
    code = ("from nextpolish2_amd import io, api\n"
            "try:\n"
            f"    io.count_kmers({gen_files!r}, {KS!r}, qc=io.SrQc.recipe())\n"
            "except api.Np2Error as e:\n"
            "    print(e.code, e)\n"
            f"print('next', io.srqc_bytes({seq!r}, {qual!r})[2]['reads'])\n")  # the process goes on to the next call
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(ENV, NP2_KCOUNT_TEST_PIECE="4096"), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    first, second = r.stdout.strip().split("\n")
    assert first.startswith(f"{E_UNSUPPORTED} ") and "5000 bases" in first and "4096" in first
    assert second == "next 20"


# ---- 5. qc=None is today's path -------------------------------------------------------------------------------------------------
def test_without_the_option_the_committed_dumps_come_out(tmp_path):
    import test_gpu_kcount as tk
    tk.test_golden_dumps_from_the_fixture(tmp_path)
    outs = [str(tmp_path / "n21.yak"), str(tmp_path / "n31.yak")]
    np2io.count_kmers_to_files(FIXTURE, KS, outs, min_count=2, qc=None)
    assert open(outs[0], "rb").read() == tk.committed(21) and open(outs[1], "rb").read() == tk.committed(31)
    same_yaks(np2io.count_kmers(FIXTURE, KS, min_count=2, qc=None), [np2io.load_yak(os.path.join(BUNDLE, f"k{k}.yak")) for k in KS])
    same_yaks(np2io.count_kmers(FIXTURE, KS, min_count=2), [np2io.load_yak(os.path.join(BUNDLE, f"k{k}.yak")) for k in KS])
    with pytest.raises(api.Np2Error) as e:  # the fixture is sequence lines, not FASTQ
        np2io.count_kmers(FIXTURE, KS, qc=np2io.SrQc.recipe())
    assert e.value.code == -1 and "FASTQ" in str(e.value) and any(f in str(e.value) for f in FIXTURE)


# ---- 6. np2_srqc_files and the module -------------------------------------------------------------------------------------------
def test_module_report_and_cleaned_files(gen_files, tmp_path):
    reads = list(gen_reads())
    half = len(reads) // 2
    parts = [(reads[:half], b"a"), (reads[half:], b"b")]
    rep, prefix = tmp_path / "qc.tsv", str(tmp_path / "clean")
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.srqc"] + gen_files + ["--report", str(rep), "--out_fq", prefix],
                       capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [x.split("\t") for x in rep.read_text().splitlines()]
    assert rows[0] == ["file"] + list(sm.STAT_NAMES) and [x[0] for x in rows[1:]] == gen_files + ["total"]
    per_file = [sm.run(p, sm.opts())[2] for p, _ in parts]
    for row, t in zip(rows[1:3], per_file):
        assert [int(x) for x in row[1:]] == [t[k] for k in sm.STAT_NAMES]
    assert [int(x) for x in rows[3][1:]] == [per_file[0][k] + per_file[1][k] for k in sm.STAT_NAMES]
    cleaned = [f"{prefix}.{i}.fq" for i in range(2)]
    for path, (p, tag) in zip(cleaned, parts):
        exp = sm.clean_fastq([(b"@%s%d" % (tag, i), s, q) for i, (s, q) in enumerate(p)], sm.opts())
        assert open(path, "rb").read() == exp
    # the cleaned files pass whole through the filters that are left without the trims and cuts
    again = [str(tmp_path / "again0.fq"), str(tmp_path / "again1.fq")]
    st = np2io.srqc_files(cleaned, np2io.SrQc.parse("front=0,tail=0,cut5=0,cut3=0"), again)
    assert st[2]["pass"] == st[2]["reads"] == per_file[0]["pass"] + per_file[1]["pass"] and st[2]["bases_out"] == st[2]["bases_in"]
    for x, y in zip(cleaned, again):
        assert open(x, "rb").read() == open(y, "rb").read()


# ---- 7. the command line --------------------------------------------------------------------------------------------------------
def bundle_reads_with_bad_ends(seed=5):
    """the bundle's short-read sequences with seeded synthetic qualities: good, with bad stretches at the ends of most reads
    and a few reads bad throughout"""
    rng = np.random.default_rng(seed)
    reads = []
    for path in FIXTURE:
        for s in gzip.open(path, "rb").read().split(b"\n")[:-1]:
            n = len(s)
            p = np.full(n, 37, np.uint8)
            e1, e2 = rng.integers(0, 25, size=2)
            p[:e1] = 4
            p[n - e2:] = 4
            if rng.random() < 0.02:
                p[:] = 6
            reads.append((s, (p + 33).tobytes()))
    return reads


def _cli(args):
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", "-t", "5", "-L", "1000", BAM, ASM, "-k", "2"] + args,
                       capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout, r.stderr.decode()


def test_cli_polishes_from_filtered_reads(tmp_path):
    reads = bundle_reads_with_bad_ends()
    files = write_two_files(tmp_path, reads, "c")
    half = len(reads) // 2
    clean = tmp_path / "model_cleaned.fq"
    clean.write_bytes(sm.clean_fastq([(b"@a%d" % i, s, q) for i, (s, q) in enumerate(reads[:half])] +
                                     [(b"@b%d" % i, s, q) for i, (s, q) in enumerate(reads[half:])], sm.opts()))
    totals = sm.run(reads, sm.opts())[2]
    assert totals["pass"] > 50000 and totals["too_short"] > 500 and totals["bases_out"] < 0.9 * totals["bases_in"]
    sr = [x for f in files for x in ("--sr", f)]
    with_qc, err = _cli(sr + ["--sr_qc"])
    from_clean, _ = _cli(["--sr", str(clean)])
    assert with_qc == from_clean and with_qc.startswith(b">")
    line = [x for x in err.splitlines() if x.startswith("[INFO] sr_qc:")]
    assert line == ["[INFO] sr_qc: " + ", ".join(f"{k} {totals[k]}" for k in sm.STAT_NAMES)]
    # the option reaches the polish: the tables the polish is counted from differ from the unfiltered ones (asserted on the
    # tables, not on the FASTA: the polished bundle need not change when 2 % of the reliable k-mers go; under the model
    # 116 185 of the 118 978 words of k = 21 at min_count 2 are left)
    a, b = np2io.count_kmers(files, [21], min_count=2, qc=np2io.SrQc.recipe())[0], np2io.count_kmers(files, [21], min_count=2)[0]
    assert (len(a.words), len(b.words)) == (116185, 118978)


# ---- 8. determinism -------------------------------------------------------------------------------------------------------------
def test_two_filtered_runs_give_identical_bytes(gen_files, tmp_path):
    outs = [[str(tmp_path / f"r{r}k{k}.yak") for k in KS] for r in range(2)]
    for o in outs:
        np2io.count_kmers_to_files(gen_files, KS, o, min_count=1, qc=np2io.SrQc.recipe())
    for a, b in zip(*outs):
        assert open(a, "rb").read() == open(b, "rb").read()
