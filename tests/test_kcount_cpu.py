"""The k-mer counter's host side, without a GPU: the sequence reader (np2_seqfile_stream), the per-lane core of the count
kernel run as a one-lane host program (csrc/np2_kcount_core.hpp through tests/tools/kcount_core_test.cpp), and the
argument checks of the entry points, which come before any device call.

Fixture: tests/golden/ref_bundle/sr.seq.{0,1,2}.gz hold ONLY THE SEQUENCE LINES of the reference's two test read files
(test/sr.R1.fastq.gz then test/sr.R2.fastq.gz, one read per line, in file order), cut into three gzip files so that each
stays below the size limit for a committed file.  The parser tests use small hand-written FASTQ / FASTA text.

The independent expectation is the numpy counter below (the recipe that produced the committed k21.yak / k31.yak)."""
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from nextpolish2_amd import api
from nextpolish2_amd import io as np2io

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUNDLE = os.path.join(HERE, "golden", "ref_bundle")
FIXTURE = [os.path.join(BUNDLE, f"sr.seq.{i}.gz") for i in range(3)]
E_ARG, E_NOMEM, E_UNSUPPORTED = -1, -3, -4


# ---- the numpy counter --------------------------------------------------------------------------------------------
def hash64(key, mask):
    key = (~key + (key << np.uint64(21))) & mask
    key = key ^ (key >> np.uint64(24))
    key = ((key + (key << np.uint64(3))) + (key << np.uint64(8))) & mask
    key = key ^ (key >> np.uint64(14))
    key = ((key + (key << np.uint64(2))) + (key << np.uint64(4))) & mask
    key = key ^ (key >> np.uint64(28))
    key = (key + (key << np.uint64(31))) & mask
    return key


def stream_hashes(stream, k):
    """Hashes of the canonical k-mers of a separator stream (SEQ_NUM: ACGTUacgtu are bases, every other byte resets)."""
    lut = np.full(256, 4, np.uint8)
    for ch, v in zip(b"ACGTU", (0, 1, 2, 3, 3)):
        lut[ch] = v
        lut[ch | 0x20] = v
    c = lut[np.frombuffer(stream, dtype=np.uint8)]
    n = c.shape[0] - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    bad = np.concatenate([[0], np.cumsum(c == 4)])
    ok = (bad[k:] - bad[:-k]) == 0
    c64 = (c & 3).astype(np.uint64)
    fw = np.zeros(n, np.uint64)
    rv = np.zeros(n, np.uint64)
    for j in range(k):
        fw |= c64[j:j + n] << np.uint64(2 * (k - 1 - j))
        rv |= (np.uint64(3) ^ c64[j:j + n]) << np.uint64(2 * j)
    return hash64(np.minimum(fw, rv)[ok], np.uint64((1 << (2 * k)) - 1))


def numpy_count(stream, k, min_count=1):
    """(words, bucket_off) of the table: bucket-major, ascending inside a bucket, counts capped at 1023."""
    h, cnt = np.unique(stream_hashes(stream, k), return_counts=True)
    keep = cnt >= max(1, min_count)
    h, cnt = h[keep], np.minimum(cnt[keep], 1023).astype(np.uint64)
    order = np.argsort(h & np.uint64(1023), kind="stable")  # (h ascending -> h >> 10 ascending inside a bucket)
    h, cnt = h[order], cnt[order]
    off = np.zeros(1025, np.uint64)
    off[1:] = np.cumsum(np.bincount((h & np.uint64(1023)).astype(np.int64), minlength=1024))
    return ((h >> np.uint64(10)) << np.uint64(10)) | cnt, off


def dump_bytes(k, words, off):
    out = [b"YAK\x02" + struct.pack("<III", k, 10, 10)]
    for b in range(1024):
        s, e = int(off[b]), int(off[b + 1])
        out.append(struct.pack("<II", 0, e - s) + words[s:e].tobytes())
    return b"".join(out)


def fixture_stream():
    return b"".join(gzip.open(p, "rb").read() for p in FIXTURE)


# ---- 1. the reader ------------------------------------------------------------------------------------------------
def test_reader_fixture_equals_gzip_parse():
    for p in FIXTURE:
        with gzip.open(p, "rb") as f:
            lines = [ln.rstrip(b"\n") for ln in f]
        assert np2io.seqfile_stream(p) == b"".join(ln + b"\n" for ln in lines)
    s = fixture_stream()
    assert s.count(b"\n") == 66196 and len(s) == 66196 * 151 and set(s) == set(b"ACGT\n")


def test_reader_hand_written_inputs(tmp_path):
    def stream(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        return np2io.seqfile_stream(str(p))

    # quality lines that begin with '@' and with '>' (the 4-line rule), CRLF, an empty read, no final newline
    fq = b"@r1 x\nACGT\n+\n@III\n@r2\nGGNcc\n+r2\n>>>>>\n@r3\n\n+\n\n@r4\nTTTT\n+\nIIII"
    assert stream("a.fq", fq) == b"ACGT\nGGNcc\n\nTTTT\n"
    assert stream("crlf.fq", fq.replace(b"\n", b"\r\n")) == b"ACGT\nGGNcc\n\nTTTT\n"
    assert stream("cut.fq", b"@r1\nACGT\n+\nIIII\n@r2\nGG") == b"ACGT\nGG\n"  # the file ends inside a sequence line
    assert stream("blank.fq", b"\n@r1\nACGT\n+\nIIII\n\n\n@r2\nGG\n+\nII\n\n") == b"ACGT\nGG\n"
    # multi-line FASTA joined, a record without sequence, no final newline
    assert stream("a.fa", b">c1 d\nACG\nTTA\n>c2\n>c3\r\nGG\r\nAA") == b"ACGTTA\n\nGGAA\n"
    assert stream("lines.txt", b"ACGT\nGG\n\nTT") == b"ACGT\nGG\n\nTT\n"
    assert stream("empty.fq", b"") == b""
    # two gzip members in one file
    two = gzip.compress(b"@r1\nACGT\n+\nIIII\n") + gzip.compress(b"@r2\nGGCC\n+\nIIII\n")
    assert stream("two.fq.gz", two) == b"ACGT\nGGCC\n"
    # a truncated gzip
    whole = gzip.compress(b"".join(b"@r%d\nACGTACGTAGCTAGCTAGCATCGATCAGCTACGACTAGC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" % i for i in range(2000)))
    with pytest.raises(api.Np2Error) as e:
        stream("cut.fq.gz", whole[: len(whole) // 2])
    assert e.value.code == E_ARG and "cut.fq.gz" in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        np2io.seqfile_stream(str(tmp_path / "missing.fq"))
    assert e.value.code == E_ARG and "cannot open" in str(e.value)


# ---- 2. the per-lane core ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kcount") / "kcount_core_test")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "tools", "kcount_core_test.cpp"), "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("k", [21, 31])
def test_core_reproduces_the_committed_dumps(core_exe, tmp_path, k):
    out = str(tmp_path / f"k{k}.yak")
    r = subprocess.run([core_exe, str(k), "2", out] + FIXTURE, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = open(out, "rb").read()
    assert got == open(os.path.join(BUNDLE, f"k{k}.yak"), "rb").read()


def test_fixture_facts():
    """The figures the reads are known by (numpy counter): k-mers, distinct, singletons, words >= 2, largest count."""
    s = fixture_stream()
    for k, facts in ((21, (8605480, 456279, 337301, 118978, 5611)), (31, (7943520, 593788, 466635, 127153, 1856))):
        h = stream_hashes(s, k)
        _, cnt = np.unique(h, return_counts=True)
        assert (len(h), len(cnt), int((cnt == 1).sum()), int((cnt >= 2).sum()), int(cnt.max())) == facts


def awkward_stream(seed=5):
    """Lower case, U, N, bytes >= 0x80, reads shorter than k, a homopolymer past saturation, palindromes (fw == rv)."""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(300):
        n = int(rng.integers(1, 120))
        r = bytearray(rng.choice(np.frombuffer(b"ACGTacgtUuN", dtype=np.uint8), size=n, p=[.2, .2, .2, .2, .04, .04, .04, .04, .01, .01, .02]).tobytes())
        reads.append(bytes(r))
    reads += [b"A" * 1500, b"ACGT" * 300, b"AATT", b"ACGCGT" * 5, b"ACGT\xc1CGTACGT\x80\xffACGTTGCA", b"acgu" * 20, b"", b"G"]
    return b"\n".join(reads) + b"\n"


@pytest.mark.parametrize("k", [2, 15, 16, 31])
@pytest.mark.parametrize("min_count", [1, 3])
def test_core_against_the_numpy_counter(core_exe, tmp_path, k, min_count):
    s = awkward_stream()
    src = tmp_path / "s.txt"
    src.write_bytes(s)
    out = str(tmp_path / "o.yak")
    r = subprocess.run([core_exe, str(k), str(min_count), out, str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    words, off = numpy_count(s, k, min_count)
    assert len(words) > 0
    if k % 2 == 0 and min_count == 1:  # an even k has k-mers equal to their own reverse complement
        assert b"AATT" in s
    assert open(out, "rb").read() == dump_bytes(k, words, off)


def test_core_high_bytes_reset_the_run(core_exe, tmp_path):
    """A byte >= 0x80 is a non-base: it must not be read as the letter its low seven bits spell (0xC1 & 0x7F == 'A')."""
    out = str(tmp_path / "o.yak")
    for data in (b"ACGT\xc1CGT\n", b"ACGTNCGT\n"):
        src = tmp_path / "s.txt"
        src.write_bytes(data)
        assert subprocess.run([core_exe, "4", "1", out, str(src)], timeout=60).returncode == 0
        words, off = numpy_count(b"ACGT\nCGT\n", 4)
        assert open(out, "rb").read() == dump_bytes(4, words, off)


# ---- 3. arguments are checked before any device is touched ----------------------------------------------------------
def test_k_32_is_unsupported_before_any_device_call(tmp_path):
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    calls = [lambda k: np2io.count_kmers([str(fq)], [k]), lambda k: np2io.count_kmers(b"ACGT\n", [k]),
             lambda k: np2io.count_kmers_to_files([str(fq)], [k], [str(tmp_path / "o.yak")]),
             lambda k: np2io.polisher_from_reads([str(fq)], [k])]
    for call in calls:
        for k in (32, 1, 0):
            with pytest.raises(api.Np2Error) as e:
                call(k)
            assert e.value.code == E_UNSUPPORTED and "only k < 32" in str(e.value), str(e.value)
    for call in calls[:1] + calls[2:]:
        with pytest.raises(api.Np2Error) as e:
            np2io.count_kmers([str(tmp_path / "missing.fq")], [21])
        assert e.value.code == E_ARG and "cannot open" in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        np2io.count_kmers([str(fq)], [21], min_count=2000)
    assert e.value.code == E_ARG


def test_cli_without_sr_and_without_yak_is_an_argparse_error(tmp_path):
    bam = os.path.join(BUNDLE, "hifi.map.sort.bam")
    fa = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", bam, fa], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "the following arguments are required: short.read.yak" in r.stderr and r.stdout == ""
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", bam, fa, os.path.join(BUNDLE, "k21.yak"), "--sr", FIXTURE[0]],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "not both" in r.stderr
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", bam, fa, "--sr", FIXTURE[0], "--sr_k", "21,32"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--sr_k" in r.stderr
