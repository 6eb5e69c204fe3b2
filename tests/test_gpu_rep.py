"""The repetitive k-mer list on the device (np2_rep_bytes, np2_rep_files, python -m nextpolish2_amd.repkmers) against the
numpy model of tests/rep_model.py: indices, counts and every stats field except the three times, exactly.  The streams are
seeded; their lengths are the count kernel's tile (8192 bytes) and its neighbours, their separators and N runs sit on and
around tile edges and lane-stretch edges (multiples of 32)."""
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import rep_model as rm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from test_rep_cpu import ASM, KNOWN, known_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
TILE = 8192
FIELDS = ("kmers", "distinct", "threshold", "listed", "listed_occurrences", "max_count")


@functools.lru_cache(maxsize=None)
def stream_of(n, seed=3):
    """n bytes: random bases with planted repeats (a 40-base motif, a homopolymer, a dinucleotide satellite), lower case and
    U mixed in, separators and N runs on and around every tile edge and some lane-stretch edges"""
    rng = np.random.default_rng(seed + n)
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    motif = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 40)]
    for at in rng.integers(0, max(1, n - 40), n // 300):
        s[at:at + 40] = motif[:len(s[at:at + 40])]
    for at in rng.integers(0, max(1, n - 200), n // 5000 + (1 if n > 400 else 0)):
        s[at:at + 100] = ord("A")
        s[at + 100:at + 200] = np.frombuffer(b"AC" * 50, np.uint8)[:len(s[at + 100:at + 200])]
    t = s == ord("T")
    s[t & (rng.random(n) < 0.02)] = ord("U")
    s[rng.random(n) < 0.1] |= 0x20
    edges = list(range(0, n + 1, TILE)) + rng.choice(np.arange(32, max(64, n), 32), min(40, max(1, n // 64)), replace=False).tolist()
    for i, e in enumerate(edges):
        at = e + (i % 3) - 1  # just before, on, just behind the edge
        run = 1 + i % 3
        fill = (ord("\n"), ord("N"), ord("n"), 0x8A)[i % 4]
        if 0 <= at < n:
            s[at:at + run] = fill
    return s.tobytes()


@functools.lru_cache(maxsize=None)
def table_of(n, k):
    return rm.table(stream_of(n), k)


def model(n, k, distinct=0.9998, min_count=None):
    return rm.listed(*table_of(n, k), distinct=distinct, min_count=min_count)


def same(got, exp):
    gi, gc, gst = got
    ei, ec, est = exp
    assert {f: gst[f] for f in FIELDS} == est
    assert gi.dtype == np.uint32 and gc.dtype == np.uint32 and np.array_equal(gi, ei) and np.array_equal(gc, ec)
    assert all(gst[f] >= 0.0 for f in ("count_ms", "select_ms", "emit_ms"))


# ---- 1. seeded streams at the tile's edges --------------------------------------------------------------------------------------
LENGTHS = ("0", "k-1", "k", "8191", "8192", "8193", "24577", "1000003")


def length_of(label, k):
    return {"k-1": k - 1, "k": k}[label] if label in ("k-1", "k") else int(label)


@pytest.mark.parametrize("k", [2, 3, 8, 15])
@pytest.mark.parametrize("label", LENGTHS)
def test_bytes_match_the_model(label, k):
    n = length_of(label, k)
    same(api.rep_bytes(stream_of(n), k=k), model(n, k))
    for m in (0, 1, 3, 50):
        same(api.rep_bytes(stream_of(n), k=k, min_count=m), model(n, k, min_count=m))


def test_stream_generator_covers_what_it_claims():
    s = stream_of(1000003)
    a = np.frombuffer(s, np.uint8)
    for edge in (TILE, 2 * TILE, 3 * TILE):
        assert rm._CODE[a[edge - 1:edge + 3]].max() == 4  # a non-base on or next to every tile edge
    assert (a == ord("u")).any() and (a == ord("U")).any() and (a == ord("n")).any() and (a >= 0x80).any() and (a == 10).any()
    assert model(1000003, 15)[2]["listed"] > 0 and model(1000003, 15)[2]["max_count"] > 100


def test_k16_on_the_committed_assembly():
    stream = np2io.seqfile_stream(ASM)
    row = [r for r in KNOWN if r[0] == 16][0]
    got = api.rep_bytes(stream, k=16, distinct=row[1])
    same(got, rm.rep(stream, 16, distinct=row[1]))
    assert {f: got[2][f] for f in FIELDS} == known_stats(row)


# ---- 2. counts above 65 535: the selection's second level and the hot address --------------------------------------------------
RUNS = b"\n".join([b"A" * 70001, b"C" * 70002, b"ACAC"])  # k = 2: AA 70 000, CC 70 001, AC 2, CA 1


@pytest.mark.parametrize("f,threshold", [(0.0, 1), (0.5, 2), (0.75, 70000), (1.0, 70001)])
def test_threshold_in_the_high_bin(f, threshold):
    got = api.rep_bytes(RUNS, k=2, distinct=f)
    same(got, rm.rep(RUNS, 2, distinct=f))
    assert got[2]["threshold"] == threshold and got[2]["max_count"] == 70001 and got[2]["distinct"] == 4
    if f == 0.75:
        assert got[0].tolist() == [5] and got[1].tolist() == [70001]


def test_homopolymer_counts_every_position(monkeypatch):
    stream = b"A" * 300000
    got = api.rep_bytes(stream, k=15, min_count=0)
    assert got[0].tolist() == [0] and got[1].tolist() == [299986] and got[2]["kmers"] == 299986 and got[2]["distinct"] == 1
    same(api.rep_bytes(stream, k=15), rm.rep(stream, 15))
    monkeypatch.setenv("NP2_REP_NO_COLLAPSE", "1")  # one add per k-mer: the same counters
    same(api.rep_bytes(stream, k=15, min_count=0), rm.rep(stream, 15, min_count=0))
    same(api.rep_bytes(stream_of(24577), k=8), model(24577, 8))


# ---- 3. pieces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [4096, 8192 + 16, 100003])
def test_pieces_give_the_one_piece_result(monkeypatch, piece):
    monkeypatch.setenv("NP2_REP_TEST_PIECE", str(piece))
    for k in (2, 15):
        same(api.rep_bytes(stream_of(1000003), k=k), model(1000003, k))
    same(api.rep_bytes(stream_of(1000003), k=15, min_count=1), model(1000003, 15, min_count=1))
    # a k-mer that spans two pieces is counted once, with the piece that holds its last byte
    same(api.rep_bytes(b"A" * (piece + 7), k=15, min_count=0), rm.rep(b"A" * (piece + 7), 15, min_count=0))


def test_two_calls_give_identical_arrays():
    a, b = api.rep_bytes(stream_of(1000003), k=15), api.rep_bytes(stream_of(1000003), k=15)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and {f: a[2][f] for f in FIELDS} == {f: b[2][f] for f in FIELDS}


# ---- 4. files ------------------------------------------------------------------------------------------------------------------
def test_files_write_the_models_text(tmp_path):
    stream = np2io.seqfile_stream(ASM)
    for row in KNOWN[:2]:
        out = tmp_path / f"rep_{row[1]}.txt"
        st = api.rep_files([ASM], str(out), k=row[0], distinct=row[1])
        mi, mc, mst = rm.rep(stream, row[0], distinct=row[1])
        assert out.read_text() == rm.text(mi, mc, row[0]) and {f: st[f] for f in FIELDS} == known_stats(row) == mst
    out = tmp_path / "both.txt"
    api.rep_files(ASM, str(out), both=True)
    mi, mc, _ = rm.rep(stream, 15)
    assert out.read_text() == rm.text(mi, mc, 15, both=True) and len(out.read_text().splitlines()) == 16


def test_a_contig_written_twice_doubles_every_count(tmp_path):
    contig = np2io.seqfile_stream(ASM)[:-1]
    twice = tmp_path / "twice.fa.gz"
    lines = b"\n".join(contig[i:i + 70] for i in range(0, len(contig), 70))
    twice.write_bytes(gzip.compress(b">a first\n" + lines + b"\n>b\n" + contig + b"\n", 1))
    out1, out2 = tmp_path / "once.txt", tmp_path / "twice.txt"
    st1 = api.rep_files([ASM], str(out1), min_count=0)
    st2 = api.rep_files([str(twice)], str(out2), min_count=0)
    assert st2["kmers"] == 2 * st1["kmers"] and st2["distinct"] == st1["distinct"] == st1["listed"] == st2["listed"]
    one = [ln.split("\t") for ln in out1.read_text().splitlines()]
    two = [ln.split("\t") for ln in out2.read_text().splitlines()]
    assert [x[0] for x in one] == [x[0] for x in two] and [2 * int(x[1]) for x in one] == [int(x[1]) for x in two]
    # two files in one call: three copies
    st3 = api.rep_files([ASM, str(twice)], str(out2), min_count=0)
    assert st3["kmers"] == 3 * st1["kmers"] and st3["max_count"] == 3 * st1["max_count"]


# ---- 5. the module -------------------------------------------------------------------------------------------------------------
def run_module(*args):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd.repkmers"] + list(args), capture_output=True, text=True, env=ENV,
                          cwd=ROOT, timeout=600)


def test_module_writes_the_list_and_the_stats(tmp_path):
    mi, mc, mst = rm.rep(np2io.seqfile_stream(ASM), 15)
    r = run_module(ASM)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == rm.text(mi, mc, 15)
    out, stats = tmp_path / "rep.txt", tmp_path / "rep.stats.tsv"
    r = run_module(ASM, "-k", "15", "--distinct", "0.9998", "--both", "--stats", str(stats), "-o", str(out))
    assert r.returncode == 0 and r.stdout == "", r.stderr[-3000:]
    assert out.read_text() == rm.text(mi, mc, 15, both=True)
    head, row = stats.read_text().splitlines()
    cells = dict(zip(head.split("\t"), row.split("\t")))
    assert cells["k"] == "15" and {f: int(cells[f]) for f in FIELDS} == mst and float(cells["count_ms"]) >= 0.0
    r = run_module(ASM, "--min_count", "1", "-k", "8", "-o", str(out))
    assert r.returncode == 0, r.stderr[-3000:]
    mi, mc, _ = rm.rep(np2io.seqfile_stream(ASM), 8, min_count=1)
    assert out.read_text() == rm.text(mi, mc, 8)


def test_module_reports_bad_k(tmp_path):
    for k in ("17", "1"):
        r = run_module(ASM, "-k", k, "-o", str(tmp_path / "no.txt"))
        assert r.returncode != 0 and "Error:" in r.stderr and f"k = {k}" in r.stderr
    r = run_module(str(tmp_path / "missing.fa"))
    assert r.returncode != 0 and "Error:" in r.stderr and "missing.fa" in r.stderr
