"""The k-mer QV scan on the device (np2_qv_strings, np2_qv_device, python -m nextpolish2_amd.qv, the command line's --qv)
against the numpy brute force of tests/test_qv_cpu.py, the known answer on the committed fixtures, and
Polisher.lookup_hashes (the polish kernels' own lookup) as an independent device path.

Every case is one bounded subprocess or a handful of in-process calls."""
import ctypes as C
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from nextpolish2_amd import Opts, Polisher, api, qv
from nextpolish2_amd import io as np2io
from nextpolish2_amd._types import Yak
from test_kcount_cpu import FIXTURE, numpy_count, stream_hashes
from test_qv_cpu import (ASM_IN, ASM_OUT, BAM, BUNDLE, FASTA, KNOWN, aggregate, fasta_records, kmer_hashes_at, numpy_qv,
                         read_dump)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
DUMPS = [os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")]
TILE, HALO = 8192, 32  # csrc/np2_qv_core.hpp, np2_kcount_core.hpp
E_ARG = -1


def yak_table(y):
    """(sorted hashes, counts) of a Yak without repeated keys"""
    b = np.repeat(np.arange(1024, dtype=np.uint64), np.diff(y.bucket_off.astype(np.int64)))
    h = ((y.words >> np.uint64(10)) << np.uint64(10)) | b
    order = np.argsort(h)
    return h[order], (y.words & np.uint64(1023)).astype(np.uint32)[order]


def yak_of(stream, k, min_count=1):
    return Yak(k, *numpy_count(stream, k, min_count))


def same_as_numpy(pol, t, k, table, seqs, min_count):
    r = pol.qv_strings(t, seqs, min_count, hist=True, bits=True)
    e_hist = np.zeros(1024, np.uint64)
    assert r.stats.shape == (len(seqs), 2) and len(r.bits) == len(seqs)
    for i, s in enumerate(seqs):
        nk, na, h, b = numpy_qv(s, k, table, min_count)
        assert (int(r.stats[i, 0]), int(r.stats[i, 1])) == (nk, na), (k, min_count, i, len(s))
        assert np.array_equal(r.bits[i], b), (k, min_count, i, len(s))
        e_hist += h
    assert np.array_equal(r.hist, e_hist), (k, min_count)
    # the outputs nobody asked for change nothing
    r2 = pol.qv_strings(t, seqs, min_count)
    assert np.array_equal(r2.stats, r.stats) and r2.hist is None and r2.bits is None
    return r


def random_bases(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()


def noisy(rng, s, rate=0.01):
    a = np.frombuffer(s, dtype=np.uint8).copy()
    m = rng.random(len(a)) < rate
    a[m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(m.sum()))
    return a.tobytes()


# ---- 1. the known answer ---------------------------------------------------------------------------------------------------
def test_known_answer_through_qv_strings():
    pol = Polisher([np2io.load_yak(p) for p in DUMPS])
    seqs = [fasta_records(FASTA[s])[0][1] for s in ("in", "out")]
    for t, k in enumerate((21, 31)):
        _, th, tc = read_dump(DUMPS[t])
        for min_count in (1, 2):
            r = same_as_numpy(pol, t, k, (th, tc), seqs, min_count)
            for i, side in enumerate(("in", "out")):
                length, n_kmers, n_absent, text = KNOWN[(k, side)]
                assert len(seqs[i]) == length and (int(r.stats[i, 0]), int(r.stats[i, 1])) == (n_kmers, n_absent)
                assert qv.qv_text(*r.stats[i], k) == text
            assert r.kernel_ms > 0
    pol.close()


def parse_tsv(path):
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


@pytest.mark.parametrize("side", ["in", "out"])
def test_known_answer_through_the_qv_module(tmp_path, side):
    tsv, bed, hist = str(tmp_path / "q.tsv"), str(tmp_path / "q.bed"), str(tmp_path / "q.hist")
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.qv", FASTA[side]] + DUMPS + ["-o", tsv, "--bed", bed, "--hist", hist],
                       capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    head, rows = parse_tsv(tsv)
    (name, seq), = fasta_records(FASTA[side])
    assert head == list(qv.TSV_HEADER)
    exp = [[c, str(k)] + [str(x) for x in KNOWN[(k, side)]] for c in (name, "total") for k in (21, 31)]
    assert rows == exp
    hist_rows = [ln.split("\t") for ln in open(hist).read().splitlines()[1:]]
    for t, k in enumerate((21, 31)):
        _, th, tc = read_dump(DUMPS[t])
        _, _, e_hist, e_bits = numpy_qv(seq, k, (th, tc), 1)
        assert open(f"{bed}.k{k}").read() == "".join(f"{name}\t{a}\t{b}\n" for a, b in qv.bed_intervals(e_bits, len(seq), k))
        assert [(int(c), int(n)) for kk, c, n in hist_rows if int(kk) == k] == [(c, int(n)) for c, n in enumerate(e_hist) if n]


def test_qv_module_counts_its_tables_from_reads(tmp_path):
    """--sr: tables counted on the device at the committed dumps' threshold give the same integers"""
    cmd = [sys.executable, "-m", "nextpolish2_amd.qv", ASM_IN, "--sr_min_count", "2", "--qv_min_count", "2"]
    for p in FIXTURE:
        cmd += ["--sr", p]
    r = subprocess.run(cmd, capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    rows = [ln.split("\t") for ln in r.stdout.decode().splitlines()[1:]]
    assert [row[1:] for row in rows[:2]] == [[str(k)] + [str(x) for x in KNOWN[(k, "in")]] for k in (21, 31)]


# ---- 2. the command line on the bundle --------------------------------------------------------------------------------------
def test_cli_qv_on_the_reference_test_bundle(tmp_path):
    tsv, prefix = str(tmp_path / "t.tsv"), str(tmp_path / "p")
    cmd = [sys.executable, "-m", "nextpolish2_amd.cli", "-t", "5", "-L", "1000", BAM, ASM_IN] + DUMPS
    r = subprocess.run(cmd + ["--qv", tsv, "--qv_bed", prefix], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == gzip.open(ASM_OUT, "rb").read()  # byte for byte the FASTA written without --qv
    head, rows = parse_tsv(tsv)
    (name, seq_in), = fasta_records(ASM_IN)
    (_, seq_out), = fasta_records(ASM_OUT)
    assert head == list(qv.CLI_HEADER)
    exp = [[c, str(k)] + [str(x) for x in KNOWN[(k, "in")] + KNOWN[(k, "out")]] for c in (name, "total") for k in (21, 31)]
    assert rows == exp
    for t, k in enumerate((21, 31)):
        _, th, tc = read_dump(DUMPS[t])
        for side, seq in (("in", seq_in), ("out", seq_out)):
            bits = numpy_qv(seq, k, (th, tc), 1)[3]
            assert open(f"{prefix}.k{k}.{side}.bed").read() == "".join(f"{name}\t{a}\t{b}\n" for a, b in qv.bed_intervals(bits, len(seq), k))
    assert open(f"{prefix}.k21.out.bed").read() == "" and open(f"{prefix}.k21.in.bed").read() != ""
    # a pass-through contig counts: out equals in (the default -L writes this contig back unpolished)
    tsv2 = str(tmp_path / "u.tsv")
    r = subprocess.run(cmd[:3] + cmd[7:] + ["--qv", tsv2], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    _, rows = parse_tsv(tsv2)
    assert rows == [[c, str(k)] + [str(x) for x in KNOWN[(k, "in")] * 2] for c in (name, "total") for k in (21, 31)]


# ---- 3. an independent device path, at size ----------------------------------------------------------------------------------
def test_12mb_assembly_equals_lookup_hashes():
    from nextpolish2_amd.synth import Synth
    s = Synth(12_000_000, depth=1, seed=5, diploid=True)
    asm = s.pileup.ref.tobytes()
    cuts = [0] + sorted(int(x) for x in np.random.default_rng(5).integers(1, len(asm), size=5)) + [len(asm)]
    contigs = [asm[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    ks = (21, 31)
    pol = Polisher([s.yak(k) for k in ks])
    for t, k in enumerate(ks):
        per = [kmer_hashes_at(c, k) for c in contigs]
        for min_count in (0, 1, 2, 5, 1023):
            r = pol.qv_strings(t, contigs, min_count, hist=True)
            e_hist = np.zeros(1024, np.uint64)
            for i, (valid, hashes) in enumerate(per):
                counts = np.zeros(len(valid), np.uint32)
                counts[valid] = pol.lookup_hashes(t, hashes[valid], min_count)
                nk, na, h, _ = aggregate(valid, counts)
                assert (int(r.stats[i, 0]), int(r.stats[i, 1])) == (nk, na), (k, min_count, i)
                e_hist += h
            assert np.array_equal(r.hist, e_hist), (k, min_count)
            if min_count <= 2:
                assert 0 < r.n_absent < r.n_kmers  # (assembly errors are absent, the rest is not)
    pol.close()


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------
def edge_sequences(rng, base, k):
    """sequences cut from `base` (whose k-mers the table holds), a base in a hundred changed (absent k-mers)"""
    def cut(n):
        a = int(rng.integers(0, len(base) - n + 1))
        return noisy(rng, base[a:a + n])
    seqs = [b"", cut(k - 1), cut(k), cut(k + 1), b"N" * 100, b"N" * (TILE + 5), cut(500).lower(),
            cut(500).replace(b"T", b"U"), cut(300).lower().replace(b"t", b"u")]
    hi = bytearray(cut(400))
    for at, ch in ((50, 0x80), (120, 0xC1), (121, 0xFF), (300, 0xE7)):  # 0xC1 & 0x7F == 'A', 0xE7 & 0x5F == 'G'
        hi[at] = ch
    seqs.append(bytes(hi))
    every = bytearray(cut(40 * k))
    every[k - 1::k] = b"N" * len(every[k - 1::k])  # a non-base every k-th byte: no k-mer at all
    seqs.append(bytes(every))
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, TILE - HALO - 1, TILE - HALO, TILE - HALO + 1):
        seqs.append(cut(n))
    return seqs


@pytest.fixture(scope="module")
def edge_setup():
    rng = np.random.default_rng(17)
    base = random_bases(rng, 60000)
    ks = (2, 16, 21, 31)
    yaks = [yak_of(base + b"\n", k) for k in ks]
    pol = Polisher(yaks)
    yield rng, base, ks, [yak_table(y) for y in yaks], pol
    pol.close()


def test_edge_sequences(edge_setup):
    rng, base, ks, tables, pol = edge_setup
    for t, k in enumerate(ks):
        seqs = edge_sequences(rng, base, k)
        for min_count in (1, 2):
            r = same_as_numpy(pol, t, k, tables[t], seqs, min_count)
        assert [int(x) for x in r.stats[:6, 0]] == [0, 0, 1, 2, 0, 0] and int(r.stats[10, 0]) == 0
        assert pol.qv_strings(t, []).stats.shape == (0, 2)
        assert pol.qv_strings(t, [b"", b""], hist=True, bits=True).n_kmers == 0


def test_5000_short_sequences_in_one_call(edge_setup):
    rng, base, ks, tables, pol = edge_setup
    seqs = []
    for _ in range(5000):
        n = int(rng.integers(0, 201))
        a = int(rng.integers(0, len(base) - n))
        seqs.append(noisy(rng, base[a:a + n], 0.02))
    for t, k in ((1, 16), (3, 31)):
        r = same_as_numpy(pol, t, k, tables[t], seqs, 1)
        assert 0 < r.n_absent < r.n_kmers


@pytest.mark.parametrize("stage_tiles", [1, 3])
def test_pieces_of_the_staging_buffer_lose_and_double_nothing(edge_setup, monkeypatch, stage_tiles):
    """NP2_QV_TEST_STAGE_TILES: a staging buffer of a few tiles, so that sequences go on from piece to piece"""
    rng, base, ks, tables, pol = edge_setup
    monkeypatch.setenv("NP2_QV_TEST_STAGE_TILES", str(stage_tiles))
    a = int(rng.integers(0, 1000))
    seqs = edge_sequences(rng, base, 21) + [noisy(rng, base[a:a + 5 * TILE + 77]), b"", noisy(rng, base[:4 * TILE])]
    for t, k in ((2, 21), (3, 31)):
        same_as_numpy(pol, t, k, tables[t], seqs, 1)


# ---- 5. no k-mer spans two sequences ---------------------------------------------------------------------------------------------
def test_no_kmer_leaks_across_sequences():
    """The table is counted from the CONCATENATION of the sequences without separators: every junction k-mer is present,
    so a k-mer leaking across two sequences would show as an extra k-mer, not as an absent one."""
    rng = np.random.default_rng(23)
    lens = [TILE, 2 * TILE, 40, TILE - HALO, 3, 100, TILE, 31, 30, TILE + 1, 2 * TILE, 64]
    seqs = [random_bases(rng, n) for n in lens]
    ks = (16, 31)
    pol = Polisher([yak_of(b"".join(seqs) + b"\n", k) for k in ks])
    for t, k in enumerate(ks):
        for order in (seqs, seqs[::-1]):
            r = pol.qv_strings(t, order, 1, bits=True)
            assert [int(x) for x in r.stats[:, 0]] == [max(0, len(s) - k + 1) for s in order]
            assert r.n_absent == 0 and not any(b.any() for b in r.bits)
    pol.close()


# ---- 6. a table that repeats keys ----------------------------------------------------------------------------------------------------
def test_repeated_keys_answer_like_lookup_hashes():
    """A hand-made dump with repeated keys in its buckets (yak writes none): the last word in file order that passes the
    threshold is the k-mer's count, as the polish kernels' lookup has it."""
    rng = np.random.default_rng(29)
    base = random_bases(rng, 20000)
    k = 21
    words, off = numpy_count(base + b"\n", k)
    out_words, out_off = [], [0]
    for b in range(1024):
        w = words[int(off[b]):int(off[b + 1])]
        extra = []
        for x in w[::3]:  # every third word again, with other counts, before and after the original
            key = x & ~np.uint64(1023)
            extra += [key | np.uint64(9), key | np.uint64(2)]
        w = np.concatenate([np.array(extra[::2], np.uint64), w, np.array(extra[1::2], np.uint64)])
        out_words.append(w)
        out_off.append(out_off[-1] + len(w))
    pol = Polisher([Yak(k, np.concatenate(out_words), np.array(out_off, np.uint64))])
    seqs = [noisy(rng, base[:9000]), noisy(rng, base[9000:]), base[100:130]]
    per = [kmer_hashes_at(s, k) for s in seqs]
    seen = set()
    for min_count in (1, 2, 3, 9, 10):
        r = pol.qv_strings(0, seqs, min_count, hist=True, bits=True)
        e_hist = np.zeros(1024, np.uint64)
        for i, (valid, hashes) in enumerate(per):
            counts = np.zeros(len(valid), np.uint32)
            counts[valid] = pol.lookup_hashes(0, hashes[valid], min_count)
            nk, na, h, bits = aggregate(valid, counts)
            assert (int(r.stats[i, 0]), int(r.stats[i, 1])) == (nk, na) and np.array_equal(r.bits[i], bits), (min_count, i)
            e_hist += h
        assert np.array_equal(r.hist, e_hist)
        seen.add(tuple(int(x) for x in np.flatnonzero(r.hist)))
    assert len(seen) >= 3  # (the threshold chooses among a key's words: 2 / 9 / the original come and go)
    pol.close()


# ---- 6b. probe chains that wrap inside a crowded sub-table ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowded(k):
    """(sequence, hashes[1024, 7], counts[1024, 7]): a seeded 200 kb sequence and, for every bucket, seven of its k-mers
    (the count model's distinct hashes) whose probe chain starts in slot 14 or 15 of a 16-slot sub-table, with distinct
    counts.  A table of at most seven words per bucket is uploaded into 16-slot sub-tables (2 * 7 + 2), so every chain
    of three and more of them runs 14, 15, 0, 1, ... and wraps; the bucket's other late-start k-mers (at least one, by the
    precondition) are not in the table and walk the whole chain to an EMPTY slot.  Shared with the trio and triobin tests."""
    seq = random_bases(np.random.default_rng(7), 200_000)
    h = np.unique(stream_hashes(seq + b"\n", k))
    late = h[((h >> np.uint64(10)) & np.uint64(15)) >= 14]
    per = [late[(late & np.uint64(1023)) == b] for b in range(1024)]
    assert min(len(x) for x in per) >= 8, (k, min(len(x) for x in per))  # the seed's precondition
    hashes = np.stack([x[:7] for x in per])
    counts = np.tile(np.arange(2, 9, dtype=np.uint64), (1024, 1))
    return seq, hashes, counts


def dump_of(hashes, counts):
    """(words, bucket_off) of a dump holding `hashes` (distinct) with `counts`: bucket-major, ascending inside a bucket"""
    order = np.lexsort((hashes, hashes & np.uint64(1023)))
    h, c = hashes[order], counts[order]
    off = np.zeros(1025, np.uint64)
    off[1:] = np.cumsum(np.bincount((h & np.uint64(1023)).astype(np.int64), minlength=1024))
    return ((h >> np.uint64(10)) << np.uint64(10)) | c, off


@pytest.mark.parametrize("k", [21, 31])
def test_probe_chains_wrap_inside_crowded_subtables(monkeypatch, k):
    seq, hashes, counts = crowded(k)
    yak = Yak(k, *dump_of(hashes.ravel(), counts.ravel()))
    assert int(np.diff(yak.bucket_off.astype(np.int64)).max()) == 7  # 16-slot sub-tables
    pol = Polisher([yak])
    valid, hh = kmer_hashes_at(seq, k)
    for min_count in (1, 5):
        found = np.zeros(len(valid), np.uint32)
        found[valid] = pol.lookup_hashes(0, hh[valid], min_count)
        nk, na, e_hist, e_bits = aggregate(valid, found)
        m_nk, m_na, m_hist, m_bits = numpy_qv(seq, k, yak_table(yak), min_count)
        assert (nk, na) == (m_nk, m_na) and np.array_equal(e_hist, m_hist) and np.array_equal(e_bits, m_bits)
        assert nk - na >= 1024 * (4 if min_count == 5 else 7) and na > 1024
        for stage_tiles in (None, 1):
            if stage_tiles is not None:
                monkeypatch.setenv("NP2_QV_TEST_STAGE_TILES", str(stage_tiles))
            r = pol.qv_strings(0, [seq], min_count, hist=True, bits=True)
            assert (r.n_kmers, r.n_absent) == (nk, na), (k, min_count, stage_tiles)
            assert np.array_equal(r.hist, e_hist) and np.array_equal(r.bits[0], e_bits), (k, min_count, stage_tiles)
        monkeypatch.delenv("NP2_QV_TEST_STAGE_TILES")
    pol.close()


# ---- 7. host path == device path --------------------------------------------------------------------------------------------------------
def test_device_path_equals_host_path_after_a_polish():
    from nextpolish2_amd.synth import Synth
    s = Synth(60000, depth=30, seed=11, diploid=True, read_len_mean=9000.0, read_len_sd=1500.0)
    ks = (21, 31)
    yaks = [s.yak(k) for k in ks]
    pol = Polisher(yaks)
    c = pol.upload(s.pileup)
    bases, _ = pol.polish_resident(c, Opts())
    ptr, n = pol.last_result_device()
    seq = bases.tobytes()
    assert n == len(seq)
    for t, k in enumerate(ks):
        table = yak_table(yaks[t])
        for skip, drop in ((0, 0), (1, 0), (3, 5), (17, 1), (HALO + 1, TILE + 3)):  # any alignment, any end
            sub = seq[skip:len(seq) - drop]
            d = pol.qv_device(t, ptr + skip, len(sub), 1, hist=True, bits=True)
            h = pol.qv_strings(t, [sub], 1, hist=True, bits=True)
            assert np.array_equal(d.stats, h.stats) and np.array_equal(d.hist, h.hist) and np.array_equal(d.bits[0], h.bits[0])
            nk, na, e_hist, e_bits = numpy_qv(sub, k, table, 1)
            assert (d.n_kmers, d.n_absent) == (nk, na) and np.array_equal(d.hist, e_hist) and np.array_equal(d.bits[0], e_bits)
        assert pol.qv_device(t, ptr, 0).n_kmers == 0 and pol.qv_device(t, ptr + 5, k - 1).n_kmers == 0
        assert pol.qv_device(t, ptr + 5, k).n_kmers == 1
    c.free()
    pol.close()


# ---- 8. argument errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(edge_setup):
    rng, base, ks, tables, pol = edge_setup
    L = api.lib()
    seq = np.frombuffer(base[:100] + b"\0", dtype=np.uint8)
    off = np.array([0, 60, 100], np.uint64)
    bad_off = np.array([0, 60, 50], np.uint64)
    out = np.zeros((2, 2), np.uint64)

    def strings(yak_idx, strs, o, n, outp):
        return L.np2_qv_strings(pol._h, yak_idx, strs, o, n, 1, outp, None, None, None)

    def device(yak_idx, ptr, n, outp):
        return L.np2_qv_device(pol._h, yak_idx, ptr, n, 1, outp, None, None, None)

    cases = [
        (lambda: strings(len(ks), seq.ctypes.data, off.ctypes.data, 2, out.ctypes.data), "yak_idx"),
        (lambda: strings(-1, seq.ctypes.data, off.ctypes.data, 2, out.ctypes.data), "yak_idx"),
        (lambda: strings(0, seq.ctypes.data, bad_off.ctypes.data, 2, out.ctypes.data), "descending"),
        (lambda: strings(0, seq.ctypes.data, off.ctypes.data, 2, None), "out is NULL"),
        (lambda: strings(0, None, off.ctypes.data, 2, out.ctypes.data), "strs is NULL"),
        (lambda: strings(0, seq.ctypes.data, None, 2, out.ctypes.data), "off is NULL"),
        (lambda: device(len(ks), None, 0, out.ctypes.data), "yak_idx"),
        (lambda: device(0, None, 10, out.ctypes.data), "dev_seq is NULL"),
        (lambda: device(0, None, 0, None), "out is NULL"),
    ]
    for call, text in cases:
        assert call() == E_ARG
        assert text in L.np2_last_error(pol._h).decode(), text
        # the context still answers
        r = pol.qv_strings(2, [base[:100], b""], 1)
        assert [int(x) for x in r.stats[:, 0]] == [80, 0] and r.n_absent == 0
    with pytest.raises(api.Np2Error) as e:
        pol.qv_strings(9, [b"ACGT"])
    assert e.value.code == E_ARG and "yak_idx" in str(e.value)
    assert L.np2_qv_strings(None, 0, None, None, 0, 1, None, None, None, None) == E_ARG
    assert strings(0, None, None, 0, out.ctypes.data) == 0  # n == 0 is fine
