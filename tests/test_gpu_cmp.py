"""K-mer completeness and copy-number spectra on the device (np2_cmp_strings, python -m nextpolish2_amd.completeness, the
command line's --cmp) against the numpy brute force of tests/test_cmp_cpu.py, the known answer on the committed fixtures,
and two independent device paths: the k-mer counter's own table of the set (np2_kcount_bytes) and the QV scan's absent
k-mers (np2_qv_strings).

Every case is one bounded subprocess or a handful of in-process calls."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from nextpolish2_amd import Polisher, api
from nextpolish2_amd import completeness as cmpl
from nextpolish2_amd import io as np2io
from nextpolish2_amd._types import Yak
from test_cmp_cpu import KNOWN, check_identities, numpy_cmp
from test_kcount_cpu import numpy_count
from test_qv_cpu import ASM_IN, ASM_OUT, BAM, BUNDLE, FASTA, fasta_records, read_dump

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
DUMPS = [os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")]
KS = (2, 5, 21, 31)
E_ARG, E_UNSUPPORTED = -1, -4
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def yak_table(y):
    """(sorted hashes, counts) of a Yak without repeated keys"""
    b = np.repeat(np.arange(1024, dtype=np.uint64), np.diff(y.bucket_off.astype(np.int64)))
    h = ((y.words >> np.uint64(10)) << np.uint64(10)) | b
    order = np.argsort(h)
    return h[order], (y.words & np.uint64(1023)).astype(np.uint32)[order]


def yak_of(stream, k, min_count=1):
    return Yak(k, *numpy_count(stream, k, min_count))


def random_bases(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()


def revcomp(s):
    return s.translate(COMP)[::-1]


def same_as_numpy(pol, t, k, table, seqs, min_count):
    r = pol.cmp_strings(t, seqs, min_count, spectra=True)
    stats, spectra, asm_only = numpy_cmp(seqs, k, table, min_count)
    assert r.stats == stats, (k, min_count, r.stats, stats)
    assert r.spectra.shape == (6, 1024) and np.array_equal(r.spectra, spectra), (k, min_count)
    assert r.asm_only.shape == (6,) and np.array_equal(r.asm_only, asm_only), (k, min_count)
    check_identities(r.stats, r.spectra, r.asm_only, min_count)
    # the output nobody asked for changes nothing
    r2 = pol.cmp_strings(t, seqs, min_count)
    assert r2.stats == r.stats and r2.spectra is None and np.array_equal(r2.asm_only, r.asm_only)
    # the other direction's independent path: the QV scan counts the set's k-mers WITH multiplicity
    assert r.n_asm_only <= pol.qv_strings(t, seqs, min_count).n_absent
    return r


class Tables:
    """a Polisher over the tables of one read stream, for every k of KS"""

    def __init__(self, stream, ks=KS, yaks=None):
        self.ks = tuple(ks)
        self.yaks = yaks if yaks is not None else [yak_of(stream, k) for k in self.ks]
        self.tables = [yak_table(y) for y in self.yaks]
        self.pol = Polisher(self.yaks)

    def check(self, seqs, min_counts=(1, 2), ks=None):
        out = {}
        for t, k in enumerate(self.ks):
            if ks is None or k in ks:
                for m in min_counts:
                    out[(k, m)] = same_as_numpy(self.pol, t, k, self.tables[t], seqs, m)
        return out

    def close(self):
        self.pol.close()


# ---- 1. the known answer ---------------------------------------------------------------------------------------------------
def test_known_answer_through_cmp_strings():
    pol = Polisher([np2io.load_yak(p) for p in DUMPS])
    seqs = {side: [s for _, s in fasta_records(FASTA[side])] for side in ("in", "out")}
    absent = {(21, "in"): 32, (21, "out"): 0, (31, "in"): 82, (31, "out"): 10}  # np2_qv_strings' n_absent (test_qv_cpu.py)
    for t, k in enumerate((21, 31)):
        _, th, tc = read_dump(DUMPS[t])
        for side in ("in", "out"):
            for min_count in (1, 2, 5, 20):
                r = same_as_numpy(pol, t, k, (th, tc), seqs[side], min_count)
                assert r.kernel_ms > 0
                if (k, side, min_count) in KNOWN:
                    n_read, n_found, text, n_asm, n_asm_only, classes = KNOWN[(k, side, min_count)]
                    assert r.stats == (n_read, n_found, n_asm, n_asm_only)
                    assert tuple(int(x) for x in r.spectra.sum(axis=1)) == classes
                    assert cmpl.completeness_text(r.n_found, r.n_read) == text
                if min_count <= 2:  # every absent k-mer of these fixtures is single-copy: distinct == with multiplicity
                    assert r.n_asm_only == absent[(k, side)] == pol.qv_strings(t, seqs[side], min_count).n_absent
    pol.close()


# ---- 2. the smallest shapes where the kernels can go wrong ------------------------------------------------------------------
@pytest.fixture(params=[None, "3"], ids=["grid", "3-blocks"])
def blocks(request, monkeypatch):
    """NP2_CMP_TEST_BLOCKS: three blocks stride over the 8 and more turns of even the smallest table, unevenly"""
    if request.param:
        monkeypatch.setenv("NP2_CMP_TEST_BLOCKS", request.param)
    return request.param


def test_reverse_complement_assembly_finds_everything(blocks):
    rng = np.random.default_rng(41)
    src = random_bases(rng, 9137)
    tb = Tables(src + b"\n")
    for (k, m), r in tb.check([revcomp(src)], (1,)).items():
        assert r.n_found == r.n_read == r.n_asm and r.n_asm_only == 0 and int(r.spectra[0].sum()) == 0
    tb.check([revcomp(src[:4000]), src[3000:]], (1, 2, 3))  # overlapping halves: the middle is 2-copy
    tb.close()


def test_junction_kmer_stays_read_only(blocks):
    """X = A..AT..T occurs in the reads once and in the set only ACROSS the junction of two sequences over {C, G} + its halves"""
    rng = np.random.default_rng(43)
    cg = np.frombuffer(b"CG", dtype=np.uint8)
    for k in KS:
        h = k // 2
        x = b"A" * h + b"T" * (k - h)
        p, q = rng.choice(cg, size=2500).tobytes(), rng.choice(cg, size=2500).tobytes()
        tb = Tables(p + b"\n" + q + b"\n" + x + b"\n", ks=(k,))
        r = tb.check([p + x[:h], x[h:] + q], (1,))[(k, 1)]
        assert int(r.spectra[0].sum()) == 1 and r.n_found == r.n_read - 1  # X alone, and it is not found
        r = tb.check([p + x + q], (1,))[(k, 1)]                             # one sequence: now it is
        assert int(r.spectra[0].sum()) == 0 and r.n_found == r.n_read
        tb.close()


def test_non_bases_and_lower_case_inside_a_sequence(blocks):
    rng = np.random.default_rng(47)
    src = random_bases(rng, 6000)
    tb = Tables(src + b"\n")
    a = bytearray(src)
    a[1000:1800] = bytes(a[1000:1800]).lower()
    a[2500:2600] = bytes(a[2500:2600]).replace(b"T", b"U")
    for at in (17, 2000, 2001, 2040, 4000, 5999):
        a[at] = ord("N")
    a[3000], a[3100] = 0x80, 0xC1  # (0xC1 & 0x7F == 'A': a high byte is no base)
    res = tb.check([bytes(a), b"NNNN", b"acgu" * 20], (1, 2))
    r = res[(31, 1)]
    assert 0 < r.n_found < r.n_read  # (the k-mers across an N are lost, the rest is found)
    tb.close()


def test_copy_number_classes_and_the_4_5_boundary(blocks):
    rng = np.random.default_rng(53)
    copies = (1, 2, 4, 5, 6)
    chunks = [random_bases(rng, 400) for _ in copies]
    extra = random_bases(rng, 3000)  # read k-mers the set does not have
    tb = Tables(b"\n".join(chunks) + b"\n" + extra + b"\n")
    seqs = []
    for c, m in zip(chunks, copies):
        seqs += [c if i % 2 == 0 else revcomp(c) for i in range(m)]
    res = tb.check(seqs, (1, 2))
    for k in (21, 31):  # (random 400-mers share no k-mer at these k: every chunk's k-mers have exactly its copy number)
        per_class = [int(x) for x in res[(k, 1)].spectra.sum(axis=1)]
        n = 400 - k + 1
        assert per_class == [3000 - k + 1, n, n, 0, n, 2 * n]
    tb.close()


def test_saturated_copy_number_is_one_kmer_in_class_5(blocks):
    rng = np.random.default_rng(59)
    src = random_bases(rng, 2000)
    for k in KS:
        tb = Tables(src + b"\n" + b"A" * (k + 2) + b"\n", ks=(k,))  # the reads count A..A three times (more at small k)
        c_a = int(tb.tables[0][1].max()) if k <= 5 else 3
        res = tb.check([b"A" * 3000], (1, 1023))                    # cn = min(3000 - k + 1, 1023) = 1023
        r = res[(k, 1)]
        assert r.n_asm == 1 and r.n_found == 1 and int(r.spectra[5].sum()) == 1 and r.n_asm_only == 0
        if k > 5:
            assert int(r.spectra[5, c_a]) == 1
            r = res[(k, 1023)]  # the reads' A..A is below the threshold now: the set's only k-mer is asm_only, class 5
            assert r.n_read == 0 and [int(x) for x in r.asm_only] == [0, 0, 0, 0, 0, 1]
        tb.close()


def test_short_and_empty_sequences_and_the_empty_set(blocks):
    rng = np.random.default_rng(61)
    src = random_bases(rng, 3000)
    tb = Tables(src + b"\n")
    for t, k in enumerate(KS):
        n_read = len(tb.tables[t][0])
        for seqs in ([], [b""], [b"", b""], [src[:k - 1]], [src[5:5 + k - 1], b"", src[40:40 + k - 1]], [b"N" * 50]):
            r = same_as_numpy(tb.pol, t, k, tb.tables[t], seqs, 1)
            assert r.stats == (n_read, 0, 0, 0) and int(r.spectra[0].sum()) == n_read
        r = same_as_numpy(tb.pol, t, k, tb.tables[t], [src[:k], b"", src[100:100 + k + 1], src[:k - 1]], 1)
        assert 1 <= r.n_asm <= 3 and r.n_found == r.n_asm
    tb.close()


def test_no_reliable_read_kmer_at_all(blocks):
    rng = np.random.default_rng(67)
    src = random_bases(rng, 300)  # (short: at k = 2 no count reaches the threshold either)
    tb = Tables(src + b"\n")
    assert all(int(tc.max()) < 1023 for _, tc in tb.tables)
    for (k, m), r in tb.check([src, revcomp(src)], (1023,)).items():
        assert r.n_read == 0 and r.n_found == 0 and r.n_asm_only == r.n_asm > 0 and int(r.spectra.sum()) == 0
        assert np.isnan(r.completeness) and cmpl.completeness_text(r.n_found, r.n_read) == "nan"
    tb.close()


def test_thresholds_at_the_ends_of_the_count_range(blocks):
    """stored counts 1, 2, 1022 and 1023 in the reads' table, min_count 0, 1, 2 and 1023"""
    rng = np.random.default_rng(71)
    src = random_bases(rng, 5000)
    yaks = []
    for k in KS:
        words, off = numpy_count(src + b"\n", k)
        counts = np.array([1, 2, 1022, 1023], np.uint64)[np.arange(len(words)) % 4]
        yaks.append(Yak(k, (words & ~np.uint64(1023)) | counts, off))
    tb = Tables(None, yaks=yaks)
    res = tb.check([src[:3000], revcomp(src[2000:4500])], (0, 1, 2, 1023))
    for k in (21, 31):
        n = len(tb.tables[KS.index(k)][0])
        assert res[(k, 0)].stats == res[(k, 1)].stats and res[(k, 0)].n_read == n
        assert res[(k, 2)].n_read == n - (n + 3) // 4 and res[(k, 1023)].n_read == n // 4
        assert res[(k, 1)].n_asm_only == 0 < res[(k, 2)].n_asm_only < res[(k, 1023)].n_asm_only
    tb.close()


def test_small_sub_tables_and_many_pieces_in_a_child(tmp_path):
    """NP2_KCOUNT_TEST_CAP_LOG2=4, NP2_KCOUNT_TEST_PIECE=4096: the set's table starts with 16-slot sub-tables and grows
    several times, its probe chains wrap inside the sub-tables, and the set spans many pieces"""
    rng = np.random.default_rng(73)
    src = random_bases(rng, 20000)
    seqs = [src[:9000], revcomp(src[8000:15000]), src[100:131], b"", src[15000:] + b"N" + src[:500]]
    ks = (5, 21, 31)
    yaks = [yak_of(src + b"\n", k) for k in ks]
    inp, out = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(inp, **{f"w{i}": y.words for i, y in enumerate(yaks)}, **{f"o{i}": y.bucket_off for i, y in enumerate(yaks)},
             **{f"s{i}": np.frombuffer(s, dtype=np.uint8) for i, s in enumerate(seqs)})
    code = ("import numpy as np\nfrom nextpolish2_amd import Polisher, io\nfrom nextpolish2_amd._types import Yak\n"
            f"d = np.load({str(inp)!r})\nks = {ks!r}\n"
            "pol = Polisher([Yak(k, d[f'w{i}'], d[f'o{i}']) for i, k in enumerate(ks)])\n"
            f"seqs = [d[f's{{i}}'].tobytes() for i in range({len(seqs)})]\n"
            "res = {}\n"
            "for t, k in enumerate(ks):\n"
            "    for m in (1, 2):\n"
            "        r = pol.cmp_strings(t, seqs, m, spectra=True)\n"
            "        res[f'st_{k}_{m}'], res[f'sp_{k}_{m}'], res[f'ao_{k}_{m}'] = np.array(r.stats, np.uint64), r.spectra, r.asm_only\n"
            "        res[f'gr_{k}_{m}'] = io.kcount_last_stats()['growths']\n"
            f"np.savez({str(out)!r}, **res)\n")
    env = dict(ENV, NP2_KCOUNT_TEST_CAP_LOG2="4", NP2_KCOUNT_TEST_PIECE="4096", NP2_CMP_TEST_BLOCKS="5")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], capture_output=True, env=env, timeout=180)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got = np.load(out)
    for t, k in enumerate(ks):
        for m in (1, 2):
            stats, spectra, asm_only = numpy_cmp(seqs, k, yak_table(yaks[t]), m)
            assert tuple(int(x) for x in got[f"st_{k}_{m}"]) == stats, (k, m)
            assert np.array_equal(got[f"sp_{k}_{m}"], spectra) and np.array_equal(got[f"ao_{k}_{m}"], asm_only), (k, m)
            if k >= 21:  # ~20 000 k-mers in 1 024 sub-tables of 16 slots: 16 -> 32 -> 64 and further
                assert int(got[f"gr_{k}_{m}"]) >= 2


@pytest.mark.parametrize("test_blocks", [None, "7"])
def test_read_table_of_3e5_kmers(monkeypatch, test_blocks):
    """2^20 slots in the reads' table (512 turns of a block) and as many in the set's: one turn per block of the device's
    grid, 73 and a bit per block of a grid of seven"""
    if test_blocks:
        monkeypatch.setenv("NP2_CMP_TEST_BLOCKS", test_blocks)
    rng = np.random.default_rng(79)
    src = random_bases(rng, 300_000)
    tb = Tables(src + b"\n", ks=(21,))
    assert 290_000 < len(tb.tables[0][0]) <= 300_000
    a = bytearray(src[20_000:280_000])
    a[100_000:100_010] = b"N" * 10
    r = tb.check([bytes(a), revcomp(src[:30_000]), random_bases(rng, 5000)], (1,))[(21, 1)]
    assert r.n_asm_only > 4900 and 0 < r.n_found < r.n_read and int(r.spectra[2].sum()) > 9000
    tb.close()


# ---- 3. independent device paths ---------------------------------------------------------------------------------------------
def test_sampled_read_kmers_have_the_counters_copy_number():
    """The set counted by np2_kcount_bytes (io.count_kmers), fetched to the host: for a SAMPLE of the reads' k-mers, held
    by a table of their own, the spectrum is the histogram of (min(that count, 5), stored read count)."""
    rng = np.random.default_rng(83)
    src = random_bases(rng, 12000)
    seqs = [src[:7000], revcomp(src[5000:9000]), src[6000:6400], src[6000:6400], src[6000:6400], src[6100:6300], b"A" * 1500]
    stream = b"".join(s + b"\n" for s in seqs)
    for k in (5, 21, 31):
        words, off = numpy_count(src + b"\n" + b"A" * 40 + b"\n", k)
        b = np.repeat(np.arange(1024, dtype=np.uint64), np.diff(off.astype(np.int64)))
        keep = rng.random(len(words)) < 0.3
        s_off = np.zeros(1025, np.uint64)
        s_off[1:] = np.cumsum(np.bincount(b[keep].astype(np.int64), minlength=1024))
        sample = Yak(k, words[keep], s_off)
        sh, sc = yak_table(sample)
        ah, ac = yak_table(np2io.count_kmers(stream, [k], min_count=1)[0])
        at = np.minimum(np.searchsorted(ah, sh), len(ah) - 1)
        cn = np.where(ah[at] == sh, ac[at], 0).astype(np.int64)
        exp = np.zeros((6, 1024), np.uint64)
        np.add.at(exp, (np.minimum(cn, 5), sc.astype(np.int64)), 1)
        pol = Polisher([sample])
        r = pol.cmp_strings(0, seqs, 1, spectra=True)
        assert np.array_equal(r.spectra, exp), k
        assert r.n_asm == len(ah) and int(exp[1:].sum()) == r.n_found > 0 and int(exp[5].sum()) >= 1
        pol.close()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable():
    rng = np.random.default_rng(89)
    base = random_bases(rng, 2000)
    pol = Polisher([yak_of(base + b"\n", 21)])
    L = api.lib()
    seq = np.frombuffer(base[:100] + b"\0", dtype=np.uint8)
    off = np.array([0, 60, 100], np.uint64)
    bad_off = np.array([0, 60, 50], np.uint64)
    out = np.zeros(4, np.uint64)

    def call(yak_idx, strs, o, n, outp, min_count=2):
        return L.np2_cmp_strings(pol._h, yak_idx, strs, o, n, min_count, outp, None, None, None)

    cases = [
        (lambda: call(1, seq.ctypes.data, off.ctypes.data, 2, out.ctypes.data), "yak_idx"),
        (lambda: call(-1, seq.ctypes.data, off.ctypes.data, 2, out.ctypes.data), "yak_idx"),
        (lambda: call(0, seq.ctypes.data, off.ctypes.data, 2, out.ctypes.data, 1024), "min_count"),
        (lambda: call(0, seq.ctypes.data, off.ctypes.data, 2, None), "out is NULL"),
        (lambda: call(0, seq.ctypes.data, None, 2, out.ctypes.data), "off is NULL"),
        (lambda: call(0, seq.ctypes.data, bad_off.ctypes.data, 2, out.ctypes.data), "descending"),
        (lambda: call(0, None, off.ctypes.data, 2, out.ctypes.data), "strs is NULL"),
    ]
    for fn, text in cases:
        assert fn() == E_ARG
        assert text in L.np2_last_error(pol._h).decode(), text
        r = pol.cmp_strings(0, [base[:100], b""], 1)  # the context still answers
        assert r.n_asm == 80 == r.n_found and r.n_asm_only == 0
    with pytest.raises(api.Np2Error) as e:
        pol.cmp_strings(3, [b"ACGT"])
    assert e.value.code == E_ARG and "yak_idx" in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        pol.cmp_strings(0, [b"ACGT"], min_count=1024)
    assert e.value.code == E_ARG and "min_count" in str(e.value)
    assert L.np2_cmp_strings(None, 0, None, None, 0, 1, None, None, None, None) == E_ARG
    assert call(0, None, None, 0, out.ctypes.data) == 0  # n == 0 is fine
    pol.close()


def test_a_table_that_repeats_keys_is_unsupported():
    rng = np.random.default_rng(97)
    base = random_bases(rng, 3000)
    words, off = numpy_count(base + b"\n", 21)
    out_words, out_off = [], [0]
    for b in range(1024):
        w = words[int(off[b]):int(off[b + 1])]
        w = np.concatenate([w, (w[:1] & ~np.uint64(1023)) | np.uint64(9)])  # every bucket's first key once more
        out_words.append(w)
        out_off.append(out_off[-1] + len(w))
    pol = Polisher([Yak(21, np.concatenate(out_words), np.array(out_off, np.uint64)), yak_of(base + b"\n", 31)])
    with pytest.raises(api.Np2Error) as e:
        pol.cmp_strings(0, [base])
    assert e.value.code == E_UNSUPPORTED and "repeats keys" in str(e.value)
    assert pol.cmp_strings(1, [base], 1).n_found == len(base) - 30  # the other table, and the context, still answer
    pol.close()


# ---- 5. the module and the command line on the bundle --------------------------------------------------------------------------
def parse_tsv(path):
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def known_row(name, k, side):
    n_read, n_found, text, n_asm, n_asm_only, _ = KNOWN[(k, side, 2)]
    return [name, str(k), str(n_read), str(n_found), text, str(n_asm), str(n_asm_only)]


def parse_spectra(path):
    head, rows = parse_tsv(path)
    assert head == list(cmpl.SPECTRA_HEADER)
    sp, ao = np.zeros((6, 1024), np.uint64), np.zeros(6, np.uint64)
    for copies, count, kmers in rows:
        if copies.startswith("asm-only:"):
            assert count == "0"
            ao[cmpl.COPIES.index(copies[len("asm-only:"):])] = int(kmers)
        else:
            sp[cmpl.COPIES.index(copies), int(count)] = int(kmers)
    return sp, ao


def test_known_answer_through_the_module_with_hap2(tmp_path):
    tsv, prefix = str(tmp_path / "c.tsv"), str(tmp_path / "sp")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "nextpolish2_amd.completeness", ASM_IN] + DUMPS
    r = subprocess.run(cmd + ["--hap2", ASM_OUT, "--spectra", prefix, "-o", tsv], capture_output=True, env=ENV, timeout=360)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    head, rows = parse_tsv(tsv)
    assert head == list(cmpl.TSV_HEADER)
    seqs = {"hap1": [s for _, s in fasta_records(ASM_IN)], "hap2": [s for _, s in fasta_records(ASM_OUT)]}
    seqs["both"] = seqs["hap1"] + seqs["hap2"]
    assert rows[:4] == [known_row("hap1", 21, "in"), known_row("hap1", 31, "in"), known_row("hap2", 21, "out"), known_row("hap2", 31, "out")]
    assert [row[:2] for row in rows[4:]] == [["both", "21"], ["both", "31"]]
    for t, k in enumerate((21, 31)):
        _, th, tc = read_dump(DUMPS[t])
        for name in ("hap1", "hap2", "both"):
            stats, spectra, asm_only = numpy_cmp(seqs[name], k, (th, tc), 2)
            if name == "both":
                assert rows[4 + t][2:] == [str(stats[0]), str(stats[1]), cmpl.completeness_text(stats[1], stats[0]), str(stats[2]), str(stats[3])]
                assert int(spectra[2].sum()) > 90000  # (the two assemblies together: the bulk is 2-copy)
            sp, ao = parse_spectra(f"{prefix}.k{k}.{name}.tsv")
            assert np.array_equal(sp, spectra) and np.array_equal(ao, asm_only), (k, name)


@pytest.mark.parametrize("with_qv", [False, True], ids=["cmp", "cmp+qv"])
def test_cli_cmp_on_the_reference_test_bundle(tmp_path, with_qv):
    tsv, prefix, qv_tsv = str(tmp_path / "c.tsv"), str(tmp_path / "sp"), str(tmp_path / "q.tsv")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "nextpolish2_amd.cli", "-t", "5", "-L", "1000", BAM, ASM_IN] + DUMPS
    cmd += ["--cmp", tsv, "--cmp_spectra", prefix] + (["--qv", qv_tsv] if with_qv else [])
    r = subprocess.run(cmd, capture_output=True, env=ENV, timeout=360)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == gzip.open(ASM_OUT, "rb").read()  # byte for byte the FASTA written without --cmp
    head, rows = parse_tsv(tsv)
    assert head == list(cmpl.TSV_HEADER)
    assert rows == [known_row("in", 21, "in"), known_row("in", 31, "in"), known_row("out", 21, "out"), known_row("out", 31, "out")]
    for t, k in enumerate((21, 31)):
        _, th, tc = read_dump(DUMPS[t])
        for side in ("in", "out"):
            _, spectra, asm_only = numpy_cmp([s for _, s in fasta_records(FASTA[side])], k, (th, tc), 2)
            sp, ao = parse_spectra(f"{prefix}.k{k}.{side}.tsv")
            assert np.array_equal(sp, spectra) and np.array_equal(ao, asm_only), (k, side)
    if with_qv:
        assert len(open(qv_tsv).read().splitlines()) == 5
