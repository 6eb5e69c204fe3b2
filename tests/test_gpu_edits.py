"""The edit report on the device (np2_edits_buffers, np2_edits_last, --edits, python -m nextpolish2_amd.edits) against the
plain model of tests/edits_model.py: records, string pools, totals and support counters must be equal exactly.

Every case is a handful of in-process calls or one bounded subprocess.  Block edges: the look-back scans own 8 192
elements per block; the elements of the two bitmap scans are 32-position words (an edge every 262 144 positions), those of
the three scans over runs are runs (an edge at run 8 192)."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import edits_cases as Cs
import edits_model as M
from nextpolish2_amd import Opts, Polisher, edits
from nextpolish2_amd import io as np2io
from nextpolish2_amd._types import Yak
from nextpolish2_amd.api import Np2Error
from test_edits_cpu import BUNDLE_EDITS, BUNDLE_TOTALS
from test_kcount_cpu import numpy_count

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
BUNDLE = os.path.join(ROOT, "tests", "golden", "ref_bundle")
ASM = os.path.join(ROOT, "tests", "golden", "ref_test_asm.fa.gz")
BAM = os.path.join(BUNDLE, "hifi.map.sort.bam")
DUMPS = [os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")]
SIZES = [0, 1, 63, 64, 65, 8191, 8192, 8193, 3 * 8192 + 5]
WORD_EDGE = 32 * 8192  # positions per block of the bitmap scans
E_ARG = -1


def bases_of(seed, n, alphabet=b"ACGT"):
    return np.random.default_rng(seed).choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).astype(np.uint8).tobytes()


GENOME = bases_of(1, 40000)  # what the tables were counted from: contigs cut from it hold present k-mers, edits make absent ones


class Ctx:
    """one context with a 9-mer and a 21-mer table of GENOME, and the model's view of the same tables"""

    def __init__(self):
        self.yaks = [Yak(k, *numpy_count(GENOME + b"\n", k)) for k in (9, 21)]
        self.pol = Polisher(self.yaks)
        self.tables = [M.Table(y) for y in self.yaks]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.pol.close()


def same_as_model(pol, tables, ref, bases, pos, min_count=1, mask=-1):
    """np2_edits_buffers against the model; tables: the model's Table per table of pol; mask: which of them to judge by"""
    res = pol.edits_buffers(ref, bases, pos, min_count=min_count, tables=mask)
    recs, tot = M.edits(ref, bases, pos)
    assert res.records() == recs
    assert [int(e["ref_len"]) for e in res.edits] == [len(r["ref"]) for r in recs]
    assert [int(e["alt_len"]) for e in res.edits] == [len(r["alt"]) for r in recs]
    assert res.ref_pool == b"".join(r["ref"] for r in recs) and res.alt_pool == b"".join(r["alt"] for r in recs)
    assert res.totals == tot
    used = [t for i, t in enumerate(tables) if mask == -1 or (mask >> i) & 1]
    assert res.table_k == [t.k for t in used] and res.support.shape == (len(recs), len(used), 4)
    for j, t in enumerate(used):
        exp = [M.support(ref, bases, r, t, min_count) for r in recs]
        assert [tuple(int(x) for x in res.support[i, j]) for i in range(len(recs))] == exp, t.k
    if tot["has_span"]:
        assert M.apply(ref, recs, tot["first"], tot["last"]).upper() == bytes(bases).upper()
    return res, recs, tot


def genome_case(seed, L, rate=0.02, span=None):
    """random_case on a contig cut from GENOME"""
    at = int(np.random.default_rng(seed).integers(0, len(GENOME) - L + 1))
    return Cs.random_case(seed, L, rate=rate, span=span, ref=GENOME[at:at + L])


# ---- 1. the hand-derived cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(Cs.HAND))
def test_hand_cases(ctx, name):
    ref, (bases, pos), recs, totals, _ = Cs.HAND[name]
    res, got, tot = same_as_model(ctx.pol, ctx.tables, ref, bases, pos)
    assert got == recs and all(tot[k] == v for k, v in totals.items())
    assert set(res.kernel_ms) == set(("flags", "runs", "trim", "shift", "emit", "support")) and all(v >= 0 for v in res.kernel_ms.values())


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SIZES)
def test_contig_lengths_with_seeded_edits(ctx, L):
    ref, bases, pos = genome_case(100 + L, L, rate=0.03)
    _, recs, tot = same_as_model(ctx.pol, ctx.tables, ref, bases, pos)
    if L >= 8191:
        k = tot["n_kind"]
        assert len(recs) > 100 and tot["same_runs"] > 10 and min(k[0], k[2], k[3]) > 0  # (what the generator is for)


@pytest.mark.parametrize("n", SIZES)
def test_output_lengths(ctx, n):
    """exactly n output bases inside a longer contig: substitutions only, positions 5 .. 5 + n - 1"""
    ref = GENOME[777:777 + n + 11]
    b = np.frombuffer(ref[5:5 + n], dtype=np.uint8).copy()
    hit = np.arange(0, n, 37)
    b[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), b[hit]) + 1) % 4]
    _, recs, tot = same_as_model(ctx.pol, ctx.tables, ref, b.tobytes(), np.arange(5, 5 + n, dtype=np.uint32))
    assert len(recs) == len(hit) and tot["outside"] == len(ref) - n


def test_partial_spans_with_seeded_edits(ctx):
    for seed, L, span in ((7, 8193, (100, 8000)), (8, 20000, (8191, 16385)), (9, 300, (299, 299)), (10, 300, (0, 0))):
        same_as_model(ctx.pol, ctx.tables, *genome_case(seed, L, rate=0.05, span=span))


# ---- 3. planted cases -------------------------------------------------------------------------------------------------------
def test_more_than_a_scan_block_of_runs(ctx):
    """every other position substituted: 12 291 raw runs, all real; run 8 191 is the last element of the run scans' first
    block and run 8 192 the first of their second (no tables: the model's support would take minutes)"""
    L = 3 * 8192 + 5
    ref = GENOME[:L]
    b = np.frombuffer(ref, dtype=np.uint8).copy()
    b[::2] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), b[::2]) + 2) % 4]
    res, recs, tot = same_as_model(ctx.pol, ctx.tables, ref, b.tobytes(), np.arange(L, dtype=np.uint32), mask=0)
    assert len(recs) == tot["raw_runs"] == (L + 1) // 2 and recs[8191]["ref_pos"] == 2 * 8191 and res.support.shape == (len(recs), 0, 4)
    # regions [8 i, 8 i + 1] rewritten the same and 8 i + 2 left alone: a run in three is no edit, the compaction moves the rest
    r8 = np.frombuffer(ref, dtype=np.uint8)
    pos, i8 = np.arange(L, dtype=np.uint32), np.arange(0, L - 2, 8)
    b[i8], b[i8 + 1], b[i8 + 2], pos[i8 + 1] = r8[i8], r8[i8 + 1], r8[i8 + 2], i8
    _, recs, tot = same_as_model(ctx.pol, ctx.tables, ref, b.tobytes(), pos, mask=0)
    assert tot["same_runs"] == len(i8) and tot["raw_runs"] > 8192 and len(recs) == tot["raw_runs"] - tot["same_runs"]


def word_edge_contig():
    L = WORD_EDGE + 6000
    return (GENOME * (L // len(GENOME) + 1))[:L]


def test_runs_at_the_bitmap_scans_block_edge(ctx):
    """a run head on the last position of the bitmap scans' first block (bit 31 of word 8 191), a run that straddles the
    edge, and runs in the words on either side"""
    ref = word_edge_contig()
    E = WORD_EDGE
    out = Cs.out_of((ref[:E - 40], 0), (b"T" * 3, [E - 40] * 3), (ref[E - 39:E - 5], E - 39),  # a CPX / INS before the edge
                    (ref[E - 5:E + 7][::-1], [E - 5] * 12), (ref[E + 7:E + 100], E + 7),       # a region across the edge, reversed
                    (ref[E + 100:E + 110], [E + 100] * 10), (ref[E + 110:], E + 110))          # one rewritten the same after it
    _, recs, tot = same_as_model(ctx.pol, ctx.tables, ref, *out)
    assert any(r["ref_pos"] < E < r["ref_pos"] + len(r["ref"]) for r in recs) and tot["same_runs"] >= 1
    # a head exactly on the last position of the block, its run ending there; and one starting on the first of the next
    b = np.frombuffer(ref, dtype=np.uint8).copy()
    for p in (E - 1, E + 1, 0, len(ref) - 1):
        b[p] = ord("A") if b[p] != ord("A") else ord("C")
    _, recs, _ = same_as_model(ctx.pol, ctx.tables, ref, b.tobytes(), np.arange(len(ref), dtype=np.uint32))
    assert [r["ref_pos"] for r in recs] == [0, E - 1, E + 1, len(ref) - 1]


def test_homopolymer_of_9000_carries_an_insertion_across_the_edge(ctx):
    ref = bytearray(word_edge_contig())
    E = WORD_EDGE
    ref[E - 4500:E + 4500] = b"A" * 9000
    ref[E - 4501], ref[E + 4500] = ord("C"), ord("G")
    ref = bytes(ref)
    # two A added at the homopolymer's right end, and further right a deletion inside a second, short one
    out = Cs.out_of((ref[:E + 4499], 0), (b"AAA", [E + 4499] * 3), (ref[E + 4500:], E + 4500))
    _, recs, _ = same_as_model(ctx.pol, ctx.tables, ref, *out)
    assert recs == [dict(ref_pos=E - 4500, out_off=E - 4500, ref=b"", alt=b"AA", kind="INS")]
    # the same with a substitution inside the homopolymer: the shift stops one past it
    b, p = bytearray(out[0]), out[1]
    b[E + 10] = ord("T")
    _, recs, _ = same_as_model(ctx.pol, ctx.tables, ref, bytes(b), p)
    assert [(r["ref_pos"], r["kind"]) for r in recs] == [(E + 10, "SNV"), (E + 11, "INS")]


def test_long_sides_go_to_the_wavefront(ctx):
    """REF and ALT of 65 and of 300 bytes, with and without long common ends"""
    ref = GENOME[3000:9000]
    other = GENOME[20000:21000]
    pieces, at = [], 0

    def region(start, ln, text):
        nonlocal at
        pieces.append((ref[at:start], at))
        pieces.append((text, [start] * len(text)))
        at = start + ln

    region(100, 65, other[:3])                       # REF 65, ALT 3
    region(300, 3, other[10:75])                     # REF 3, ALT 65
    region(600, 300, other[100:107])                 # REF 300, ALT 7
    region(1100, 5, other[200:500])                  # REF 5, ALT 300
    region(1600, 300, ref[1600:1750] + b"N" + ref[1751:1900])   # 300 rewritten, one base in the middle changed: an SNV
    region(2100, 300, ref[2100:2250] + ref[2251:2400])          # ... one dropped: a DEL, then shifted
    region(2600, 300, ref[2600:2900])                           # ... rewritten the same
    region(3100, 65, ref[3100:3165])                            # 65 rewritten the same
    region(3300, 65, ref[3300:3364] + other[:1] + ref[3364:3365])  # 65 with one base added before its last
    region(3600, 300, other[600:900])                # REF 300, ALT 300 of other text: an MNV (or shorter, by chance ends)
    region(4000, 64, other[:64])                     # 64 / 64: the one-lane path at its limit
    region(4200, 64, other[:65])
    pieces.append((ref[at:], at))
    _, recs, tot = same_as_model(ctx.pol, ctx.tables, ref, *Cs.out_of(*pieces))
    assert tot["raw_runs"] == 12 and tot["same_runs"] == 2
    assert (1750, "SNV") in [(r["ref_pos"], r["kind"]) for r in recs] and "DEL" in [r["kind"] for r in recs]


def test_edits_at_the_ends_and_close_together(ctx):
    """edits at 0, at L - 1, at first, at last; two edits closer than k; windows clipped at both sequence ends; an N in a window"""
    ref = bytearray(GENOME[12000:12400])
    ref[200] = ord("N")
    ref = bytes(ref)
    b = bytearray(ref)
    for p in (0, 5, 196, 204, 399):
        b[p] = ord("G") if b[p] != ord("G") else ord("T")
    res, recs, _ = same_as_model(ctx.pol, ctx.tables, ref, bytes(b), np.arange(400, dtype=np.uint32))
    assert [r["ref_pos"] for r in recs] == [0, 5, 196, 204, 399]
    assert int(res.support[0, 1, 0]) == 1 and int(res.support[4, 1, 0]) == 1  # (one 21-mer fits a window clipped to 21 bases)
    assert int(res.support[2, 1, 0]) < 21  # (the N breaks k-mers of the window around 196)
    # the same edits with first = 3 and last = 396: those at 0 and 399 lie outside the span; those at 5 and 396 stay
    b[396] = ord("G") if b[396] != ord("G") else ord("T")
    b[3] = ord("G") if b[3] != ord("G") else ord("T")
    _, recs, tot = same_as_model(ctx.pol, ctx.tables, ref, bytes(b[3:397]), np.arange(3, 397, dtype=np.uint32))
    assert [r["ref_pos"] for r in recs] == [3, 5, 196, 204, 396] and tot["outside"] == 6
    # a contig shorter than k
    same_as_model(ctx.pol, ctx.tables, b"ACGTACG", b"ACTTACG", np.arange(7, dtype=np.uint32))


def test_table_choice_and_threshold(ctx):
    ref, bases, pos = genome_case(77, 5000, rate=0.03)
    for mask in (0, 1, 2, 3, -1):
        same_as_model(ctx.pol, ctx.tables, ref, bases, pos, mask=mask)
    for min_count in (0, 2, 3):
        same_as_model(ctx.pol, ctx.tables, ref, bases, pos, min_count=min_count)
    with pytest.raises(Np2Error) as e:
        ctx.pol.edits_buffers(ref, bases, pos, tables=4)
    assert e.value.code == E_ARG and "table 2" in str(e.value)
    nopol = Polisher([])
    res = nopol.edits_buffers(ref, bases, pos)
    assert res.records() == M.edits(ref, bases, pos)[0] and res.support.shape == (len(res), 0, 4)
    nopol.close()


def test_a_table_that_repeats_keys():
    """a hand-made dump with repeated keys in its buckets (yak writes none): the last word in file order that passes the
    threshold is the k-mer's count"""
    k = 21
    words, off = numpy_count(GENOME[:20000] + b"\n", k)
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
    y = Yak(k, np.concatenate(out_words), np.array(out_off, np.uint64))
    pol, table = Polisher([y]), M.Table(y)
    ref, bases, pos = genome_case(31, 6000, rate=0.02)
    seen = set()
    for min_count in (1, 2, 3, 9, 10):
        res, _, _ = same_as_model(pol, [table], ref, bases, pos, min_count=min_count)
        seen.add(res.support.tobytes())
    assert len(seen) >= 3  # (the threshold chooses among a key's words)
    pol.close()


# ---- 4. errors -----------------------------------------------------------------------------------------------------------------
def test_bad_positions_are_an_argument_error_not_a_fault(ctx):
    ref, bases, pos = genome_case(5, 20000, rate=0.02)
    good = ctx.pol.edits_buffers(ref, bases, pos).records()
    for at in (1, len(pos) // 2, len(pos) - 1):
        bad = pos.copy()
        bad[at] = bad[at - 1] - 1 if bad[at - 1] else 0
        if at == 1 and bad[1] >= bad[0]:
            bad[0] = 7
        with pytest.raises(Np2Error) as e:
            ctx.pol.edits_buffers(ref, bases, bad)
        assert e.value.code == E_ARG and "decrease" in str(e.value)
    for at, v in ((0, len(ref)), (len(pos) - 1, len(ref)), (len(pos) // 2, 0xFFFFFFFF), (len(pos) - 1, 0xFFFFFFFF)):
        bad = pos.copy()
        bad[at] = v
        with pytest.raises(Np2Error) as e:
            ctx.pol.edits_buffers(ref, bases, bad)
        assert e.value.code == E_ARG
    with pytest.raises(Np2Error) as e:
        ctx.pol.edits_buffers(b"", b"A", np.zeros(1, dtype=np.uint32))
    assert e.value.code == E_ARG
    with pytest.raises(Np2Error) as e:
        ctx.pol.edits_last(type("C", (), {"_h": None})())
    assert e.value.code == E_ARG
    assert ctx.pol.edits_buffers(ref, bases, pos).records() == good  # the context goes on working


# ---- 5. the bundle: np2_edits_last == np2_edits_buffers == the model ----------------------------------------------------
def test_last_equals_buffers_equals_the_model_on_the_bundle():
    (name, ref), = list(np2io.read_fasta(ASM))
    yaks = [np2io.load_yak(p) for p in DUMPS]
    pol = Polisher(yaks)
    c = np2io.contig_from_bam(pol, np2io.Bam(BAM), name, ref, np2io.FrontOpts())
    with pytest.raises(Np2Error) as e:  # nothing polished yet
        pol.edits_last(c)
    assert e.value.code == E_ARG
    b, p = pol.polish_resident(c, Opts())
    last = pol.edits_last(c)
    res, recs, tot = same_as_model(pol, [M.Table(y) for y in yaks], ref, b.tobytes(), p)
    assert last.records() == res.records() and last.totals == res.totals and np.array_equal(last.support, res.support)
    assert [(r["ref_pos"], r["out_off"], r["ref"], r["alt"], r["kind"]) for r in recs] == BUNDLE_EDITS
    assert all(tot[k] == v for k, v in BUNDLE_TOTALS.items())
    # the support identity: the edits are at least k apart and the span is the whole contig
    for t, (drop_in, drop_out) in enumerate(((32, 0), (82, 10))):
        assert int(res.support[:, t, 1].sum()) - int(res.support[:, t, 3].sum()) == drop_in - drop_out
    # with the sequence left on the device (deferred output) the report is the same
    pol.polish_resident(c, Opts(), defer_output=True)
    assert pol.edits_last(c, tables=1).records() == res.records()
    c.free()
    pol.close()


# ---- 6. the command line ------------------------------------------------------------------------------------------------------
def bundle_vcf():
    (name, ref), = list(np2io.read_fasta(ASM))
    head = edits.vcf_header([(name, len(ref))], [21, 31])
    return name, ref, head


def test_cli_edits_on_the_reference_test_bundle(tmp_path):
    vcf, tsv = str(tmp_path / "e.vcf"), str(tmp_path / "e.tsv")
    cmd = [sys.executable, "-m", "nextpolish2_amd.cli", "-t", "5", BAM, ASM] + DUMPS
    r = subprocess.run(cmd + ["-L", "1000", "--edits", vcf, "--edits_summary", tsv], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == gzip.open(os.path.join(BUNDLE, "expected.fa.gz"), "rb").read()  # byte for byte the FASTA written without --edits
    name, ref, head = bundle_vcf()
    lines = open(vcf, "rb").read().splitlines(keepends=True)
    assert lines[:len(head)] == head
    body = [ln.split(b"\t") for ln in lines[len(head):]]
    assert [(int(f[1]), f[3], f[4]) for f in body] == [edits.anchor(ref, s, r, a, k) for s, _, r, a, k in BUNDLE_EDITS]
    assert all(f[0] == name.encode() and b"KIND=INS" in f[7] and b"VERDICT=better" in f[7] for f in body)
    assert [f[7].split(b";")[1] for f in body] == [b"OUT=%d" % o for _, o, _, _, _ in BUNDLE_EDITS]
    rows = [ln.split("\t") for ln in open(tsv).read().splitlines()]
    assert rows[0] == list(edits.SUMMARY_HEADER) and len(rows) == 2
    row = dict(zip(rows[0], rows[1]))
    assert (row["contig"], row["polished"], row["raw_runs"], row["same_runs"], row["edits"], row["INS"], row["bases_inserted"], row["better"]) == \
           (name, "1", "2128", "2124", "4", "4", "4", "4")
    # without -L the contig passes through: a summary row of zeros, no record
    r = subprocess.run(cmd + ["--edits", vcf, "--edits_summary", tsv], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert open(vcf, "rb").read().splitlines(keepends=True) == head
    assert open(tsv).read().splitlines()[1].split("\t") == [name, str(len(ref))] + ["0"] * (len(edits.SUMMARY_HEADER) - 2)


def test_stand_alone_tool_on_an_out_pos_text_gives_the_same_vcf(tmp_path):
    vcf, txt, vcf2, tsv2 = (str(tmp_path / n) for n in ("e.vcf", "o.tsv", "e2.vcf", "e2.tsv"))
    cmd = [sys.executable, "-m", "nextpolish2_amd.cli", "-L", "1000", BAM, ASM] + DUMPS
    r = subprocess.run(cmd + ["--edits", vcf, "-o", str(tmp_path / "o.fa")], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run(cmd + ["--out_pos", "-o", txt], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.edits", ASM, txt] + DUMPS + ["-o", vcf2, "--summary", tsv2],
                       capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert open(vcf2, "rb").read() == open(vcf, "rb").read() and open(vcf, "rb").read().count(b"KIND=INS") == 4
    assert open(tsv2).read().splitlines()[1].split("\t")[6:9] == ["2128", "2124", "4"]
    # refused where they cannot work
    r = subprocess.run(cmd + ["--out_pos", "--edits", vcf], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 2 and b"--out_pos" in r.stderr


def parse_vcf(path):
    per = {}
    for ln in open(path, "rb").read().splitlines():
        if not ln.startswith(b"#"):
            f = ln.split(b"\t")
            per.setdefault(f[0].decode(), []).append((int(f[1]), f[3], f[4], f[7]))
    return per


def apply_vcf(ref, recs, first, last):
    """anchored VCF records applied to ref[first .. last]"""
    out, at = [], first
    for pos, r, a, _ in recs:
        out.append(ref[at:pos - 1])
        out.append(a)
        at = pos - 1 + len(r)
    out.append(ref[at:last + 1])
    return b"".join(out)


def test_two_synthetic_contigs_through_the_batch_driver(tmp_path):
    from nextpolish2_amd.bamio import pileup_to_records, write_bam
    from nextpolish2_amd.synth import Synth
    syn = [Synth(30000, depth=15, seed=900 + i, diploid=True, read_len_mean=5000.0, read_len_sd=700.0, name=f"c{i}") for i in range(2)]
    recs = []
    for i, s in enumerate(syn):
        recs += pileup_to_records(s.pileup, tid=i, rng=np.random.default_rng(910 + i), decorate=False)
    write_bam(str(tmp_path / "m.bam"), [(f"c{i}", s.pileup.L) for i, s in enumerate(syn)], sorted(recs, key=lambda r: (r["tid"], r["pos"])))
    with open(tmp_path / "g.fa", "w") as f:
        for i, s in enumerate(syn):
            f.write(f">c{i}\n{s.pileup.ref.tobytes().decode()}\n")
    np2io.write_yak(str(tmp_path / "k21.yak"), Synth.yak_assembly(syn, 21))
    cmd = [sys.executable, "-m", "nextpolish2_amd.cli", "-t", "2", "-L", "10000", str(tmp_path / "m.bam"), str(tmp_path / "g.fa"),
           str(tmp_path / "k21.yak")]
    plain = subprocess.run(cmd, capture_output=True, env=ENV, timeout=600)
    assert plain.returncode == 0, plain.stderr.decode()[-2000:]
    vcf = str(tmp_path / "e.vcf")
    r = subprocess.run(cmd + ["--edits", vcf], capture_output=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == plain.stdout and r.stdout.count(b">") == 2
    per = parse_vcf(vcf)
    n_recs = 0
    for rec in r.stdout.split(b">")[1:]:
        head, seq = rec.split(b"\n")[:2]
        name, first, last = head.split()[0].decode(), int(head.split()[1][6:]), int(head.split()[2][4:])
        ref = syn[int(name[1:])].pileup.ref.tobytes()
        assert apply_vcf(ref, per.get(name, []), first, last).upper() == seq.upper(), name
        n_recs += len(per.get(name, []))
    assert n_recs > 0  # (the generator's assembly errors are there to be corrected)
