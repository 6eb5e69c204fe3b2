"""Cases of the candidate kernels' tests (test_cand_cases_cpu.py, test_gpu_cand_edges.py): small pileups, each the smallest
shape at which one decision of k_region_measure / k_region_write (csrc/np2_cand.hip) can go wrong.  Those kernels take a
shortcut for a read without an exception record at [start, end + k + 2] of a region (its candidate is copied from the
contig), and only under a conjunction of conditions; every case straddles one of them: the last input taking the shortcut
and the first not taking it.  The expected answer is the CPU oracle's, stage by stage.

Every contig is a prefix of one homopolymer-free sequence B (an LQ region is its site plus padding: a lone SNP at p gives
[p - 3, p + 4], SNPs close enough to merge give [first - 3, last + 4]), so that all cases of one k share one k-mer table
and go through one batch.  A case states the regions it is built for; geometry() holds the oracle's lq.start / lq.end to
them, so a change of the region rule cannot silently move a case off its edge.

Boundaries the region rule cannot reach (main.rs line numbers as in oracle/np2_oracle.cpp's comments):
  * a region of 1 - 7 positions inside the shortcut.  A site lowers three consecutive consensus positions (the graph's
    nodes are 3-column-mers) and main.rs:1600-1611 pads them by 2 towards the contig's end and 3 towards its start: 8 at
    the least.  Shorter regions (3 - 7) exist only where the padding is cut at the contig's end (cases contig_end_short, _len4, _len7), and
    there end + k + 2 >= L: outside the shortcut, every pair decoded.  The residues mod 4 of the unaligned dword copy in
    k_region_write are therefore taken by the lengths 8, 9, 10, 11 (and 64).
  * a region whose end >> 10 exceeds the last tile: end is a contig position, end < L, so min(end >> 10, n_tiles - 1) never
    clamps.
  * a paired read that starts inside its region (t0 = max(start, aln_t_s) > start): main.rs:1445-1476 pairs a read only with
    regions whose start >= aln_t_s, and slices align_bases[start - aln_t_s ..].  Reads that start inside or behind the
    region sit in the tile's read list unpaired (case read_starts): they shift lanes, never strings.

Bounds of the shortcut that are wider than any input can tell (the cases sit on them all the same; moving one by a position
changes which pairs are decoded, never a result):
  * ends_inside, aln_t_e < end + k.  A lent candidate needs the read over [start, end] for the string and over
    [start, start + k - 1] for the first k-mer; pairing gives aln_t_e >= end, and end >= start + 7 inside the shortcut, so
    aln_t_e >= end + k - 1 would do as well (read_ends has both reads).
  * the window's first position, record at pos >= start.  A difference files records at its column and the two behind it,
    so one that touches the candidate (t_pos >= start) always has a record at t_pos > start as well, in the same tile;
    records at start alone come from differences at start - 2, which touch nothing (records, offsets -3 .. 0).
  * the window's last positions and the letter mask behind `end`.  The string needs the contig's letters at [start, end]
    only; the first k-mer of a lent candidate is the one decoded from the contig's own row, whose columns a read without
    records shares whatever the letters are.  Differences behind start + k (one more behind a deletion) change nothing:
    the records at end + k + 1 and end + k + 2 and an N at end + k only send pairs to the decoder (records, non_acgt)."""
import functools

import numpy as np

from nextpolish2_amd import Opts
from nextpolish2_amd._types import Pileup
from nextpolish2_amd.synth import pileup_from_alignments
from oracle import np2_oracle as orc
from test_oracle_pinning import backbone, other, yak_counted

TILE = 1024
B = backbone(9000, 77)


@functools.lru_cache(maxsize=None)
def yak(k):
    """the one table of every haploid case of this k: the k-mers of B, count 50 (a candidate carrying another allele scores 0)"""
    return yak_counted([(B, 50)], k)


def alt(p):
    """the other allele of a site: no new homopolymer next to it"""
    return other(B[p], skip=(B[p - 1], B[p + 1]))


def ins(p):
    """a letter to insert behind p"""
    return other(B[p], skip=(B[p + 1],))


def snp_region(first, last=None):
    """the region of SNP sites first..last that merge (close enough: at most 7 apart)"""
    return first - 3, (first if last is None else last) + 4


class Build:
    """a contig (B[:L], letters overridden by `ref`) and its reads in read-index order"""

    def __init__(self, L, ref=None):
        self.L, self.ref = L, ref or B[:L]
        assert len(self.ref) == L
        self.alns, self.dropped = [], []

    def add(self, s, e, edits=(), n=1, dropped=False):
        """n reads over [s, e] carrying the contig's letters but for edits: (p, 'X', base) a mismatch, (p, 'D') the base
        deleted, (p, 'I', letters) letters inserted behind p.  -> index of the first one"""
        ed = {}
        for p, kind, *arg in edits:
            assert s <= p <= e
            ed.setdefault(p, []).append((kind, arg[0] if arg else None))
        t, q = [], []
        for p in range(s, e + 1):
            here = dict(ed.get(p, ()))
            t.append(self.ref[p])
            q.append("-" if "D" in here else here.get("X", self.ref[p]))
            if "I" in here:
                t.append("-" * len(here["I"]))
                q.append(here["I"])
        first = 1 + len(self.alns)
        for _ in range(n):
            self.dropped.append(dropped)
            self.alns.append((s, "".join(t), "".join(q)))
        return first

    def snps(self, sites, s=0, e=None, n=1):
        return self.add(s, self.L - 1 if e is None else e, [(p, "X", alt(p)) for p in sites if s <= p <= (self.L - 1 if e is None else e)], n)

    def pileup(self):
        pu = pileup_from_alignments(self.ref, self.alns)
        if any(self.dropped):
            reads = pu.reads.copy()
            reads["flags"][1:][np.array(self.dropped)] = 1  # align_bases == [] but the index retained (main.rs:571)
            pu = Pileup(pu.ref, reads, pu.nibbles)
        return pu


def done(b, k, regions, opts=None, yaks=None, later=()):
    """regions: those of pass 0; later: those of the passes after it"""
    alns = [(0, b.ref, b.ref)] + b.alns  # by read index, for the restatement of the emission rule
    return b.pileup(), yaks or [yak(k)], opts or Opts(iter_count=1), regions and [sorted(regions)] + [sorted(r) for r in later], alns


def plain(L, sites, n_clean=9, n_alt=3, ref=None):
    """n_clean reads equal to the contig and n_alt carrying every site's other allele, all over the whole contig, the two
    kinds interleaved"""
    b = Build(L, ref)
    b.add(0, L - 1, n=n_clean - n_clean // 2)
    b.snps(sites, n=n_alt)
    b.add(0, L - 1, n=n_clean // 2)
    return b


# ---- the region and its window --------------------------------------------------------------------------------------------------
def _region_len(k=21):
    """CLEAN_MAX_LEN: lengths 8, 9, 10, 11 (every residue mod 4 of the dword copy), 64 (the last inside) and 65 (the first outside)"""
    groups = [[300], [1324, 1325], [2348, 2350], [3372, 3375], [4396 + 7 * i for i in range(9)], [5420 + d for d in (0, 7, 14, 21, 28, 35, 42, 47, 52, 57)]]
    regions = [snp_region(g[0], g[-1]) for g in groups]
    assert [e - s + 1 for s, e in regions] == [8, 9, 10, 11, 64, 65]
    assert all(s >> 10 == (e + k + 2) >> 10 for s, e in regions)  # nothing else keeps a region out of the shortcut
    return done(plain(6400, [p for g in groups for p in g]), k, regions)


def _tile_border(k):
    """the window's last position end + k + 2 at 1023 (inside the tile; the last group of 16 of the record index: j1 == 64 takes
    tile_n) and at 2048 (outside); a region that starts in tile 2 and ends in tile 3 (the tile is chosen by its end); a region
    whose window and first k-mer reach into tile 4.  Single-difference reads sit where only the right records make them dirty:
    the last base of the first k-mer in the window's last group of 16, and first-k-mer bases behind the tile border."""
    e0, e1 = 1023 - k - 2, 2048 - k - 2
    p2, p3 = 3 * TILE - 1, 4 * TILE - 11
    sites = [e0 - 4, e1 - 4, p2, p3]
    regions = [snp_region(p) for p in sites]
    assert regions[0][1] + k + 2 == 1023 and regions[1][1] + k + 2 == 2048
    assert regions[2][0] >> 10 == 2 and regions[2][1] >> 10 == 3
    s3, en3 = regions[3]
    assert en3 >> 10 == 3 and (en3 + k + 2) >> 10 == 4 and s3 + k - 1 >= 4 * TILE + 2
    L = 5200
    b = Build(L)  # 64 rows: the most the shortcut takes, and three rows differing in one column stay above the 95 % that start a region
    b.add(0, L - 1, n=24)
    b.snps(sites, n=5)
    s0 = regions[0][0]
    km_last = s0 + k - 1  # the last base of region 0's first k-mer
    assert km_last == 1013  # (whatever k: start = 1023 - k - 2 - 7)
    for p in (km_last, km_last - 1, 1023 - 2, 1023):
        b.add(0, L - 1, [(p, "X", alt(p))])
    b.add(0, L - 1, [(km_last, "D")])
    for p in (4 * TILE, s3 + k - 1):  # region 3: first-k-mer bases in the next tile
        b.add(0, L - 1, [(p, "X", alt(p))])
    b.add(0, L - 1, [(4 * TILE, "D")])
    b.add(0, L - 1, [(4 * TILE + 5, "I", ins(4 * TILE + 5))])
    b.add(0, L - 1, [(regions[1][1] + k, "X", alt(regions[1][1] + k))])
    b.add(0, L - 1, n=64 - 2 - len(b.alns))
    b.add(0, L - 1, [(regions[2][0] + k - 1, "X", alt(regions[2][0] + k - 1))])
    assert 1 + len(b.alns) == 64
    return done(b, k, regions)


def _contig_end(delta, k=21):
    """we < L: end + k + 2 == L - 1 (delta 0: the last window inside the contig) and == L (delta 1)"""
    L = 1500
    en = L - 1 - k - 2 + delta
    regions = [snp_region(en - 4)]
    assert regions[0][1] + k + 2 == L - 1 + delta
    b = plain(L, [en - 4], n_clean=22)
    b.add(0, L - 1, [(L - 2, "X", alt(L - 2))])  # a difference in the window's last positions
    b.add(0, L - 1, [(regions[0][0] + k - 1, "X", alt(regions[0][0] + k - 1))])
    return done(b, k, regions)


def _contig_end_short(k=21):
    """a site at the contig's last position: the padding is cut at the end (main.rs:1600-1611: lq_s - 2, not past 1) and the region is
    [L - 4, L - 2], three long; next to it a region whose window ends at L - 1 exactly"""
    L = 1200
    regions = [snp_region(L - 1 - k - 2 - 4), (L - 4, L - 2)]
    return done(plain(L, [L - 1 - k - 2 - 4, L - 1]), k, regions)


def _contig_end_short_n(back, k=21):
    """a site `back` positions before the last: a region of 3 + back positions ending at L - 2 (outside the shortcut: we >= L)"""
    L = 1200
    p = L - 1 - back
    return done(plain(L, [p]), k, [(p - 3, L - 2)])


def _record_index(k=21):
    """k_tile_sort's index of every 16th position: start - tile_start = 15, 16, 17 (tiles 0, 1, 2); the tile's only other record
    well before the window (tile 0), inside it (tile 1) and well behind it (tile 2)"""
    sites = [15 + 3, TILE + 16 + 3, 2 * TILE + 17 + 3]
    regions = [snp_region(p) for p in sites]
    assert [s - (s >> 10 << 10) for s, _ in regions] == [15, 16, 17]
    L = 3300
    b = plain(L, sites, n_clean=20)
    b.add(0, L - 1, [(3, "X", alt(3))])
    b.add(0, L - 1, [(TILE + 16 + 8, "X", alt(TILE + 16 + 8))])
    b.add(0, L - 1, [(2 * TILE + 900, "X", alt(2 * TILE + 900))])
    b.add(0, L - 1, n=3)
    return done(b, k, regions)


def _non_acgt(k=21):
    """the contig's own letters at [start, end + k] must be A/C/G/T for its string to be lent: N at start with start & 7 in
    {0, 7}, at start - 1 (outside the mask: the word before, and the same word), at end + k with (end + k) & 7 in {0, 7}, at
    end + k + 1 (outside: the next word, and the same word), in the middle, and a lower-case stretch over a whole window.  The
    reads carry the contig's letters, N included: no exception record marks them, only the letter mask stops the shortcut."""
    want = []  # (site, position of the N relative to the region: ("s", d) start + d, ("e", d) end + k + d)
    p = 100
    plan = [("s", 0, lambda s, e: s & 7 == 0), ("s", 0, lambda s, e: s & 7 == 7), ("s", -1, lambda s, e: s & 7 == 0),
            ("s", -1, lambda s, e: s & 7 == 3), ("e", 0, lambda s, e: (e + k) & 7 == 0), ("e", 0, lambda s, e: (e + k) & 7 == 7),
            ("e", 1, lambda s, e: (e + k) & 7 == 7), ("e", 1, lambda s, e: (e + k) & 7 == 2), ("s", 4, lambda s, e: True)]
    ref = list(B[:2600])
    sites, regions = [], []
    for side, d, ok in plan:
        while not ok(*snp_region(p)):
            p += 1
        s, e = snp_region(p)
        ref[s + d if side == "s" else e + k + d] = "N"
        sites.append(p)
        regions.append((s, e))
        p += 90
    assert p < 1000
    s, e = snp_region(1500)  # lower case: upper-cased on the way in, the shortcut stays
    ref[s - 5:e + k + 5] = "".join(ref[s - 5:e + k + 5]).lower()
    sites.append(1500)
    regions.append((s, e))
    # 30 reads: the contig's own row differs from the others nowhere, but keep any single row under 5 % all the same
    return done(plain(2600, sites, n_clean=26, n_alt=4, ref="".join(ref)), k, regions)


def _bucket(k=21):
    """tn <= bucket_cap: a mismatch files three records (its column and the two behind it), two adjacent ones four.  Tile 0 holds
    4 x 3 = 12 records, tile 1 3 x 3 + 4 = 13 (test_cand_cases_cpu.py counts them in the oracle's graph).  A contig with a
    tile over its bucket takes the device-wide sort, which leaves no record index (run_diff, np2_polish.cpp): under
    NP2_TILE_CAP = 13 both regions take the shortcut, under 12 tile 1 spills and neither does — the kernel's own test of
    tile_n restates that tile by tile.  The device test runs the caps 11 .. 14."""
    L = 2100
    sites = [500, TILE + 500]
    b = Build(L)
    b.add(0, L - 1, n=12)  # (28 reads: one read's difference alone stays above the 95 % that start a region)
    b.snps(sites, n=3)
    b.add(0, L - 1, [(500, "X", alt(500)), (TILE + 700, "X", alt(TILE + 700)), (TILE + 701, "X", alt(TILE + 701))])
    b.add(0, L - 1, n=12)
    return done(b, k, [snp_region(p) for p in sites])


BUCKET_CAPS = (11, 12, 13, 14)


# ---- the reads of a region ------------------------------------------------------------------------------------------------------
def _records(k=17):
    """A single mismatch (tile 0), a single deleted base (tile 1), a single inserted base behind it (tile 2) at every position of
    [start - 3, end + k + 3], one read each; the other reads equal the contig but for three that carry the sites.  A
    difference at p files records at p, p + 1, p + 2: the series shows which of them must make a read dirty (those that
    change the string, [start, end], or the first k-mer, [start, start + k - 1] and one base more behind a deletion) and
    which must not.  Three regions a tile share the sweep, positions 0, 1, 2 mod 3 from start - 3 on, and a read carries one
    difference in each: no column sees two differing rows, so no region arises but at the sites."""
    L = 3 * TILE
    sites = [t * TILE + at for t in range(3) for at in (200, 500, 800)]
    b = Build(L)
    for t, kind in enumerate("XDI"):
        lo, hi = t * TILE + 20, t * TILE + 1000
        mine = sites[3 * t:3 * t + 3]
        b.add(lo, hi, n=5)
        b.snps(mine, lo, hi, n=3)
        for d in range(-3, 8 + k + 3 + 1, 3):
            at = [snp_region(p)[0] + d + j for j, p in enumerate(mine)]
            b.add(lo, hi, [(p, "X", alt(p)) if kind == "X" else (p, "D") if kind == "D" else (p, "I", ins(p)) for p in at])
        b.add(lo, hi, n=5)
    return done(b, k, [snp_region(p) for p in sites])


def _many_records(k=21):
    """more than 64 records inside one window (the second loop of `mark`): three paired reads with 30 letters inserted behind the
    site (32 records each), one unpaired read (it ends inside the region) with the same, and a paired read whose only record
    group lies beyond the first 64"""
    L, p = 1400, 600
    letters = "".join("ACGT"[(i * 7 + i // 4) % 4] for i in range(30))
    b = Build(L)
    b.add(0, L - 1, n=5)
    b.add(0, L - 1, [(p, "I", letters)], n=3)
    b.add(0, p + 1, [(p, "I", letters)])             # ends inside the region: not paired
    b.add(0, L - 1, [(p + 6, "X", alt(p + 6))])      # its records sort behind the 128 of position p .. p + 2
    b.add(0, L - 1, n=5)
    return done(b, k, None)  # (the region of an insertion site: whatever the rule gives, held to the window conditions in geometry())


def _read_ends(k=21):
    """ends_inside: reads ending at end - 1 (not paired), end, end + 1, start + k - 2 (the first k-mer is one base short),
    start + k - 1, end + k - 1 (the last dirty one), end + k (the first clean one), end + k + 2, between reads over the whole contig"""
    L, p = 1400, 700
    s, e = snp_region(p)
    b = Build(L)
    b.add(0, L - 1, n=3)
    for te in (e - 1, e, e + 1, s + k - 2, s + k - 1, e + k - 1, e + k, e + k + 2):
        b.add(0, te)
        b.add(0, L - 1)
    b.snps([p], n=4)
    b.snps([p], e=e + k - 1)
    b.snps([p], e=e + k)
    b.add(0, L - 1, n=3)
    return done(b, k, [(s, e)])


def _read_starts(k=21):
    """reads starting at start - 1 and start (paired, the whole string), at start + 1, inside, at end and behind end (in the
    tile's read list, not paired: main.rs:1445-1476), before and between the kept reads: the kept ones are ranked by
    lanes_below over a list with holes.  One region, so the reference's region cursor comes back for the later reads."""
    L, p = 1400, 700
    s, e = snp_region(p)
    b = Build(L)
    b.add(e + 2, L - 1)
    b.add(s + 4, L - 1)
    b.add(0, L - 1, n=16)  # (enough rows that the odd first columns of the reads starting here start no region of their own)
    for ts in (s - 1, s, s + 1, e, e + 1, e + 30):
        b.add(ts, L - 1)
        b.add(0, L - 1)
    b.snps([p], n=4)
    b.snps([p], s=s - 2)
    b.snps([p], s=s + 2)
    b.add(0, L - 1, n=16)
    return done(b, k, [(s, e)])


def _read_list(rows, k=21):
    """nlist <= 64: `rows` reads over the region's tile, the contig's own row, four dropped reads (flags = 1) and five unpaired
    ones (they overlap the tile, not the region) among them"""
    L, p = 1400, 700
    b = Build(L)
    b.add(0, L - 1, n=10)
    b.add(0, L - 1, n=2, dropped=True)
    b.add(0, 400, n=3)
    b.snps([p], n=6)
    b.add(0, L - 1, n=2, dropped=True)
    b.add(900, L - 1, n=2)
    b.add(0, L - 1, n=rows - 1 - len(b.alns))
    assert 1 + len(b.alns) == rows
    return done(b, k, [snp_region(p)])


def _kept(paired, rows, k=21):
    """the first 60 non-empty candidates are kept: `paired` rows give one each (the contig's among them), `rows` rows lie over the
    tile; reads carrying the site, which have to be decoded, lie among the first 60 and beyond them"""
    L, p = 1400, 700
    b = Build(L)
    dirty = {5, 6, 7, 30, 57, 58, 59, 60, 62}  # which of the paired reads carry the site
    for r in range(1, paired):
        b.snps([p]) if r in dirty else b.add(0, L - 1)
        if r in (10, 40) and 1 + len(b.alns) + (paired - 1 - r) < rows:
            b.add(0, 300)  # unpaired rows inside the list
    b.add(0, 300, n=rows - 1 - len(b.alns))
    assert 1 + len(b.alns) == rows
    return done(b, k, [snp_region(p)])


# ---- the set of regions ---------------------------------------------------------------------------------------------------------
def _counts(n, k=21):
    """n regions in one contig: four per wavefront, 16 per block, blk_sum by groups of four, the closing cand_seq_off entry
    written by the last region's lane.  The second region from the right straddles the tile border (outside the shortcut), the
    others are inside it."""
    L = 1500
    sites = ([1100] + [1023 - 60 * j for j in range(16)])[:n]
    regions = [snp_region(p) for p in sites]
    if n > 1:
        assert regions[1][0] >> 10 == 0 and regions[1][1] >> 10 == 1
    return done(plain(L, sites), k, regions)


# ---- the phasing pass -----------------------------------------------------------------------------------------------------------
def _phasing(k=21):
    """a diploid input under the default options: a phasing pass, then the final pass.  Two haplotypes ten reads each, four
    sites; one region's window ends at 1023, one straddles tiles 1 / 2; two reads carry an error of their own next to a site."""
    L = 2600
    e0 = 1023 - k - 2
    sites = [400, e0 - 4, 2 * TILE - 1, 2300]
    regions = [snp_region(p) for p in sites]
    assert regions[1][1] + k + 2 == 1023 and regions[2][0] >> 10 == 1 and regions[2][1] >> 10 == 2
    h1 = B[:L]
    for p in sites:
        h1 = h1[:p] + alt(p) + h1[p + 1:]
    b = Build(L)
    for i in range(10):
        b.add(0, L - 1)
        b.snps(sites)
    b.add(0, L - 1, [(sites[1] + 10, "X", alt(sites[1] + 10))])
    b.snps(sites + [405])
    return done(b, k, regions, Opts(), [yak_counted([(h1, 30), (B[:L], 30)], k)], later=[[snp_region(sites[1] + 10)]])


BUILDERS = {
    "region_len": _region_len,
    "tile_border_k17": lambda: _tile_border(17),
    "tile_border_k21": lambda: _tile_border(21),
    "tile_border_k31": lambda: _tile_border(31),  # the largest k a Polisher takes (main.rs:1433-1434: k < 32)
    "contig_end_in": lambda: _contig_end(0),
    "contig_end_out": lambda: _contig_end(1),
    "contig_end_k31": lambda: _contig_end(0, 31),
    "contig_end_short": _contig_end_short,
    "contig_end_len4": lambda: _contig_end_short_n(1),
    "contig_end_len7": lambda: _contig_end_short_n(4),
    "record_index": _record_index,
    "non_acgt": _non_acgt,
    "bucket": _bucket,
    "records": _records,
    "many_records": _many_records,
    "read_ends": _read_ends,
    "read_starts": _read_starts,
    "read_list_64": lambda: _read_list(64),
    "read_list_65": lambda: _read_list(65),
    "kept_60": lambda: _kept(60, 64),
    "kept_61": lambda: _kept(61, 64),
    "kept_64": lambda: _kept(64, 64),
    "kept_61_list_70": lambda: _kept(61, 70),
    "counts_1": lambda: _counts(1),
    "counts_3": lambda: _counts(3),
    "counts_4": lambda: _counts(4),
    "counts_5": lambda: _counts(5),
    "counts_15": lambda: _counts(15),
    "counts_16": lambda: _counts(16),
    "counts_17": lambda: _counts(17),
    "phasing": _phasing,
}
_BUILT = {name: fn() for name, fn in BUILDERS.items()}
CASES = {name: c[:3] for name, c in _BUILT.items()}
REGIONS = {name: c[3] for name, c in _BUILT.items()}  # the regions a case is built for, by pass, ascending (None: see geometry())
ALNS = {name: c[4] for name, c in _BUILT.items()}     # [(aln_t_s, gapped target, gapped query)] by read index
POISONED = [n for n in CASES if n.startswith(("kept_", "read_list_"))]  # the cases run on poisoned memory


@functools.lru_cache(maxsize=None)
def expected(name):
    """the traced oracle's (oracle, bases, positions) of a case, computed once; None where the reference panics"""
    pu, yaks, opts = CASES[name]
    o = orc.Oracle(yaks)
    o.set_trace(True)
    try:
        ob, op = o.polish(pu, opts)
    except orc.RefPanic:
        return None
    return o, ob, op


def geometry(name):
    """the oracle's regions (of every pass) are the ones the case is built for"""
    ref = expected(name)
    assert ref is not None, "no case here is built to make the reference panic"
    pu, yaks, opts = CASES[name]
    k = yaks[0].k
    for ps in range(opts.iter_count):
        got = sorted(zip(ref[0].trace(ps, "lq.start").tolist(), ref[0].trace(ps, "lq.end").tolist()))
        if REGIONS[name] is not None:
            assert got == REGIONS[name][ps], (name, ps, got, REGIONS[name][ps])
        else:  # many_records: one region over the site, inside the shortcut's conditions
            (s, e), = got
            assert s <= 600 <= e and e - s + 1 <= 64 and s >> 10 == (e + k + 2) >> 10 and e + k + 2 < len(pu.ref), got
