"""Switch and Hamming error of a diploid assembly against parental k-mer tables, measured on the GPU (what
`yak trioeval pat.yak mat.yak asm.fa` does after nextPolish2 in the reference's benchmarks).

    python -m nextpolish2_amd.trio asm.fa[.gz] pat.yak mat.yak [--min_count 2] [--mid_count 5] [--bed FILE] [-o FILE]
    python -m nextpolish2_amd.trio asm.fa[.gz] --pat_sr FILE... --mat_sr FILE... [--sr_k 21] [--sr_min_count 2] ...

A k-mer is a PATERNAL marker when the paternal table counts it at least --mid_count times and the maternal table fewer
than --min_count times, a MATERNAL marker the other way round (yak's -d / -c).  Per contig, over its markers in order:
pp, pm, mp, mm count the consecutive marker pairs as (earlier, later); switch = pm + mp and the switch rate is switch over
all pairs; hamming = min(pat, mat) and the Hamming rate is hamming over all markers.  The totals are the sums of the
integers over the contigs.  The semantics are this project's own: yak's report is not reproduced byte for byte.

The helpers at the top need no device (rate, rate_text, switch_sites, format_rows); TrioReport and main() drive
Polisher.trio_strings."""
import argparse
import math
import os
import sys

import numpy as np

STAT_NAMES = ("kmers", "pat", "mat", "pp", "pm", "mp", "mm", "switch", "switch_rate", "hamming", "hamming_rate")
TSV_HEADER = ("contig", "k", "len") + STAT_NAMES
CLI_HEADER = ("contig", "k") + tuple(f"{c}_{side}" for side in ("in", "out") for c in ("len",) + STAT_NAMES)
DEFAULT_MIN_COUNT, DEFAULT_MID_COUNT = 2, 5


def thresholds_ok(min_count, mid_count):
    return 1 <= min_count <= mid_count <= 1023


def rate(num, den):
    """num / den; nan when the denominator is 0"""
    return int(num) / int(den) if int(den) else math.nan


def rate_text(num, den):
    v = rate(num, den)
    return "nan" if math.isnan(v) else "%.6f" % v


def switch_of(stats):
    """(switches, pairs) of (kmers, pat, mat, pp, pm, mp, mm)"""
    return int(stats[4]) + int(stats[5]), sum(int(x) for x in stats[3:7])


def hamming_of(stats):
    """(hamming, markers)"""
    return min(int(stats[1]), int(stats[2])), int(stats[1]) + int(stats[2])


def switch_sites(pat_bits, mat_bits, length, k):
    """[(start, end, "pm" | "mp")], 0-based half-open: for every pair of consecutive markers of different parents with
    ends e0 < e1 (set bits of the two marker bitmaps of one sequence, least significant bit first), from the first base of
    the earlier marker to one past the last base of the later: (e0 - k + 1, e1 + 1)."""
    def ends(bits):
        return np.flatnonzero(np.unpackbits(np.ascontiguousarray(bits, dtype=np.uint8), bitorder="little")[:length]).astype(np.int64)
    p, m = ends(pat_bits), ends(mat_bits)
    e = np.concatenate([p, m])
    cls = np.concatenate([np.zeros(len(p), np.int8), np.ones(len(m), np.int8)])
    order = np.argsort(e, kind="stable")  # (no position is both parents' marker)
    e, cls = e[order], cls[order]
    at = np.flatnonzero(cls[1:] != cls[:-1])
    return [(int(e[i]) - k + 1, int(e[i + 1]) + 1, "pm" if cls[i] == 0 else "mp") for i in at]


def format_rows(rows):
    """rows of (contig, k, len, kmers, pat, mat, pp, pm, mp, mm[, len, kmers, ...]) -> TSV lines: switch, switch rate,
    hamming and Hamming rate after every eight integers"""
    out = []
    for r in rows:
        f = [str(r[0]), str(r[1])]
        for i in range(2, len(r), 8):
            st = [int(x) for x in r[i + 1:i + 8]]
            sw, pairs = switch_of(st)
            hm, markers = hamming_of(st)
            f += [str(int(r[i]))] + [str(x) for x in st] + [str(sw), rate_text(sw, pairs), str(hm), rate_text(hm, markers)]
        out.append("\t".join(f) + "\n")
    return out


class TrioReport:
    """Collects the trio statistics of named sequence sets ("in" / "out" on the command line) against tables `pat_idx` and
    `mat_idx` of a Polisher and writes the TSV and the switch-site BED files.  One context, one thread."""

    def __init__(self, k, min_count=DEFAULT_MIN_COUNT, mid_count=DEFAULT_MID_COUNT, want_bed=False, sides=("in", "out"),
                 pat_idx=0, mat_idx=1):
        self.k, self.min_count, self.mid_count, self.want_bed, self.sides = int(k), int(min_count), int(mid_count), want_bed, tuple(sides)
        self.pat_idx, self.mat_idx = pat_idx, mat_idx
        self.rows = []  # (contig, [per side: (len, kmers, pat, mat, pp, pm, mp, mm)])
        self.beds = {s: [] for s in self.sides}

    def add(self, pol, name, *seqs):
        """one contig: its sequence on every side (bytes)"""
        r = pol.trio_strings(self.pat_idx, self.mat_idx, seqs, self.min_count, self.mid_count, bits=self.want_bed)
        self.rows.append((name, [(len(s),) + tuple(int(x) for x in r.stats[i]) for i, s in enumerate(seqs)]))
        if self.want_bed:
            for i, side in enumerate(self.sides):
                self.beds[side] += [(name, a, b, kind) for a, b, kind in switch_sites(r.pat_bits[i], r.mat_bits[i], len(seqs[i]), self.k)]

    def lines(self, header):
        rows = [(name, self.k) + tuple(x for side in per for x in side) for name, per in self.rows]
        tot = np.zeros(8 * len(self.sides), dtype=np.int64)  # the totals: sums of the integers over the contigs
        for _, per in self.rows:
            tot += np.array([x for side in per for x in side], dtype=np.int64)
        rows.append(("total", self.k) + tuple(int(x) for x in tot))
        return ["\t".join(header) + "\n"] + format_rows(rows)

    def bed_text(self, side):
        return "".join("%s\t%d\t%d\t%s\n" % r for r in self.beds[side])

    def write_cli(self, tsv_path, bed_prefix=None):
        """the command line's --trio FILE and --trio_bed PREFIX (PREFIX.in.bed / PREFIX.out.bed)"""
        with open(tsv_path, "w") as f:
            f.writelines(self.lines(CLI_HEADER))
        if bed_prefix:
            for side in self.sides:
                with open(f"{bed_prefix}.{side}.bed", "w") as f:
                    f.write(self.bed_text(side))


def build_parser():
    p = argparse.ArgumentParser(prog="nextpolish2_amd.trio", description="switch and Hamming error of an assembly against parental k-mer tables")
    p.add_argument("fa", metavar="asm.fa[.gz]", help="assembly in [GZIP] FASTA format")
    p.add_argument("yak", nargs="*", metavar="parent.yak", help="the paternal and the maternal k-mer dump in yak format, in this order")
    p.add_argument("--pat_sr", action="append", nargs="+", default=[], metavar="FILE", help="paternal short reads: count their k-mers on the GPU instead")
    p.add_argument("--mat_sr", action="append", nargs="+", default=[], metavar="FILE", help="maternal short reads")
    p.add_argument("--sr_k", type=int, default=21, metavar="K", help="k-mer size counted from the reads [21]")
    p.add_argument("--sr_min_count", type=int, default=2, metavar="N", help="drop k-mers of the reads counted fewer than N times [2]")
    p.add_argument("--min_count", type=int, default=DEFAULT_MIN_COUNT, metavar="N", help="a parent counting a k-mer fewer than N times does not have it [2]")
    p.add_argument("--mid_count", type=int, default=DEFAULT_MID_COUNT, metavar="N", help="a parent counting a k-mer at least N times has it [5]")
    p.add_argument("--bed", default=None, metavar="FILE", help="switch sites: contig, start, end, pm|mp")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("-o", "--out", default=None, metavar="FILE", help="TSV [stdout]")
    return p


def parse_args(argv=None):
    """every argument error stops here, before a device is touched"""
    parser = build_parser()
    a = parser.parse_args(argv)
    a.pat_sr = [f for group in a.pat_sr for f in group]
    a.mat_sr = [f for group in a.mat_sr for f in group]
    if a.yak and (a.pat_sr or a.mat_sr):
        parser.error("give either pat.yak mat.yak or --pat_sr / --mat_sr reads, not both")
    if not a.yak and not (a.pat_sr and a.mat_sr):
        parser.error("give pat.yak mat.yak, or both --pat_sr and --mat_sr")
    if a.yak and len(a.yak) != 2:
        parser.error("exactly two dumps: pat.yak mat.yak")
    if not thresholds_ok(a.min_count, a.mid_count):
        parser.error("thresholds: 1 <= --min_count <= --mid_count <= 1023")
    if not 2 <= a.sr_k < 32:
        parser.error("--sr_k: only 2 <= k < 32 is supported")
    if a.sr_min_count < 1:
        parser.error("--sr_min_count: at least 1")
    return a


def parental_k(pat, mat):
    """k of two parental dumps; ValueError when they differ or a header is broken"""
    from . import io as np2io
    kp, km = np2io.check_yak_header(pat), np2io.check_yak_header(mat)
    if kp != km:
        raise ValueError(f"the parental dumps have different k: {pat} has k = {kp}, {mat} has k = {km}")
    return kp


def polisher_from_parental_reads(pat_sr, mat_sr, k, min_count=2, device=0):
    """a context with the paternal (index 0) and the maternal (index 1) table, each counted from its reads on the device"""
    from . import io as np2io
    from .api import Polisher
    yaks = [np2io.count_kmers(files, [k], min_count=min_count, device=device)[0] for files in (pat_sr, mat_sr)]
    return Polisher(yaks, device=device)


def main(argv=None):
    from . import io as np2io
    from .api import Np2Error
    a = parse_args(argv)
    try:
        if a.yak:
            try:
                k = parental_k(*a.yak)
            except (ValueError, OSError) as e:
                raise SystemExit(f"Error: {e}")
            pol = np2io.polisher_from_yak_files([os.path.abspath(y) for y in a.yak], device=a.device)
        else:
            k = a.sr_k
            pol = polisher_from_parental_reads(a.pat_sr, a.mat_sr, k, a.sr_min_count, a.device)
        rep = TrioReport(k, a.min_count, a.mid_count, want_bed=a.bed is not None, sides=("asm",))
        for name, seq in np2io.read_fasta(a.fa):
            rep.add(pol, name, seq)
        pol.close()
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    text = "".join(rep.lines(TSV_HEADER))
    if a.out is None:
        sys.stdout.write(text)
    else:
        with open(a.out, "w") as f:
            f.write(text)
    if a.bed is not None:
        with open(a.bed, "w") as f:
            f.write(rep.bed_text("asm"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
