"""K-mer QV of an assembly against short-read k-mer tables, measured on the GPU (what `yak qv` / Merqury do after
nextPolish2 in the reference's benchmarks).

    python -m nextpolish2_amd.qv asm.fa[.gz] k21.yak [k31.yak ...] [--qv_min_count N] [--bed FILE] [--hist FILE] [-o FILE]
    python -m nextpolish2_amd.qv asm.fa[.gz] --sr reads.fq.gz [--sr ...] [--sr_k 21,31] [--sr_min_count 2] ...

Every position's canonical k-mer counts (with multiplicity); a k-mer is ABSENT when the table's count for it, with counts
below --qv_min_count read as 0, is 0.  Tables counted with a threshold of their own (--sr_min_count 2, `yak count -b 37`)
hold no singletons: a k-mer the reads show once is absent by construction.  QV is Merqury's:
P = 1 - absent / k-mers, E = 1 - P^(1/k), QV = -10 log10(E).

The helpers at the top need no device (qv_value, bed_intervals, format_rows); QvReport and main() drive
Polisher.qv_strings."""
import argparse
import math
import sys

import numpy as np

TSV_HEADER = ("contig", "k", "len", "kmers", "absent", "qv")
CLI_HEADER = ("contig", "k", "len_in", "kmers_in", "absent_in", "qv_in", "len_out", "kmers_out", "absent_out", "qv_out")


def qv_value(n_kmers, n_absent, k):
    """Merqury's QV.  No k-mers: nan; no absent k-mer: inf."""
    n_kmers, n_absent = int(n_kmers), int(n_absent)
    if n_kmers == 0:
        return math.nan
    if n_absent == 0:
        return math.inf
    if n_absent >= n_kmers:
        return 0.0
    # E = 1 - P^(1/k) without the cancellation of 1 - (something close to 1)
    e = -math.expm1(math.log1p(-n_absent / n_kmers) / k)
    return -10.0 * math.log10(e)


def qv_text(n_kmers, n_absent, k):
    v = qv_value(n_kmers, n_absent, k)
    return "nan" if math.isnan(v) else "inf" if math.isinf(v) else "%.4f" % v


def bed_intervals(bits, length, k):
    """[(start, end)], 0-based half-open: the union of [e - k + 1, e + 1) over the set bits e < length of a sequence's
    absent bitmap (least significant bit first), overlapping or touching intervals merged."""
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    e = np.flatnonzero(np.unpackbits(bits, bitorder="little")[:length]).astype(np.int64)
    if e.size == 0:
        return []
    first = np.concatenate([[True], np.diff(e) > k])  # a new interval starts where start > previous end: e - k + 1 > e' + 1
    last = np.concatenate([first[1:], [True]])
    return [(max(0, int(a) - k + 1), int(b) + 1) for a, b in zip(e[first], e[last])]


def format_rows(rows):
    """rows of (contig, k, len, kmers, absent[, len, kmers, absent ...]) -> TSV lines, a QV after every (len, kmers, absent)"""
    out = []
    for r in rows:
        f = [str(r[0]), str(r[1])]
        for i in range(2, len(r), 3):
            f += [str(int(r[i])), str(int(r[i + 1])), str(int(r[i + 2])), qv_text(r[i + 1], r[i + 2], r[1])]
        out.append("\t".join(f) + "\n")
    return out


class QvReport:
    """Collects, per table of a Polisher, the k-mer statistics of named sequence sets ("in" / "out" on the command line)
    and writes the TSV and the BED files.  One context, one thread."""

    def __init__(self, ks, min_count=1, want_bed=False, sides=("in", "out"), want_hist=False):
        self.ks, self.min_count, self.want_bed, self.sides = list(ks), int(min_count), want_bed, tuple(sides)
        self.rows = []  # (contig, [per table: [per side: (len, kmers, absent)]])
        self.beds = {(t, s): [] for t in range(len(self.ks)) for s in self.sides}
        self.hists = [np.zeros(1024, np.uint64) for _ in self.ks] if want_hist else None

    def add(self, pol, name, *seqs):
        """one contig: its sequence on every side (bytes), measured against every table of `pol`"""
        per_table = []
        for t, k in enumerate(self.ks):
            r = pol.qv_strings(t, seqs, self.min_count, hist=self.hists is not None, bits=self.want_bed)
            per_table.append([(len(s), int(r.stats[i, 0]), int(r.stats[i, 1])) for i, s in enumerate(seqs)])
            if self.hists is not None:
                self.hists[t] += r.hist
            if self.want_bed:
                for i, side in enumerate(self.sides):
                    self.beds[(t, side)] += [(name, a, b) for a, b in bed_intervals(r.bits[i], len(seqs[i]), k)]
        self.rows.append((name, per_table))

    def lines(self, header):
        rows = [(name, k) + tuple(x for side in per[t] for x in side) for name, per in self.rows for t, k in enumerate(self.ks)]
        for t, k in enumerate(self.ks):  # the totals: sums over the contigs, per table
            tot = np.zeros(3 * len(self.sides), dtype=np.int64)
            for _, per in self.rows:
                tot += np.array([x for side in per[t] for x in side], dtype=np.int64)
            rows.append(("total", k) + tuple(int(x) for x in tot))
        return ["\t".join(header) + "\n"] + format_rows(rows)

    def bed_text(self, t, side):
        return "".join("%s\t%d\t%d\n" % r for r in self.beds[(t, side)])

    def write_cli(self, tsv_path, bed_prefix=None):
        """the command line's --qv FILE and --qv_bed PREFIX (PREFIX.k<K>.in.bed / PREFIX.k<K>.out.bed)"""
        with open(tsv_path, "w") as f:
            f.writelines(self.lines(CLI_HEADER))
        if bed_prefix:
            for t, k in enumerate(self.ks):
                for side in self.sides:
                    with open(f"{bed_prefix}.k{k}.{side}.bed", "w") as f:
                        f.write(self.bed_text(t, side))


def build_parser():
    from . import io as np2io
    p = argparse.ArgumentParser(prog="nextpolish2_amd.qv", description="k-mer QV of an assembly against short-read k-mer tables")
    p.add_argument("fa", metavar="asm.fa[.gz]", help="assembly in [GZIP] FASTA format")
    np2io.add_table_args(p)
    p.add_argument("--qv_min_count", type=int, default=1, metavar="N", help="read a count below N as absent [1]")
    p.add_argument("--bed", default=None, metavar="FILE", help="intervals covered by absent k-mers (FILE.k<K> per table when there are several)")
    p.add_argument("--hist", default=None, metavar="FILE", help="count histogram: k, count, k-mers")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("-o", "--out", default=None, metavar="FILE", help="TSV [stdout]")
    return p


def main(argv=None):
    from . import io as np2io
    from .api import Np2Error
    parser = build_parser()
    a = parser.parse_args(argv)
    if bool(a.sr) == bool(a.yak):
        parser.error("give either k.yak dumps or --sr reads")
    if not 0 <= a.qv_min_count <= 1023:
        parser.error("--qv_min_count: 0 .. 1023")
    try:
        pol, ks = np2io.open_tables(parser, a)
        rep = QvReport(ks, a.qv_min_count, want_bed=a.bed is not None, sides=("asm",), want_hist=a.hist is not None)
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
        for t, k in enumerate(ks):
            with open(a.bed if len(ks) == 1 else f"{a.bed}.k{k}", "w") as f:
                f.write(rep.bed_text(t, "asm"))
    if a.hist is not None:
        with open(a.hist, "w") as f:
            f.write("k\tcount\tkmers\n")
            for t, k in enumerate(ks):
                f.writelines(f"{k}\t{c}\t{int(n)}\n" for c, n in enumerate(rep.hists[t]) if n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
