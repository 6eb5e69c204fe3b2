"""The repetitive k-mers of an assembly, counted and selected on the GPU: the list `winnowmap -W` takes, which the
reference's recipe makes with `meryl count k=15` and `meryl print greater-than distinct=0.9998`.

    python -m nextpolish2_amd.repkmers asm.fa[.gz] [more.fa ...] [-k 15] [--distinct 0.9998 | --min_count N] [--both]
                                       [--stats FILE] [--device N] [-o FILE]

Every canonical k-mer (the lexicographically smaller of a k-mer and its reverse complement; ACGTU in either case, U read as
T, anything else ends a run of bases) gets an exact 32-bit count.  With D distinct k-mers, the threshold of --distinct f is
the smallest occurring count c for which at least (int)(f * D) distinct k-mers have a count <= c; --min_count N sets the
threshold to N instead.  Every k-mer counted MORE often than the threshold is written as "KMER<tab>COUNT", in ascending
ACGT order.  --both adds each k-mer's reverse complement on the next line (not for a k-mer that is its own).  The rule is
this project's, written on meryl's documented options (include/np2_io.h); it is not pinned against the meryl binary.

The helpers at the top need no device (kmer_text, kmer_index, revcomp_index, list_lines, stats_row); main() drives
api.rep_files."""
import argparse
import os
import shutil
import sys
import tempfile

STATS_HEADER = ("k", "kmers", "distinct", "threshold", "listed", "listed_occurrences", "max_count", "count_ms", "select_ms",
                "emit_ms")
K_MIN, K_MAX = 2, 16


def kmer_text(index, k):
    """index -> k upper-case letters: first base most significant, A=0 C=1 G=2 T=3"""
    index = int(index)
    return "".join("ACGT"[(index >> (2 * (k - 1 - i))) & 3] for i in range(k))


def kmer_index(text):
    """k letters (ACGTU, either case) -> index; the inverse of kmer_text"""
    v = 0
    for ch in text.upper():
        v = v << 2 | "ACGT".index("T" if ch == "U" else ch)
    return v


def revcomp_index(index, k):
    index, r = int(index), 0
    for _ in range(k):
        r = r << 2 | (3 - (index & 3))
        index >>= 2
    return r


def list_lines(index, count, k, both=False):
    """the list's lines, as np2_rep_files writes them"""
    out = []
    for v, c in zip(index, count):
        v, c = int(v), int(c)
        out.append("%s\t%d\n" % (kmer_text(v, k), c))
        rc = revcomp_index(v, k)
        if both and rc != v:
            out.append("%s\t%d\n" % (kmer_text(rc, k), c))
    return out


def stats_row(k, stats):
    """--stats: a header line and one TSV row of the stats dict (times in ms, three decimals)"""
    cells = [str(int(k))] + [str(int(stats[f])) for f in STATS_HEADER[1:7]] + ["%.3f" % float(stats[f]) for f in STATS_HEADER[7:]]
    return "\t".join(STATS_HEADER) + "\n" + "\t".join(cells) + "\n"


def build_parser():
    p = argparse.ArgumentParser(prog="nextpolish2_amd.repkmers",
                                description="list the repetitive k-mers of an assembly (the file winnowmap -W takes)")
    p.add_argument("fa", nargs="+", metavar="asm.fa[.gz]", help="assembly in [GZIP] FASTA format")
    p.add_argument("-k", type=int, default=15, metavar="K", help="k-mer size, 2 .. 16 [15]")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--distinct", type=float, default=0.9998, metavar="F",
                   help="list the k-mers counted more often than the fraction F of the distinct k-mers [0.9998]")
    g.add_argument("--min_count", type=int, default=None, metavar="N", help="list the k-mers counted more than N times instead")
    p.add_argument("--both", action="store_true", help="write each k-mer's reverse complement on the line after it")
    p.add_argument("--stats", default=None, metavar="FILE", help="one TSV row: k-mers, distinct, threshold, listed, times")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("-o", "--out", default=None, metavar="FILE", help="the list [stdout]")
    return p


def main(argv=None):
    from . import api
    a = build_parser().parse_args(argv)
    if a.min_count is not None and not 0 <= a.min_count <= 0xFFFFFFFF:
        raise SystemExit("Error: --min_count: 0 .. 4294967295")
    if not 0 <= a.k <= 0xFFFFFFFF:
        raise SystemExit(f"Error: k = {a.k}: the repetitive k-mer list is built for 2 <= k <= 16")
    tmp = None
    try:
        out = a.out
        if out is None:  # the library writes a file: a temporary one, copied to stdout
            fd, tmp = tempfile.mkstemp(prefix="repkmers.", suffix=".txt")
            os.close(fd)
            out = tmp
        try:
            stats = api.rep_files(a.fa, out, k=a.k, distinct=a.distinct, min_count=a.min_count, both=a.both, device=a.device)
        except (api.Np2Error, ImportError) as e:
            raise SystemExit(f"Error: {e}")
        if tmp is not None:
            with open(tmp, "r") as f:
                shutil.copyfileobj(f, sys.stdout)
            sys.stdout.flush()
        if a.stats is not None:
            with open(a.stats, "w") as f:
                f.write(stats_row(a.k, stats))
    finally:
        if tmp is not None and os.path.exists(tmp):
            os.remove(tmp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
