"""Bin long reads by parental k-mers on the GPU (what `yak triobin pat.yak mat.yak reads.fa.gz` and the awk lines
behind it do in the reference's trio recipe: reads of the other haplotype are dropped before the mapping).

    python -m nextpolish2_amd.triobin pat.yak mat.yak reads.fa[.gz] ... [-o triobin.tsv] [--pat_list F] [--mat_list F]
          [--pat_fa F] [--mat_fa F] [--min_count 2] [--mid_count 5] [--min_score 2] [--max_minor 0.33]
    python -m nextpolish2_amd.triobin --pat_sr FILE... --mat_sr FILE... [--sr_k 21] [--sr_min_count 2] reads...

Markers are nextpolish2_amd.trio's: a k-mer is a PATERNAL marker when the paternal table counts it at least --mid_count
times and the maternal table fewer than --min_count times, a MATERNAL marker the other way round.  Per read, over its
markers in order, s_pat = pp and s_mat = mm count the markers that directly follow a marker of the same parent (an
isolated marker scores nothing).  The class is `0` when both scores are below --min_score; otherwise `a` (ambiguous) when
the scores are equal or the smaller one is more than --max_minor of the larger; otherwise `p` or `m`, the larger score.
The paternal bin keeps p, a and 0, the maternal bin m, a and 0.  The semantics are this project's own: yak's report is
not reproduced byte for byte.

An output named *.gz or *.bgz (the bins, the lists, the TSV) is written as BGZF, compressed on the device; any other name
as plain text.

TSV columns: read, class, s_pat, s_mat, n_pat, n_mat, pm, mp, kmers, len.  A summary per class goes to stderr.

The helpers at the top need no device (classify, keep, permille_of, parse_args); main() drives np2_bin_files."""
import argparse
import os
import sys

from .trio import DEFAULT_MID_COUNT, DEFAULT_MIN_COUNT, parental_k, polisher_from_parental_reads, thresholds_ok

TSV_HEADER = ("read", "class", "s_pat", "s_mat", "n_pat", "n_mat", "pm", "mp", "kmers", "len")
DEFAULT_MIN_SCORE, DEFAULT_MAX_MINOR = 2, 0.33
CLASSES = "pma0"


def permille_of(max_minor):
    """--max_minor as the integer the device compares with: thousandths, rounded"""
    return int(round(float(max_minor) * 1000))


def classify(s_pat, s_mat, min_score=DEFAULT_MIN_SCORE, minor_permille=330):
    """the class of a read from its two scores: integers only, as csrc/np2_bin_core.hpp has it"""
    s_pat, s_mat = int(s_pat), int(s_mat)
    if s_pat < min_score and s_mat < min_score:
        return "0"
    big, small = max(s_pat, s_mat), min(s_pat, s_mat)
    if s_pat == s_mat or small * 1000 > big * minor_permille:
        return "a"
    return "p" if s_pat > s_mat else "m"


def keep(cls, side):
    """the recipe's awk rule: the paternal bin ("pat") keeps p, a, 0; the maternal bin ("mat") keeps m, a, 0"""
    if side not in ("pat", "mat") or cls not in tuple(CLASSES):
        raise ValueError(f"keep({cls!r}, {side!r})")
    return cls != ("m" if side == "pat" else "p")


def build_parser():
    p = argparse.ArgumentParser(prog="nextpolish2_amd.triobin", description="bin long reads by parental k-mer tables")
    p.add_argument("inputs", nargs="*", metavar="FILE", help="pat.yak mat.yak reads.fa[.gz] ...; with --pat_sr / --mat_sr the read files only")
    p.add_argument("--pat_sr", action="append", nargs="+", default=[], metavar="FILE", help="paternal short reads: count their k-mers on the GPU instead")
    p.add_argument("--mat_sr", action="append", nargs="+", default=[], metavar="FILE", help="maternal short reads")
    p.add_argument("--sr_k", type=int, default=21, metavar="K", help="k-mer size counted from the short reads [21]")
    p.add_argument("--sr_min_count", type=int, default=2, metavar="N", help="drop k-mers of the short reads counted fewer than N times [2]")
    p.add_argument("--min_count", type=int, default=DEFAULT_MIN_COUNT, metavar="N", help="a parent counting a k-mer fewer than N times does not have it [2]")
    p.add_argument("--mid_count", type=int, default=DEFAULT_MID_COUNT, metavar="N", help="a parent counting a k-mer at least N times has it [5]")
    p.add_argument("--min_score", type=int, default=DEFAULT_MIN_SCORE, metavar="N", help="a read whose scores are both below N is class 0 [2]")
    p.add_argument("--max_minor", type=float, default=DEFAULT_MAX_MINOR, metavar="F", help="ambiguous when the smaller score is more than F of the larger [0.33]")
    p.add_argument("-o", "--out", default=None, metavar="FILE", help="TSV [stdout]")
    p.add_argument("--pat_list", default=None, metavar="FILE", help="names of the paternal bin (p, a, 0)")
    p.add_argument("--mat_list", default=None, metavar="FILE", help="names of the maternal bin (m, a, 0)")
    p.add_argument("--pat_fa", default=None, metavar="FILE", help="the paternal bin as FASTA; a name ending in .gz or .bgz is written as BGZF, compressed on the device")
    p.add_argument("--mat_fa", default=None, metavar="FILE", help="the maternal bin as FASTA (the same rule)")
    p.add_argument("--device", type=int, default=0)
    return p


def parse_args(argv=None):
    """every argument error stops here, before a device is touched"""
    parser = build_parser()
    a = parser.parse_intermixed_args(argv)  # (read files may stand behind the options, as in the usage above)
    a.pat_sr = [f for group in a.pat_sr for f in group]
    a.mat_sr = [f for group in a.mat_sr for f in group]
    if a.pat_sr or a.mat_sr:
        if not (a.pat_sr and a.mat_sr):
            parser.error("give pat.yak mat.yak, or both --pat_sr and --mat_sr")
        a.yak, a.reads = [], list(a.inputs)
    else:
        if len(a.inputs) < 2:
            parser.error("give pat.yak mat.yak before the read files, or both --pat_sr and --mat_sr")
        a.yak, a.reads = list(a.inputs[:2]), list(a.inputs[2:])
    if not a.reads:
        parser.error("no read file given")
    if not thresholds_ok(a.min_count, a.mid_count):
        parser.error("thresholds: 1 <= --min_count <= --mid_count <= 1023")
    if not 0 <= a.min_score < 2 ** 32:
        parser.error("--min_score: 0 <= N < 2^32")
    if not 0.0 <= a.max_minor <= 1.0:  # (nan fails both comparisons)
        parser.error("--max_minor: a fraction in [0, 1]")
    if not 2 <= a.sr_k < 32:
        parser.error("--sr_k: only 2 <= k < 32 is supported")
    if a.sr_min_count < 1:
        parser.error("--sr_min_count: at least 1")
    for f in a.yak + a.reads + a.pat_sr + a.mat_sr:
        if not os.path.isfile(f):
            parser.error(f"cannot open {f}")
    a.minor_permille = permille_of(a.max_minor)
    return a


def summary_text(counts):
    total = sum(counts.values())
    lines = ["class\treads\tfraction\n"]
    for c in CLASSES:
        lines.append("%s\t%d\t%s\n" % (c, counts[c], "%.6f" % (counts[c] / total) if total else "nan"))
    lines.append("paternal bin\t%d\nmaternal bin\t%d\n" % (total - counts["m"], total - counts["p"]))
    return "".join(lines)


def main(argv=None):
    import tempfile

    from . import io as np2io
    from .api import Np2Error
    a = parse_args(argv)
    try:
        if a.yak:
            try:
                parental_k(*a.yak)
            except (ValueError, OSError) as e:
                raise SystemExit(f"Error: {e}")
            pol = np2io.polisher_from_yak_files([os.path.abspath(y) for y in a.yak], device=a.device)
        else:
            pol = polisher_from_parental_reads(a.pat_sr, a.mat_sr, a.sr_k, a.sr_min_count, a.device)
        tmp = None
        tsv = a.out
        if tsv is None:  # the report is written natively: to a file of its own, then copied to standard output
            fd, tmp = tempfile.mkstemp(suffix=".triobin.tsv")
            os.close(fd)
            tsv = tmp
        try:
            counts, _ = np2io.bin_files(pol, a.reads, 0, 1, a.min_count, a.mid_count, a.min_score, a.minor_permille, tsv=tsv,
                                        pat_list=a.pat_list, mat_list=a.mat_list, pat_fa=a.pat_fa, mat_fa=a.mat_fa)
            if tmp is not None:
                with open(tmp, "rb") as f:
                    while True:
                        chunk = f.read(1 << 20)
                        if not chunk:
                            break
                        sys.stdout.buffer.write(chunk)
                sys.stdout.buffer.flush()
        finally:
            if tmp is not None:
                os.remove(tmp)
        pol.close()
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    sys.stderr.write(summary_text(counts))
    return 0


if __name__ == "__main__":
    sys.exit(main())
