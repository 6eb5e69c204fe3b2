"""Cut the stretches of low mapping depth out of an assembly, on the GPU (what the reference's
`other/remove_low_depth_in_fasta.py` does with pysam, one base at a time: NextPolish2 can only correct the regions that are
mapped by HiFi reads, and this tells a user which regions those are).

    python -m nextpolish2_amd.lowdepth reads.map.sort.bam genome.fa[.gz] > genome.filter.fa
          [-d 3] [-l 1000] [--min_fra 0.8] [--min_mapq 0] [--exclude_flags 4] [--bed F] [--low_bed F] [--bedgraph F] [-o F]

The mapping is a coordinate-sorted, indexed BAM; from the mapper's SAM text `python -m nextpolish2_amd.samsort` writes one.

-o F writes the FASTA to F instead of standard output; an F ending in .gz or .bgz is written as BGZF, compressed on the device.

Depth counts alignment records (include/np2_io.h, np2_depth_*): a record is counted unless one of its flag bits is in
--exclude_flags, its mapping quality is below --min_mapq, it has no CIGAR, or its aligned query bases (M I = X) are less
than --min_fra of its read length (M I S H = X); it covers its reference span (M D N = X), clamped to the contig.  A run is a
maximal stretch of depth >= --min_depth; runs of at least --min_len positions are kept.

For every contig of the FASTA, in input order, and every kept run [s, e] (0-based, inclusive) standard output receives
    >{name}_{s}_{e}
    {the contig's bases s .. e, in upper case}
(name: the header up to the first whitespace) and standard error `output rate in {name}: {percent}%`.

One difference from the reference's names, on purpose: its workers count positions past the contig's end as depth 0 and so
close every run with its inclusive end, except a run that is still open after the last counted position, which it names
with e + 1 — that happens only when a record overhangs the contig's end.  Here coverage is clamped to the contig's length
and the name always carries the inclusive e.

--bed writes the kept runs (name, s, e + 1), --low_bed their complement inside each contig — the regions a polish could
not correct —, --bedgraph the depth itself (name, start, end, depth per stretch of equal depth; the only option that
brings the per-base array back from the device).

The helpers at the top need no device (parse_args, low_runs, fasta_text, bed_text, bedgraph_text); main() drives
np2_depth_from_bam."""
import argparse
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prog="nextpolish2_amd.lowdepth", description="write the stretches of an assembly whose mapping depth reaches a threshold")
    p.add_argument("bam", metavar="reads.map.sort.bam", help="coordinate-sorted, indexed BAM of the reads on the assembly")
    p.add_argument("genome", metavar="genome.fa[.gz]", help="the assembly")
    p.add_argument("-d", "--min_depth", type=int, default=3, metavar="N", help="keep positions covered by at least N counted records [3]")
    p.add_argument("-l", "--min_len", type=int, default=1000, metavar="N", help="keep runs of at least N positions [1000]")
    p.add_argument("-t", "--thread", type=int, default=1, metavar="N", help="accepted and ignored: the depth is counted on the device")
    p.add_argument("--min_fra", type=float, default=0.8, metavar="F", help="count a record only if its aligned bases are at least F of its read length [0.8]")
    p.add_argument("--min_mapq", type=int, default=0, metavar="Q", help="count a record only if its mapping quality is at least Q [0]")
    p.add_argument("--exclude_flags", type=lambda s: int(s, 0), default=0x4, metavar="FLAGS", help="do not count records with any of these flag bits [4]")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--bed", default=None, metavar="FILE", help="the kept runs as BED")
    p.add_argument("--low_bed", default=None, metavar="FILE", help="the complement of the kept runs inside each contig as BED")
    p.add_argument("--bedgraph", default=None, metavar="FILE", help="the depth as bedGraph (brings the per-base array back to the host)")
    p.add_argument("-o", "--out", default=None, metavar="FILE", help="FASTA [stdout]; a name ending in .gz or .bgz is written as BGZF; an existing file is not overwritten")
    return p


def parse_args(argv=None):
    """every argument error stops here, before a device is touched"""
    parser = build_parser()
    a = parser.parse_args(argv)
    if not 0 <= a.min_depth < 2 ** 32:
        parser.error("--min_depth: 0 <= N < 2^32")
    if not 0 <= a.min_len < 2 ** 32:
        parser.error("--min_len: 0 <= N < 2^32")
    if not 0.0 <= a.min_fra <= 1.0:  # (nan fails both comparisons)
        parser.error("--min_fra: a fraction in [0, 1]")
    if not 0 <= a.min_mapq <= 255:
        parser.error("--min_mapq: 0 <= Q <= 255")
    if not 0 <= a.exclude_flags <= 0xFFFF:
        parser.error("--exclude_flags: 16 flag bits")
    for f in (a.bam, a.genome):
        if not os.path.isfile(f):
            parser.error(f"cannot open {f}")
    if a.out is not None and os.path.exists(os.path.abspath(a.out)):
        raise SystemExit(f"Error: {os.path.abspath(a.out)!r} already exists!")
    return a


def low_runs(runs, L):
    """the complement of the kept runs (inclusive (s, e), ascending) inside [0, L): a list of inclusive (s, e)"""
    out, at = [], 0
    for s, e in runs:
        s, e = int(s), int(e)
        if s > at:
            out.append((at, s - 1))
        at = e + 1
    if at < L:
        out.append((at, L - 1))
    return out


def fasta_text(name, seq, runs):
    """the records of one contig: `seq` bytes, `runs` inclusive (s, e)"""
    return b"".join(b">%s_%d_%d\n%s\n" % (name.encode(), int(s), int(e), seq[int(s):int(e) + 1].upper()) for s, e in runs)


def bed_text(name, runs):
    return "".join("%s\t%d\t%d\n" % (name, int(s), int(e) + 1) for s, e in runs)


def bedgraph_text(name, depth):
    """name, start, end, depth per stretch of equal depth of the per-base array"""
    depth = np.asarray(depth)
    if len(depth) == 0:
        return ""
    cuts = np.concatenate([[0], np.flatnonzero(depth[1:] != depth[:-1]) + 1, [len(depth)]])
    return "".join("%s\t%d\t%d\t%d\n" % (name, cuts[i], cuts[i + 1], depth[cuts[i]]) for i in range(len(cuts) - 1))


def rate_text(name, bases_kept, L):
    return "output rate in %s: %.3f%%\n" % (name, 100.0 * bases_kept / L if L else 0.0)


def main(argv=None):
    a = parse_args(argv)
    from . import io as np2io
    from .api import Np2Error, Polisher
    try:
        if a.out is None:
            out = sys.stdout.buffer
        elif np2io.is_bgzf_path(a.out):  # the writers' rule: .gz / .bgz is BGZF, compressed on the device
            out = np2io.BgzfWriter(os.path.abspath(a.out), device=a.device)
        else:
            out = open(os.path.abspath(a.out), "xb")
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    side = {k: open(p, "w") for k, p in (("bed", a.bed), ("low_bed", a.low_bed), ("bedgraph", a.bedgraph)) if p is not None}
    try:
        pol = Polisher([], device=a.device)  # (no k-mer table: the depth needs the device and the BAM only)
        bam = np2io.Bam(os.path.abspath(a.bam))
        for name, seq in np2io.read_fasta(os.path.abspath(a.genome)):
            L = len(seq)
            runs, st, depth = np2io.depth_from_bam(pol, bam, name, L, min_depth=a.min_depth, min_len=a.min_len, min_aligned_fra=a.min_fra,
                                                   exclude_flags=a.exclude_flags, min_mapq=a.min_mapq, want_depth="bedgraph" in side)
            out.write(fasta_text(name, seq, runs))
            sys.stderr.write(rate_text(name, st["bases_kept"], L))
            if "bed" in side:
                side["bed"].write(bed_text(name, runs))
            if "low_bed" in side:
                side["low_bed"].write(bed_text(name, low_runs(runs, L)))
            if "bedgraph" in side:
                side["bedgraph"].write(bedgraph_text(name, depth))
        bam.close()
        pol.close()
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    finally:
        out.flush()
        if a.out is not None:
            out.close()
        for f in side.values():
            f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
