"""Call read-supported variants of an assembly from the reads mapped to it, on the GPU, and count the homozygous ones: a site
where nearly every read disagrees with the assembly is a potential error of the assembly, not a heterozygous site (the
reference's doc/benchmark5.md, step 5, compares that count before and after the polish).

    python -m nextpolish2_amd.varcall hifi.map.sort.bam asm.fa[.gz] -o calls.vcf[.gz] [--summary calls.tsv] [--het]

The BAM is the one `map -a --qual --MD ... | samsort --full` writes (coordinate-sorted, indexed, SEQ present).  The rule is
this project's own (include/np2_io.h, np2_varcall_*): per-position counts of the counted records, indel alleles left-aligned
and tallied, integer thresholds.  It has no quality model; equality with DeepVariant, bcftools or any other caller is not
claimed.  A record is counted unless one of its flag bits is in --exclude_flags (0xF04), its mapping quality is below -q (5),
its aligned fraction is below --min_fra (0), it has an N operation or no SEQ.  A site is called when at least -d (8) counted
records cover it, at least --min_alt (3) of them hold the allele, and they are at least --hom (0.8) of the depth: a
homozygous call, 1/1.  With --het, alleles of at least --het_frac (0.25) are called too, as 0/1.

Contig by contig over the BAM's references; names the FASTA lacks are skipped.  VCF 4.2: POS is 1-based (an indel's is its
anchor base), QUAL is '.', FILTER PASS, INFO KIND=SNV|INS|DEL;DP=d;AC=c, FORMAT GT:DP:AD.  A path ending in .gz or .bgz is
written as BGZF, compressed on the device.  --summary: per contig and in total, the callable bases (covered by -d records, A
C G T in the assembly), the calls by kind and genotype, and the homozygous calls per Mb of callable bases.

Not here: a quality score or genotype likelihoods, more than one alt per site, MNVs and complex alleles, SAM text or reads
as input (write the BAM with samsort first), several ranks, base qualities, gVCF."""
import argparse
import os
import sys

KINDS = ("SNV", "DEL", "INS")
VCF_META = ("##fileformat=VCFv4.2\n##source=nextpolish2_amd.varcall\n%s"
            "##INFO=<ID=KIND,Number=1,Type=String,Description=\"SNV, INS or DEL\">\n"
            "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Counted records covering the site\">\n"
            "##INFO=<ID=AC,Number=1,Type=Integer,Description=\"Counted records holding the called allele\">\n"
            "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
            "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Counted records covering the site\">\n"
            "##FORMAT=<ID=AD,Number=1,Type=Integer,Description=\"Counted records holding the called allele\">\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
SUMMARY_COLS = ("callable", "snv_hom", "ins_hom", "del_hom", "snv_het", "ins_het", "del_het")
SUMMARY_HEADER = "#contig\tcallable\thom_snv\thom_ins\thom_del\thet_snv\thet_ins\thet_del\thom_per_mb\n"


def build_parser():
    p = argparse.ArgumentParser(prog="nextpolish2_amd.varcall", description="call read-supported variants of an assembly; the homozygous ones are its potential errors")
    p.add_argument("bam", metavar="hifi.map.sort.bam", help="coordinate-sorted, indexed BAM of the reads on the assembly, with SEQ")
    p.add_argument("genome", metavar="asm.fa[.gz]", help="the assembly")
    p.add_argument("-o", "--out", required=True, metavar="FILE", help="VCF; a name ending in .gz or .bgz is written as BGZF; an existing file is not overwritten")
    p.add_argument("--summary", default=None, metavar="FILE", help="per contig and in total: callable bases, calls by kind and genotype, homozygous calls per Mb")
    p.add_argument("--het", action="store_true", help="also call alleles of at least --het_frac of the depth, as 0/1")
    p.add_argument("-d", "--min_depth", type=int, default=8, metavar="N", help="call only where at least N counted records cover the site [8]")
    p.add_argument("--min_alt", type=int, default=3, metavar="N", help="call only alleles held by at least N counted records [3]")
    p.add_argument("--hom", type=float, default=0.8, metavar="F", help="homozygous: the allele is at least F of the depth [0.8]")
    p.add_argument("--het_frac", type=float, default=0.25, metavar="F", help="with --het: heterozygous from F of the depth on [0.25]")
    p.add_argument("-q", "--min_mapq", type=int, default=5, metavar="Q", help="count a record only if its mapping quality is at least Q [5]")
    p.add_argument("--exclude_flags", type=lambda s: int(s, 0), default=0xF04, metavar="FLAGS", help="do not count records with any of these flag bits [0xF04]")
    p.add_argument("--min_fra", type=float, default=0.0, metavar="F", help="count a record only if its aligned bases are at least F of its read length [0]")
    p.add_argument("--max_indel", type=int, default=28, metavar="N", help="tally insertions and deletions of up to N bases, at most 28 [28]")
    p.add_argument("--device", type=int, default=0)
    return p


def per_mille(f):
    return int(round(f * 1000))


def parse_args(argv=None):
    """every argument error stops here, before the library is loaded"""
    parser = build_parser()
    a = parser.parse_args(argv)
    if not 0 <= a.min_depth < 2 ** 32:
        parser.error("--min_depth: 0 <= N < 2^32")
    if not 1 <= a.min_alt < 2 ** 32:
        parser.error("--min_alt: 1 <= N < 2^32 (a call needs a read)")
    if not 0.0 <= a.hom <= 1.0:  # (nan fails both comparisons)
        parser.error("--hom: a fraction in [0, 1]")
    if not 0.0 <= a.het_frac <= 1.0:
        parser.error("--het_frac: a fraction in [0, 1]")
    if a.het and per_mille(a.het_frac) > per_mille(a.hom):
        parser.error("--het_frac must not exceed --hom")
    if not 0 <= a.min_mapq <= 255:
        parser.error("--min_mapq: 0 <= Q <= 255")
    if not 0 <= a.exclude_flags <= 0xFFFF:
        parser.error("--exclude_flags: 16 flag bits")
    if not 0.0 <= a.min_fra <= 1.0:
        parser.error("--min_fra: a fraction in [0, 1]")
    if not 1 <= a.max_indel <= 28:
        parser.error("--max_indel: 1 <= N <= 28")
    for f in (a.bam, a.genome):
        if not os.path.isfile(f):
            parser.error(f"cannot open {f}")
    for f in (a.out, a.summary):
        if f is not None and os.path.exists(os.path.abspath(f)):
            raise SystemExit(f"Error: {os.path.abspath(f)!r} already exists!")
    a.hom_pm = per_mille(a.hom)
    a.het_pm = per_mille(a.het_frac) if a.het else a.hom_pm  # (het_pm = hom_pm: homozygous calls only)
    return a


def vcf_header(contigs):
    """contigs: [(name, length)]"""
    return VCF_META % "".join("##contig=<ID=%s,length=%d>\n" % c for c in contigs)


def vcf_text(name, seq, calls):
    """the records of one contig: `seq` its bytes, `calls` an api.VARCALL_DTYPE array"""
    out = []
    for pos, depth, count, bases, kind, gt, n, alt_code in zip(*(calls[f].tolist() for f in ("pos", "depth", "count", "bases", "kind", "gt", "len", "alt_code"))):
        anchor = seq[pos:pos + 1].upper().decode()
        if kind == 0:
            ref, alt = anchor, "ACGT"[alt_code]
        elif kind == 1:
            ref, alt = seq[pos:pos + 1 + n].upper().decode(), anchor
        else:
            ref, alt = anchor, anchor + "".join("ACGT"[(bases >> (2 * (n - 1 - i))) & 3] for i in range(n))
        out.append("%s\t%d\t.\t%s\t%s\t.\tPASS\tKIND=%s;DP=%d;AC=%d\tGT:DP:AD\t%s:%d:%d\n"
                   % (name, pos + 1, ref, alt, KINDS[kind], depth, count, "1/1" if gt == 2 else "0/1", depth, count))
    return "".join(out)


def summary_text(rows):
    """rows: [(name, stats)] -> one row per contig and the total"""
    total = dict.fromkeys(SUMMARY_COLS, 0)
    for _, st in rows:
        for k in SUMMARY_COLS:
            total[k] += int(st[k])
    out = [SUMMARY_HEADER]
    for name, st in rows + [("total", total)]:
        hom = int(st["snv_hom"]) + int(st["ins_hom"]) + int(st["del_hom"])
        out.append("%s\t%s\t%.3f\n" % (name, "\t".join(str(int(st[k])) for k in SUMMARY_COLS), hom * 1e6 / int(st["callable"]) if int(st["callable"]) else 0.0))
    return "".join(out)


def main(argv=None):
    a = parse_args(argv)
    from . import io as np2io
    from .api import Np2Error, Polisher, varcall_from_bam
    try:
        out = np2io.BgzfWriter(os.path.abspath(a.out), device=a.device) if np2io.is_bgzf_path(a.out) else open(os.path.abspath(a.out), "xb")
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    rows = []
    try:
        pol = Polisher([], device=a.device)  # (no k-mer table: the caller needs the device, the BAM and the assembly only)
        bam = np2io.Bam(os.path.abspath(a.bam))
        seqs = {name: seq for name, seq in np2io.read_fasta(os.path.abspath(a.genome))}
        refs = [(name, n) for name, n in bam.refs() if name in seqs]
        for name, n in refs:
            if len(seqs[name]) != n:
                raise SystemExit(f"Error: {name} has {n} bases in the BAM header and {len(seqs[name])} in {a.genome}")
        out.write(vcf_header(refs).encode())
        for name, _ in refs:
            calls, st, _, _ = varcall_from_bam(pol, bam, name, seqs[name], min_depth=a.min_depth, min_alt=a.min_alt, hom_pm=a.hom_pm, het_pm=a.het_pm,
                                               max_indel=a.max_indel, min_aligned_fra=a.min_fra, exclude_flags=a.exclude_flags, min_mapq=a.min_mapq)
            out.write(vcf_text(name, seqs[name], calls).encode())
            rows.append((name, st))
            sys.stderr.write("%s: %d of %d records counted, %d callable bases, %d homozygous and %d heterozygous calls\n"
                             % (name, st["records_counted"], st["records_seen"], st["callable"], st["snv_hom"] + st["ins_hom"] + st["del_hom"],
                                st["snv_het"] + st["ins_het"] + st["del_het"]))
        bam.close()
        pol.close()
        if a.summary is not None:
            with open(os.path.abspath(a.summary), "x") as f:
                f.write(summary_text(rows))
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    finally:
        out.flush()
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
