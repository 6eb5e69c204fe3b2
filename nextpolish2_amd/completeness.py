"""K-mer completeness and copy-number spectrum of an assembly against short-read k-mer tables, measured on the GPU (what
Merqury reports beside its QV: `reads.meryl`, `meryl greater-than 1`, spectra-cn).

    python -m nextpolish2_amd.completeness asm.fa[.gz] k21.yak [k31.yak ...] [--hap2 other.fa[.gz]] [--min_count 2]
                                           [--spectra PREFIX] [-o FILE]
    python -m nextpolish2_amd.completeness asm.fa[.gz] --sr reads.fq.gz [--sr ...] [--sr_k 21,31] [--sr_min_count 2] ...

QV asks which assembly k-mers the reads do not support; completeness asks which RELIABLE read k-mers (stored count >=
max(--min_count, 1)) the assembly lost: found / read_kmers over distinct canonical k-mers, as a percentage.  The spectrum
splits the reliable read k-mers by their copy number in the assembly (read-only, 1, 2, 3, 4, >4) and their read count; a
collapsed haplotype shows as a 2-copy band that moved to 1, which QV cannot see.  asm_only are the assembly's k-mers whose
read count, read as 0 below --min_count, is 0.  With --hap2 the two files are measured apart (hap1, hap2) and together
(both: one set of all their sequences).

The helpers at the top need no device (completeness_value, completeness_text, spectra_rows); CmpReport and main() drive
Polisher.cmp_strings."""
import argparse
import math
import sys

import numpy as np

TSV_HEADER = ("set", "k", "read_kmers", "found", "completeness", "asm_kmers", "asm_only")
SPECTRA_HEADER = ("copies", "count", "kmers")
COPIES = ("read-only", "1", "2", "3", "4", ">4")  # min(copy number in the assembly, 5)


def completeness_value(n_found, n_read):
    """found / reliable read k-mers as a percentage.  No reliable read k-mer: nan."""
    n_found, n_read = int(n_found), int(n_read)
    return math.nan if n_read == 0 else 100.0 * n_found / n_read


def completeness_text(n_found, n_read):
    v = completeness_value(n_found, n_read)
    return "nan" if math.isnan(v) else "%.4f" % v


def spectra_rows(spectra, asm_only):
    """[(copies, count, kmers)]: the non-zero cells of a (6, 1024) spectrum, class by class in ascending count, then the
    non-zero asm_only entries as ("asm-only:<copies>", 0, kmers)."""
    sp = np.asarray(spectra, dtype=np.uint64).reshape(len(COPIES), -1)
    rows = [(COPIES[cls], int(c), int(sp[cls, c])) for cls in range(len(COPIES)) for c in np.flatnonzero(sp[cls])]
    return rows + [("asm-only:" + COPIES[cls], 0, int(v)) for cls, v in enumerate(np.asarray(asm_only, dtype=np.uint64)) if v]


class CmpReport:
    """Collects, per table of a Polisher, the completeness of named sequence sets ("in" / "out" on the command line) and
    writes the TSV and the spectra files.  One context, one thread."""

    def __init__(self, ks, min_count=2, want_spectra=False):
        self.ks, self.min_count, self.want_spectra = list(ks), int(min_count), want_spectra
        self.rows = []     # (set, k, (n_read, n_found, n_asm, n_asm_only))
        self.spectra = {}  # (set, k) -> (spectra, asm_only)

    def add(self, pol, name, seqs):
        """one set: its sequences (bytes each) taken together, measured against every table of `pol`"""
        for t, k in enumerate(self.ks):
            r = pol.cmp_strings(t, seqs, self.min_count, spectra=self.want_spectra)
            self.rows.append((name, k, tuple(int(x) for x in r.stats)))
            if self.want_spectra:
                self.spectra[(name, k)] = (r.spectra, r.asm_only)

    def lines(self):
        out = ["\t".join(TSV_HEADER) + "\n"]
        for name, k, (n_read, n_found, n_asm, n_asm_only) in self.rows:
            out.append("\t".join([str(name), str(k), str(n_read), str(n_found), completeness_text(n_found, n_read), str(n_asm),
                                  str(n_asm_only)]) + "\n")
        return out

    def spectra_text(self, name, k):
        sp, ao = self.spectra[(name, k)]
        return "\t".join(SPECTRA_HEADER) + "\n" + "".join("%s\t%d\t%d\n" % r for r in spectra_rows(sp, ao))

    def write_spectra(self, prefix):
        for name, k in self.spectra:
            with open(f"{prefix}.k{k}.{name}.tsv", "w") as f:
                f.write(self.spectra_text(name, k))

    def write_cli(self, tsv_path, spectra_prefix=None):
        """the command line's --cmp FILE and --cmp_spectra PREFIX (PREFIX.k<K>.in.tsv / PREFIX.k<K>.out.tsv)"""
        with open(tsv_path, "w") as f:
            f.writelines(self.lines())
        if spectra_prefix:
            self.write_spectra(spectra_prefix)


def build_parser():
    from . import io as np2io
    p = argparse.ArgumentParser(prog="nextpolish2_amd.completeness",
                                description="k-mer completeness and copy-number spectrum of an assembly against short-read k-mer tables")
    p.add_argument("fa", metavar="asm.fa[.gz]", help="assembly in [GZIP] FASTA format")
    p.add_argument("--hap2", default=None, metavar="FILE", help="the other haplotype's assembly: rows hap1, hap2 and both")
    np2io.add_table_args(p)
    p.add_argument("--min_count", type=int, default=2, metavar="N", help="a read k-mer counted at least N times is reliable [2]")
    p.add_argument("--spectra", default=None, metavar="PREFIX", help="copy-number spectra: PREFIX.k<K>.<set>.tsv (copies, count, kmers)")
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
    if not 0 <= a.min_count <= 1023:
        parser.error("--min_count: 0 .. 1023")
    try:
        pol, ks = np2io.open_tables(parser, a)
        rep = CmpReport(ks, a.min_count, want_spectra=a.spectra is not None)
        hap1 = [seq for _, seq in np2io.read_fasta(a.fa)]
        if a.hap2 is None:
            rep.add(pol, "asm", hap1)
        else:
            hap2 = [seq for _, seq in np2io.read_fasta(a.hap2)]
            rep.add(pol, "hap1", hap1)
            rep.add(pol, "hap2", hap2)
            rep.add(pol, "both", hap1 + hap2)
        pol.close()
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    text = "".join(rep.lines())
    if a.out is None:
        sys.stdout.write(text)
    else:
        with open(a.out, "w") as f:
            f.write(text)
    if a.spectra is not None:
        rep.write_spectra(a.spectra)
    return 0


if __name__ == "__main__":
    sys.exit(main())
