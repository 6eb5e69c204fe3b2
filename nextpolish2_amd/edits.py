"""What a polish changed, as VCF: the edits between a contig and its polished sequence, found and judged on the GPU
(np2_edits_* of include/np2.h, which states the rule: clean positions, raw runs, trimming, kinds, left-alignment, k-mer
support).

    python -m nextpolish2_amd.edits asm.fa[.gz] out_pos.tsv [k21.yak ...] -o edits.vcf [--summary FILE.tsv] [--edits_min_count N]

out_pos.tsv is the three-column text (contig, base, 0-based contig position) that the hidden --out_pos of nextPolish2 —
this project's or the reference binary's — writes instead of FASTA.  On the polishing command line the same report comes
from --edits FILE.vcf / --edits_summary FILE.tsv.

The library's records are unanchored; POS, REF and ALT are anchored here: an INS or DEL gets the contig base before it
prepended, or, where it starts the contig, the base after it appended (VCF 4.2, section 1.6.1).  INFO: KIND; OUT, the
0-based offset of ALT in the polished sequence; per k-mer table K<k>=absent_in/n_in,absent_out/n_out (the k-mers around
the edit in the contig and in the polished sequence that the table does not hold); VERDICT from the absent counts summed
over the tables: fewer after the edit is better, as many same, more worse (no table: same).

The helpers at the top need no device (anchor, vcf_line, read_out_pos); EditsReport and main() drive Polisher.edits_buffers."""
import argparse
import os
import sys

import numpy as np

SUMMARY_HEADER = ("contig", "len", "polished", "first", "last", "outside_span", "raw_runs", "same_runs", "edits", "SNV", "MNV", "INS",
                  "DEL", "CPX", "bases_inserted", "bases_deleted", "better", "same", "worse")


def anchor(ref, ref_pos, ref_s, alt_s, kind):
    """an unanchored record -> (POS 1-based, REF, ALT) as VCF wants them"""
    ref_s, alt_s = bytes(ref_s), bytes(alt_s)
    if kind not in ("INS", "DEL"):
        return ref_pos + 1, ref_s, alt_s
    if ref_pos > 0:
        a = bytes(ref[ref_pos - 1:ref_pos])
        return ref_pos, a + ref_s, a + alt_s
    a = bytes(ref[len(ref_s):len(ref_s) + 1]) or b"N"  # (the base after the event; a contig deleted whole has none)
    return 1, ref_s + a, alt_s + a


def verdict(support):
    """support: rows of (n_in, absent_in, n_out, absent_out), one per table"""
    a_in, a_out = sum(int(r[1]) for r in support), sum(int(r[3]) for r in support)
    return "better" if a_out < a_in else "same" if a_out == a_in else "worse"


def vcf_line(name, ref, rec, ks=(), support=()):
    """one record (dict: ref_pos, out_off, ref, alt, kind) of contig `name` whose sequence is `ref` -> a VCF line (bytes)"""
    pos, r, a = anchor(ref, rec["ref_pos"], rec["ref"], rec["alt"], rec["kind"])
    info = [b"KIND=" + rec["kind"].encode(), b"OUT=%d" % rec["out_off"]]
    info += [b"K%d=%d/%d,%d/%d" % (k, s[1], s[0], s[3], s[2]) for k, s in zip(ks, support)]
    info.append(b"VERDICT=" + verdict(support).encode())
    return b"\t".join([name.encode(), b"%d" % pos, b".", r, a, b".", b".", b";".join(info)]) + b"\n"


def vcf_header(contigs, ks):
    """contigs: (name, length) in file order"""
    h = [b"##fileformat=VCFv4.2\n", b"##source=nextPolish2 --edits (np2-mi355x)\n"]
    h += [b"##contig=<ID=%s,length=%d>\n" % (n.encode(), ln) for n, ln in contigs]
    h.append(b'##INFO=<ID=KIND,Number=1,Type=String,Description="SNV, MNV, INS, DEL or CPX (a replaced region is not aligned inside)">\n')
    h.append(b'##INFO=<ID=OUT,Number=1,Type=Integer,Description="0-based offset of the unanchored ALT in the polished sequence">\n')
    for k in ks:
        h.append(b'##INFO=<ID=K%d,Number=2,Type=String,Description="%d-mers around the edit the table does not hold: absent/all in the '
                 b'contig, absent/all in the polished sequence">\n' % (k, k))
    h.append(b'##INFO=<ID=VERDICT,Number=1,Type=String,Description="better, same or worse: absent k-mers after against before, '
             b'summed over the tables">\n')
    h.append(b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    return h


def read_out_pos(path):
    """the three-column --out_pos text -> {contig: (bases as uint8 array, positions as uint32 array)}, contigs in file order"""
    names, cuts = [], []
    bases, pos = [], []
    with open(path, "rb") as f:
        for i, line in enumerate(f):
            c = line.rstrip(b"\n").split(b"\t")
            if len(c) != 3 or len(c[1]) != 1:
                raise ValueError(f"{path}: line {i + 1} is not 'contig<TAB>base<TAB>position'")
            if not names or names[-1] != c[0]:
                if c[0] in names:
                    raise ValueError(f"{path}: contig {c[0].decode()!r} comes in two pieces")
                names.append(c[0])
                cuts.append(len(bases))
            bases.append(c[1][0])
            pos.append(int(c[2]))
    cuts.append(len(bases))
    b, p = np.array(bases, dtype=np.uint8), np.array(pos, dtype=np.int64)
    if len(p) and (p.min() < 0 or p.max() > 0xFFFFFFFF):
        raise ValueError(f"{path}: a position is not a 32-bit number")
    p = p.astype(np.uint32)
    return {n.decode(): (b[cuts[i]:cuts[i + 1]], p[cuts[i]:cuts[i + 1]]) for i, n in enumerate(names)}


class EditsReport:
    """Collects the edits of an assembly's contigs in file order and writes the VCF and the per-contig summary.  One
    context, one thread."""

    def __init__(self, ks, min_count=1):
        self.ks, self.min_count = list(ks), int(min_count)
        self.contigs = []  # (name, length, ref or None, api.Edits or None)

    def add(self, pol, name, ref, bases, pos):
        """one polished contig: np2_edits_buffers of its output against `ref` on `pol`, every table of it"""
        self.add_result(name, ref, pol.edits_buffers(ref, bases, pos, min_count=self.min_count))

    def add_result(self, name, ref, res):
        if res.table_k != self.ks:
            raise ValueError(f"the edits of {name} were judged by tables of k = {res.table_k}, the report is for {self.ks}")
        self.contigs.append((name, len(ref), bytes(ref), res))

    def add_unpolished(self, name, length):
        """a contig passed through as it was (-L): a summary row of zeros"""
        self.contigs.append((name, int(length), None, None))

    def vcf_lines(self):
        out = vcf_header([(n, ln) for n, ln, _, _ in self.contigs], self.ks)
        for name, _, ref, res in self.contigs:
            if res is None:
                continue
            for i, rec in enumerate(res.records()):
                out.append(vcf_line(name, ref, rec, self.ks, res.support[i]))
        return out

    def summary_lines(self):
        out = ["\t".join(SUMMARY_HEADER) + "\n"]
        for name, ln, _, res in self.contigs:
            if res is None:
                out.append("\t".join([name, str(ln)] + ["0"] * (len(SUMMARY_HEADER) - 2)) + "\n")
                continue
            t = res.totals
            v = [verdict(res.support[i]) for i in range(len(res))]
            row = [name, ln, 1, t["first"], t["last"], t["outside"], t["raw_runs"], t["same_runs"], len(res)] + t["n_kind"] + \
                  [t["bases_inserted"], t["bases_deleted"], v.count("better"), v.count("same"), v.count("worse")]
            out.append("\t".join(str(x) for x in row) + "\n")
        return out

    def write_cli(self, vcf_path=None, summary_path=None):
        """the command line's --edits FILE.vcf and --edits_summary FILE.tsv"""
        if vcf_path:
            with open(vcf_path, "wb") as f:
                f.writelines(self.vcf_lines())
        if summary_path:
            with open(summary_path, "w") as f:
                f.writelines(self.summary_lines())


def build_parser():
    p = argparse.ArgumentParser(prog="nextpolish2_amd.edits", description="the edits between an assembly and its polished --out_pos text, as VCF")
    p.add_argument("fa", metavar="asm.fa[.gz]", help="the assembly that was polished, in [GZIP] FASTA format")
    p.add_argument("out_pos", metavar="out_pos.tsv", help="the polish's --out_pos text: contig, base, 0-based contig position")
    p.add_argument("yak", nargs="*", metavar="k.yak", help="k-mer dumps in yak format to judge every edit by")
    p.add_argument("-o", "--out", default=None, metavar="FILE", help="VCF [stdout]")
    p.add_argument("--summary", default=None, metavar="FILE", help="per-contig summary TSV")
    p.add_argument("--edits_min_count", type=int, default=1, metavar="N", help="read a k-mer count below N as absent [1]")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    from . import io as np2io
    from .api import Np2Error, Polisher
    parser = build_parser()
    a = parser.parse_args(argv)
    if not 0 <= a.edits_min_count <= 1023:
        parser.error("--edits_min_count: 0 .. 1023")
    try:
        ks = sorted(np2io.check_yak_header(y) for y in a.yak)
        outs = read_out_pos(a.out_pos)
    except (ValueError, OSError) as e:
        raise SystemExit(f"Error: {e}")
    try:
        pol = np2io.polisher_from_yak_files([os.path.abspath(y) for y in a.yak], device=a.device) if a.yak else Polisher([], device=a.device)
        rep = EditsReport(ks, a.edits_min_count)
        seen = set()
        for name, seq in np2io.read_fasta(a.fa):
            if name in outs:
                rep.add(pol, name, seq, *outs[name])
                seen.add(name)
            else:
                rep.add_unpolished(name, len(seq))
        pol.close()
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    missing = [n for n in outs if n not in seen]
    if missing:
        raise SystemExit(f"Error: {a.out_pos} names contigs the assembly does not have: {', '.join(missing[:5])}")
    if a.out is None:
        sys.stdout.buffer.writelines(rep.vcf_lines())
    else:
        rep.write_cli(a.out, None)
    rep.write_cli(None, a.summary)
    return 0


if __name__ == "__main__":
    sys.exit(main())
