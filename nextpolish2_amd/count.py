"""python -m nextpolish2_amd.count: short reads -> yak v2 k-mer dumps, counted on the GPU (what `yak count` does in the
reference workflow, README steps 2-3).

    python -m nextpolish2_amd.count -k 21 -o k21.yak [-k 31 -o k31.yak] [-m MIN_COUNT] reads.fq.gz ...

Inputs are FASTA / FASTQ / one-sequence-per-line files, plain or gzip; they are parsed once for all k.  -m is an exact
threshold (words with a smaller count are not written); counts saturate at 1023.  --sr_qc [SPEC] quality-trims and filters
the reads on the GPU first (FASTQ input; python -m nextpolish2_amd.srqc has the rule).  --sr_adapter [SPEC] trims adapters
as well: alone, the files are pairs R1 R2 R1 R2 .. and the mates' overlap decides (include/np2_io.h has the rule)."""
import argparse
import sys

from . import io as np2io
from .api import Np2Error


def build_parser():
    p = argparse.ArgumentParser(prog="nextpolish2_amd.count", description="count canonical k-mers of short reads into yak dumps")
    p.add_argument("reads", nargs="+", metavar="reads.fq[.gz]", help="sequence files (FASTA / FASTQ / one sequence per line, plain or gzip)")
    p.add_argument("-k", dest="k", type=int, action="append", help="k-mer size, 2 .. 31; may repeat [21]")
    p.add_argument("-o", dest="out", action="append", metavar="FILE", help="output dump, one per -k [k<K>.yak]")
    p.add_argument("-m", "--min_count", type=int, default=1, help="leave out words counted fewer times [1]")
    p.add_argument("--mem", type=float, default=0.0, metavar="GB", help="device memory for the counting tables [half of what is free]")
    p.add_argument("--sr_qc", nargs="?", const=np2io.SrQc(), default=None, type=np2io.sr_qc_arg, metavar="SPEC", help=np2io.SR_QC_HELP)
    p.add_argument("--sr_adapter", nargs="?", const="", default=None, type=np2io.sr_adapter_arg, metavar="SPEC", help=np2io.SR_ADAPTER_HELP)
    p.add_argument("--device", type=int, default=0)
    return p


def parse_args(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    np2io.check_sr_adapter(p, a.sr_adapter, a.reads)
    return a


def main(argv=None):
    a = parse_args(argv)
    ks = a.k or [21]
    outs = a.out or [f"k{k}.yak" for k in ks]
    if len(outs) != len(ks):
        raise SystemExit("error: one -o per -k")
    try:
        np2io.count_kmers_to_files(a.reads, ks, outs, min_count=a.min_count, device=a.device, mem_bytes=int(a.mem * 1e9),
                                   qc=a.sr_qc, ad=a.sr_adapter)
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    st = np2io.kcount_last_stats()
    print(f"[np2 count] {st['kmers']} k-mers, {st['distinct']} distinct, {st['passes']} pass(es), {st['growths']} table growth(s), "
          f"count kernel {st['kernel_ms']:.1f} ms" + (f"; sr_adapter: {np2io.sradapt_stats_text(np2io.sradapt_last_stats())}" if a.sr_adapter is not None else
                                                       f"; sr_qc: {np2io.srqc_stats_text(np2io.srqc_last_stats())}" if a.sr_qc is not None else ""),
          file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
