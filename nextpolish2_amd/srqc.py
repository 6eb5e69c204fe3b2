"""python -m nextpolish2_amd.srqc: quality-trim and filter short reads on the GPU (the preparation step the reference's
README asks for before `yak count`; its recipe is fastp -5 -3 -n 0 -f 5 -F 5 -t 5 -T 5 -q 20).

    python -m nextpolish2_amd.srqc reads.fq.gz ... [--sr_qc SPEC] [--sr_adapter [SPEC]] [--report qc.tsv] [--out_fq PREFIX [--out_gz]]

The rule is this project's own, built on the options of that recipe; it is not pinned against the fastp binary.  One read
has n bases and n quality bytes, p[i] = max(0, byte - 33):
  1. the first `front` and the last `tail` bases go;
  2. cut5: the kept span starts at the first window of `window` bases whose quality sum is at least mean * window (no such
     window: the read is emptied), then leading N are skipped;
  3. cut3: the same from the end;
  4. the read fails as too short (fewer than `len` bases left, or none), too many N (more than `n`), or low quality (more
     than `u` percent of the kept bases below `q`), in this order.
Reads are judged one by one: paired files are not kept in step.  No adapter trimming, no poly-G / poly-X trimming, no
complexity and no average-quality filter.  Inputs are FASTQ, plain or gzip.

--report writes a TSV, one line per file and a total: reads, pass, too_short, too_many_n, low_quality, bases_in, bases_out
(standard output without it).  --out_fq PREFIX writes the passing reads of input i, trimmed, to PREFIX.<i>.fq; with --out_gz
to PREFIX.<i>.fq.gz, BGZF compressed on the device (what the reference's recipe names sr.R1.clean.fastq.gz).  Existing
files are not overwritten.  The k-mer counter takes the same option (nextpolish2_amd.count --sr_qc, nextPolish2 --sr ..
--sr_qc) and filters on the way, without the files.

--sr_adapter [SPEC] adds adapter trimming (include/np2_io.h has the rule; it is this project's own, on fastp's documented
options, and equality with the fastp binary is not claimed).  Alone it is pair=1,overlap=30,diff=5,diffpct=20: the files are
R1 R2 R1 R2 .. and are read in step, the mates' overlap is searched and a read-through adapter cut off both, a pair is
dropped as soon as one mate fails (class mate_failed), and --out_fq writes only pairs that pass in both mates, so the
outputs stay in step.  seq=ACGT..[,seq2=ACGT..] trims by sequence where no overlap was found; pair=0,seq=.. trims
single-end reads.  The report then has one line per pair of files (named R1,R2) and the columns mate_failed, pairs,
pairs_overlap, pairs_unsearched, trimmed_overlap, trimmed_seq, adapter_bases as well.  Not done: interleaved FASTQ,
read-name checks, fastp's base correction inside the overlap, merging mates, poly-G / poly-X, adapter auto-detection for
single-end input."""
import argparse
import os
import sys

from . import io as np2io
from ._types import SRADAPT_STATS, SRQC_STATS
from .api import Np2Error


def build_parser():
    p = argparse.ArgumentParser(prog="nextpolish2_amd.srqc", description="quality-trim and filter short reads on the GPU",
                                epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("reads", nargs="+", metavar="reads.fq[.gz]", help="FASTQ files, plain or gzip")
    p.add_argument("--sr_qc", nargs="?", const=np2io.SrQc(), default=np2io.SrQc(), type=np2io.sr_qc_arg, metavar="SPEC", help=np2io.SR_QC_HELP)
    p.add_argument("--sr_adapter", nargs="?", const="", default=None, type=np2io.sr_adapter_arg, metavar="SPEC", help=np2io.SR_ADAPTER_HELP)
    p.add_argument("--report", default=None, metavar="FILE", help="the totals as a TSV [stdout]")
    p.add_argument("--out_fq", default=None, metavar="PREFIX", help="write the cleaned reads of input i to PREFIX.<i>.fq")
    p.add_argument("--out_gz", action="store_true", help="with --out_fq: write PREFIX.<i>.fq.gz, BGZF compressed on the device")
    p.add_argument("--device", type=int, default=0)
    return p


def report_text(paths, stats, names=SRQC_STATS):
    rows = ["\t".join(("file",) + names)]
    for name, st in zip(list(paths) + ["total"], stats):
        rows.append("\t".join([name] + [str(st[k]) for k in names]))
    return "\n".join(rows) + "\n"


def parse_args(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    np2io.check_sr_adapter(p, a.sr_adapter, a.reads)
    if a.out_gz and a.out_fq is None:
        p.error("--out_gz needs --out_fq")
    for r in a.reads:
        if not os.path.exists(r):
            p.error(f"cannot open {r}")
    a.out_paths = None if a.out_fq is None else [f"{a.out_fq}.{i}.fq" + (".gz" if a.out_gz else "") for i in range(len(a.reads))]
    for out in ([a.report] if a.report else []) + (a.out_paths or []):
        if os.path.exists(out):  # like the other modules: nothing is overwritten
            raise SystemExit(f"Error: {os.path.abspath(out)!r} already exists!")
    return a


def main(argv=None):
    a = parse_args(argv)
    try:
        if a.sr_adapter is not None:
            stats = np2io.sradapt_files(a.reads, a.sr_qc, a.sr_adapter, a.out_paths, device=a.device)
        else:
            stats = np2io.srqc_files(a.reads, a.sr_qc, a.out_paths, device=a.device)
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    if a.sr_adapter is not None:
        units = [",".join(a.reads[i:i + 2]) for i in range(0, len(a.reads), 2)] if a.sr_adapter.pair else a.reads
        text = report_text(units, stats, SRADAPT_STATS)
    else:
        text = report_text(a.reads, stats)
    if a.report:
        with open(a.report, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print(f"[np2 srqc] {(np2io.sradapt_stats_text if a.sr_adapter is not None else np2io.srqc_stats_text)(stats[-1])}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
