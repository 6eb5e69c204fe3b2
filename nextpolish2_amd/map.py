"""Map HiFi reads to the assembly on the device: minimizer seeds chained into PAF, or with -a the primary chain aligned base
by base and written as SAM (the recipe's `winnowmap -ax` step; its SAM pipes into `python -m nextpolish2_amd.cli -`).

    python -m nextpolish2_amd.map asm.fa[.gz] hifi.fa[.gz] [more reads ...] [-o map.paf[.gz]] [-k 19] [-w 19] [--max_occ 200]
                                  [--lookback 64] [--max_gap 10000] [--bandwidth 500] [--min_cnt 3] [--min_score 40] [--stats FILE]
                                  [-a [-A 1] [-B 4] [-O 6] [-E 2] [--band 32] [--end_bonus 5] [--ext_max 2048] [--max_cells N]]

One line per mapped read, in read order: qname qlen qs qe strand tname tlen ts te matches block mapq tp:A:P cm:i: s1:i: s2:i:
(the rule: include/np2_io.h, np2_map_*; it follows minimap2's published seed-and-chain algorithm and is not pinned against
the minimap2 binary).  An output path ending in .gz / .bgz is written as BGZF, compressed on the device.

With -a: a SAM header and one line per read, in read order: qname flag rname pos mapq CIGAR * 0 0 SEQ * NM:i: AS:i: cm:i: s1:i:
s2:i: (the rule: np2_map_align_*; M, I, D and S only, gaps left-aligned; an unmapped read has flag 4).  --stats then writes a
second header and row, ALIGN_STATS_HEADER.
"""
import argparse
import os
import shutil
import sys
import tempfile

STATS_HEADER = ("reads", "mapped", "unmapped", "minimizers", "anchors", "dropped_occ", "index_minimizers", "pieces", "groups", "index_ms",
                "sketch_ms", "seed_ms", "sort_ms", "chain_ms", "read_ms", "write_ms")


def stats_row(stats, index_ms):
    """--stats: a header line and one TSV row (counts, then times in ms with three decimals)"""
    st = dict(stats, index_ms=index_ms)
    cells = [str(int(st[f])) for f in STATS_HEADER[:9]] + ["%.3f" % float(st[f]) for f in STATS_HEADER[9:]]
    return "\t".join(STATS_HEADER) + "\n" + "\t".join(cells) + "\n"


ALIGN_STATS_HEADER = ("pins", "segments", "equal", "pure_gap", "snv", "cores", "cells", "clipped_bases", "overflow", "pins_ms",
                      "classify_ms", "dp_ms", "assemble_ms", "write_ms")
ALIGN_FLAGS = (("match", "-A"), ("mismatch", "-B"), ("gap_open", "-O"), ("gap_ext", "-E"), ("band", "--band"), ("end_bonus", "--end_bonus"),
               ("ext_max", "--ext_max"), ("max_cells", "--max_cells"))


def align_stats_row(stats):
    """--stats with -a: a second header line and TSV row (counts, then times in ms with three decimals)"""
    cells = [str(int(stats[f])) for f in ALIGN_STATS_HEADER[:9]] + ["%.3f" % float(stats[f]) for f in ALIGN_STATS_HEADER[9:]]
    return "\t".join(ALIGN_STATS_HEADER) + "\n" + "\t".join(cells) + "\n"


def build_parser():
    from .io import ALIGN_DEFAULTS as AD
    from .io import MAP_DEFAULTS as D
    p = argparse.ArgumentParser(prog="nextpolish2_amd.map", description="map long reads to an assembly: minimizer seeds and chains to PAF")
    p.add_argument("asm", metavar="asm.fa[.gz]", help="assembly in [GZIP] FASTA format")
    p.add_argument("reads", nargs="+", metavar="hifi.fa[.gz]", help="reads in [GZIP] FASTA / FASTQ format")
    p.add_argument("-k", type=int, default=D["k"], metavar="K", help="k-mer size, 11 .. 28 [19]")
    p.add_argument("-w", type=int, default=D["w"], metavar="W", help="minimizer window, 1 .. 64 [19]")
    p.add_argument("--max_occ", type=int, default=D["max_occ"], metavar="N", help="drop minimizers that occur more often in the assembly [200]")
    p.add_argument("--lookback", type=int, default=D["lookback"], metavar="N", help="chain predecessors tried per anchor, 1 .. 64 [64]")
    p.add_argument("--max_gap", type=int, default=D["max_gap"], metavar="N", help="largest gap between two chained anchors [10000]")
    p.add_argument("--bandwidth", type=int, default=D["bandwidth"], metavar="N", help="largest diagonal shift between them [500]")
    p.add_argument("--min_cnt", type=int, default=D["min_cnt"], metavar="N", help="fewest anchors of a reported chain [3]")
    p.add_argument("--min_score", type=int, default=D["min_score"], metavar="N", help="smallest score of a reported chain [40]")
    p.add_argument("--stats", default=None, metavar="FILE", help="one TSV row: reads, mapped, minimizers, anchors, stage times")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("-o", "--out", default=None, metavar="FILE", help="the PAF, or with -a the SAM [stdout]; .gz / .bgz: BGZF")
    p.add_argument("-a", dest="sam", action="store_true", help="align the primary chain base by base and write SAM")
    helps = dict(match="match score", mismatch="mismatch penalty", gap_open="gap open penalty", gap_ext="gap extension penalty",
                 band="diagonals either side of a core's corners", end_bonus="score bonus for reaching a read's end",
                 ext_max="read bases an end extension considers", max_cells="largest matrix; a read beyond it is written unmapped")
    for f, flag in ALIGN_FLAGS:
        p.add_argument(flag, dest=f, type=int, default=AD[f], metavar="N", help=f"with -a: {helps[f]} [{AD[f]}]")
    return p


def main(argv=None):
    from . import api
    from . import io as np2io
    a = build_parser().parse_args(argv)
    kw = {f: getattr(a, f) for f in np2io.MAP_DEFAULTS}
    for f, v in kw.items():
        if not 0 <= v <= 0xFFFFFFFF:
            raise SystemExit(f"Error: {f}: 0 .. 4294967295")
    k, w = kw.pop("k"), kw.pop("w")
    akw = {f: getattr(a, f) for f in np2io.ALIGN_DEFAULTS} if a.sam else {}
    for f, v in akw.items():
        if not 0 <= v <= 0xFFFFFFFF:
            raise SystemExit(f"Error: {f}: 0 .. 4294967295")
    tmp = None
    try:
        out = a.out
        if out is None:  # the library writes a file: a temporary one, copied to stdout
            fd, tmp = tempfile.mkstemp(prefix="map.", suffix=".sam" if a.sam else ".paf")
            os.close(fd)
            out = tmp
        try:
            np2io.map_opts(k=k, w=w, **kw)
            with np2io.MapIndex(a.asm, k=k, w=w, device=a.device) as ix:
                if a.sam:
                    np2io.align_opts(**akw)
                    stats = np2io.map_align_files(ix, a.reads, out, **kw, **akw)
                    align_stats = np2io.align_last_stats()
                else:
                    stats = np2io.map_files(ix, a.reads, out, **kw)
                index_ms = ix.build_ms
        except (api.Np2Error, ImportError) as e:
            raise SystemExit(f"Error: {e}")
        if tmp is not None:
            with open(tmp, "r") as f:
                shutil.copyfileobj(f, sys.stdout)
            sys.stdout.flush()
        if a.stats is not None:
            with open(a.stats, "w") as f:
                f.write(stats_row(stats, index_ms))
                if a.sam:
                    f.write(align_stats_row(align_stats))
    finally:
        if tmp is not None and os.path.exists(tmp):
            os.remove(tmp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
