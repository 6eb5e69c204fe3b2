"""Map HiFi reads to the assembly on the device: minimizer seeds chained into PAF, or with -a the primary chain aligned base
by base and written as SAM (the recipe's `winnowmap -ax` step; its SAM pipes into `python -m nextpolish2_amd.cli -`).

    python -m nextpolish2_amd.map asm.fa[.gz] hifi.fa[.gz] [more reads ...] [-o map.paf[.gz]] [-k 19] [-w 19] [--max_occ 200]
                                  [--lookback 64] [--max_gap 10000] [--bandwidth 500] [--min_cnt 3] [--min_score 40] [--stats FILE]
                                  [-a [-A 1] [-B 4] [-O 6] [-E 2] [--band 32] [--end_bonus 5] [--ext_max 2048] [--max_cells N]
                                      [--qual] [--MD] [--cs] [--eqx]]
                                  [-W repetitive_k15.txt | --rep [distinct=0.9998 | min_count=N]]
                                  [--supp] [--secondary N | -N N] [--max_chains N] [--mask_level 0.5] [--pri_ratio 0.8]

One line per mapped read, in read order: qname qlen qs qe strand tname tlen ts te matches block mapq tp:A:P cm:i: s1:i: s2:i:
(the rule: include/np2_io.h, np2_map_*; it follows minimap2's published seed-and-chain algorithm and is not pinned against
the minimap2 binary).  An output path ending in .gz / .bgz is written as BGZF, compressed on the device.

With -a: a SAM header and one line per read, in read order: qname flag rname pos mapq CIGAR * 0 0 SEQ * NM:i: AS:i: cm:i: s1:i:
s2:i: (the rule: np2_map_align_*; M, I, D and S only, gaps left-aligned; an unmapped read has flag 4).  --stats then writes a
second header and row, ALIGN_STATS_HEADER.

With -a and --qual / --MD / --cs / --eqx (the rule: np2_map_align_*, "Tags"): QUAL carries a FASTQ read's base qualities
(reversed with flag 16), MD:Z: and the short cs:Z: follow s2:i:, and M becomes = and X.  `map -a --qual --MD hifi.fastq.gz |
samsort - --full -o hifi.map.sort.bam` is the `minimap2 -a ... | samtools sort` of the reference's benchmark recipe (step 5:
the BAM a variant caller reads).  (-Q is not used: minimap2 gives it the opposite meaning.)  --stats then gains a third header
and row, TAG_STATS_HEADER.

With -W FILE (winnowmap's -W): the k-mers of the list (one a line, as python -m nextpolish2_amd.repkmers or meryl print
writes it; plain or gzip) are made less likely to win a minimizer window, so that the unique k-mers inside repeats become
the seeds (the rule: np2_map_*, "Weights"; 11 <= k <= 15).  --rep counts the assembly's own repetitive k-mers in this process
with repkmers' rule instead, and no list file is written.  With either and no -k, k is the list's (15 for --rep).

With --supp and / or --secondary N (the rule: np2_io.h, "More chains"): a read's further chains follow its primary line, a
supplementary one (another part of the read, as across a misjoin) with tp:A:P, a secondary one (the same part of the read
at another copy of a repeat) with tp:A:S, s2:i:0 and mapq 0.  --max_chains caps the selections per read, the primary among
them [1 + N + 4 with --supp, 16 at the most]; --mask_level and --pri_ratio are minimap2's, kept per mille.  With -a every
kept chain is aligned and written as a record of its own behind the read's primary: FLAG | 2048 (supplementary) or | 256
(secondary), soft clips with the full SEQ (and QUAL with --qual), and SA:Z: as the last field of a read's primary and
supplementary records when it has more than one.  `map -a --supp ... | cli - asm.fa.gz k21.yak k31.yak -s -c 100000` and
`map -a --secondary 5 --qual ... | samsort - --full -o x.bam`, then `cli x.bam ... -S -q -1`, feed the polisher's -s and -S
doors.  --stats then gains MULTI_STATS_HEADER and a row.
"""
import argparse
import os
import shutil
import sys
import tempfile

STATS_HEADER = ("reads", "mapped", "unmapped", "minimizers", "anchors", "dropped_occ", "index_minimizers", "pieces", "groups", "index_ms",
                "sketch_ms", "seed_ms", "sort_ms", "chain_ms", "read_ms", "write_ms")


WEIGHTS_HEADER = ("weights_k", "weights_listed")


def stats_row(stats, index_ms, weights=None):
    """--stats: a header line and one TSV row (counts, then times in ms with three decimals); with `weights` (k, listed) the
    columns WEIGHTS_HEADER behind them, as the command line writes it (0, 0 for an unweighted run)"""
    st = dict(stats, index_ms=index_ms)
    cells = [str(int(st[f])) for f in STATS_HEADER[:9]] + ["%.3f" % float(st[f]) for f in STATS_HEADER[9:]]
    head = STATS_HEADER
    if weights is not None:
        head, cells = head + WEIGHTS_HEADER, cells + [str(int(weights[0])), str(int(weights[1]))]
    return "\t".join(head) + "\n" + "\t".join(cells) + "\n"


def rep_arg(text):
    """argparse type of --rep [distinct=F | min_count=N] -> the keywords of api.rep_bytes"""
    key, eq, val = text.partition("=")
    try:
        if key == "distinct" and eq:
            f = float(val)
            if 0.0 <= f <= 1.0:
                return dict(distinct=f)
        elif key == "min_count" and eq and val.isdigit() and int(val) <= 0xFFFFFFFF:
            return dict(min_count=int(val))
    except ValueError:
        pass
    raise argparse.ArgumentTypeError(f"{text!r}: distinct=F with 0 <= F <= 1, or min_count=N, is expected")


def list_k(path):
    """the length of a list file's first k-mer (plain or gzip; 0 for an empty file), read without the library so that a -k that
    contradicts it is refused first; the library checks every line"""
    import gzip
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    with (gzip.open if gz else open)(path, "rb") as f:
        line = f.readline()
    return len(line.split(b"\t", 1)[0].rstrip(b"\r\n"))


def resolve_k(k, weights_k, default, flag="-k "):
    """-k beside a weight list of k-mer length weights_k (0: none or empty) -> (k, error text or None)"""
    if k is None:
        return (weights_k or default), None
    if weights_k and k != weights_k:
        return k, f"{flag}{k} contradicts the weight list, whose k-mers have {weights_k} letters (leave it out: k is the list's)"
    return k, None


REP_K = 15  # --rep without -k: the recipe's meryl k

ALIGN_STATS_HEADER = ("pins", "segments", "equal", "pure_gap", "snv", "cores", "cells", "clipped_bases", "overflow", "pins_ms",
                      "classify_ms", "dp_ms", "assemble_ms", "write_ms")
ALIGN_FLAGS = (("match", "-A"), ("mismatch", "-B"), ("gap_open", "-O"), ("gap_ext", "-E"), ("band", "--band"), ("end_bonus", "--end_bonus"),
               ("ext_max", "--ext_max"), ("max_cells", "--max_cells"))


def align_stats_row(stats):
    """--stats with -a: a second header line and TSV row (counts, then times in ms with three decimals)"""
    cells = [str(int(stats[f])) for f in ALIGN_STATS_HEADER[:9]] + ["%.3f" % float(stats[f]) for f in ALIGN_STATS_HEADER[9:]]
    return "\t".join(ALIGN_STATS_HEADER) + "\n" + "\t".join(cells) + "\n"


TAG_STATS_HEADER = ("md_bytes", "cs_bytes", "eqx_words", "qual_reads", "tags_ms")
TAG_FLAGS = (("qual", "--qual"), ("md", "--MD"), ("cs", "--cs"), ("eqx", "--eqx"))


def tag_stats_row(stats):
    """--stats with -a and one of TAG_FLAGS: a third header line and TSV row"""
    cells = [str(int(stats[f])) for f in TAG_STATS_HEADER[:4]] + ["%.3f" % float(stats["tags_ms"])]
    return "\t".join(TAG_STATS_HEADER) + "\n" + "\t".join(cells) + "\n"


MULTI_STATS_HEADER = ("units", "selections", "dropped_min_cnt", "dropped_secondary", "kept_supplementary", "kept_secondary", "overflow_units",
                      "more_ms")


def multi_stats_row(stats):
    """--stats with --supp / --secondary / --max_chains: a further header line and TSV row"""
    cells = [str(int(stats[f])) for f in MULTI_STATS_HEADER[:7]] + ["%.3f" % float(stats["more_ms"])]
    return "\t".join(MULTI_STATS_HEADER) + "\n" + "\t".join(cells) + "\n"


def per_mille(text):
    """argparse type of --mask_level / --pri_ratio: a fraction in 0 .. 1, converted once to per mille by rounding"""
    try:
        f = float(text)
    except ValueError:
        f = -1.0
    if not 0.0 <= f <= 1.0:
        raise argparse.ArgumentTypeError(f"{text!r}: a fraction in 0 .. 1 is expected")
    return int(f * 1000.0 + 0.5)


def multi_of(a):
    """the parsed arguments -> the multi-chain options as a dict, or None when none of them was given (the plain doors)"""
    from .io import MULTI_DEFAULTS, multi_chains_default
    if not a.supp and a.secondary is None and a.max_chains is None and a.mask_level is None and a.pri_ratio is None:
        return None
    n = a.secondary or 0
    cap = a.max_chains
    if cap is None:
        cap = multi_chains_default(a.supp, n) if (a.supp or a.secondary is not None) else MULTI_DEFAULTS["max_chains"]
    return dict(max_chains=cap, supplementary=int(a.supp), secondary_n=n,
                mask_pm=MULTI_DEFAULTS["mask_pm"] if a.mask_level is None else a.mask_level,
                pri_pm=MULTI_DEFAULTS["pri_pm"] if a.pri_ratio is None else a.pri_ratio)


def build_parser():
    from .io import ALIGN_DEFAULTS as AD
    from .io import MAP_DEFAULTS as D
    p = argparse.ArgumentParser(prog="nextpolish2_amd.map", description="map long reads to an assembly: minimizer seeds and chains to PAF")
    p.add_argument("asm", metavar="asm.fa[.gz]", help="assembly in [GZIP] FASTA format")
    p.add_argument("reads", nargs="+", metavar="hifi.fa[.gz]", help="reads in [GZIP] FASTA / FASTQ format")
    p.add_argument("-k", type=int, default=None, metavar="K", help="k-mer size, 11 .. 28 [19; with -W the list's; with --rep 15]")
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
    p.add_argument("--qual", dest="qual", action="store_true", help="with -a: write a FASTQ read's base qualities as QUAL")
    p.add_argument("--MD", dest="md", action="store_true", help="with -a: write the MD:Z: tag")
    p.add_argument("--cs", dest="cs", action="store_true", help="with -a: write the short cs:Z: tag")
    p.add_argument("--eqx", dest="eqx", action="store_true", help="with -a: write = and X in place of M")
    g = p.add_mutually_exclusive_group()
    g.add_argument("-W", dest="weights", default=None, metavar="FILE",
                   help="down-weight the k-mers of this list in minimizer sampling (winnowmap -W; one k-mer a line, [GZIP]; 11 <= k <= 15)")
    g.add_argument("--rep", nargs="?", const=dict(distinct=0.9998), default=None, type=rep_arg, metavar="distinct=F|min_count=N",
                   help="down-weight the assembly's own repetitive k-mers, counted here with repkmers' rule [distinct=0.9998]")
    p.add_argument("--supp", action="store_true", help="report supplementary chains: other parts of the read (tp:A:P)")
    p.add_argument("--secondary", "-N", dest="secondary", type=int, default=None, metavar="N",
                   help="report up to N secondary chains per parent: the same part of the read elsewhere (tp:A:S), 0 .. 15 [0]")
    p.add_argument("--max_chains", type=int, default=None, metavar="N", help="selections per read, the primary among them, 1 .. 16 [1 + N + 4 with --supp]")
    p.add_argument("--mask_level", type=per_mille, default=None, metavar="F", help="a chain that overlaps a parent by more than F of the shorter is secondary [0.5]")
    p.add_argument("--pri_ratio", type=per_mille, default=None, metavar="F", help="keep a secondary chain that scores F of its parent or more [0.8]")
    return p


def main(argv=None):
    from . import api
    from . import io as np2io
    parser = build_parser()
    a = parser.parse_args(argv)
    tags = {f: getattr(a, f) for f, _ in TAG_FLAGS}
    for f, flag in TAG_FLAGS:
        if tags[f] and not a.sam:
            parser.error(f"{flag} needs -a (it is an output of the base-level alignment)")
    multi = multi_of(a)
    if multi is not None:
        for f, v in multi.items():
            if not 0 <= v <= 0xFFFFFFFF:
                raise SystemExit(f"Error: {f}: 0 .. 4294967295")
    wk = 0
    if a.weights is not None:
        try:
            wk = list_k(a.weights)
        except OSError as e:
            raise SystemExit(f"Error: -W: {e}")
    elif a.rep is not None:
        wk = REP_K if a.k is None else a.k  # (the k-mers are counted at the k that is mapped with)
    a.k, bad = resolve_k(a.k, wk, np2io.MAP_DEFAULTS["k"])
    if bad:
        raise SystemExit(f"Error: {bad}")
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
            multi_stats = None
            weights = None
            if a.weights is not None:
                weights = np2io.MapWeights(a.weights)
            elif a.rep is not None:
                weights = np2io.MapWeights.from_assembly(a.asm, k=k, device=a.device, **a.rep)
            with np2io.MapIndex(a.asm, k=k, w=w, device=a.device, weights=weights) as ix:
                if weights is not None:
                    weights.close()
                if a.sam:
                    np2io.align_opts(**akw)
                    stats = np2io.map_align_files(ix, a.reads, out, multi=multi, **tags, **kw, **akw)
                    if multi is not None:
                        multi_stats = np2io.map_last_multi_stats()
                    align_stats = np2io.align_last_stats()
                    tag_stats = np2io.align_last_tag_stats() if any(tags.values()) else None
                else:
                    stats = np2io.map_files(ix, a.reads, out, multi=multi, **kw)
                    if multi is not None:
                        multi_stats = np2io.map_last_multi_stats()
                index_ms, wstats = ix.build_ms, (ix.weights_k, ix.weights_listed)
        except (api.Np2Error, ImportError) as e:
            raise SystemExit(f"Error: {e}")
        if tmp is not None:
            with open(tmp, "r") as f:
                shutil.copyfileobj(f, sys.stdout)
            sys.stdout.flush()
        if a.stats is not None:
            with open(a.stats, "w") as f:
                f.write(stats_row(stats, index_ms, wstats))
                if a.sam:
                    f.write(align_stats_row(align_stats))
                    if tag_stats is not None:
                        f.write(tag_stats_row(tag_stats))
                if multi_stats is not None:
                    f.write(multi_stats_row(multi_stats))
    finally:
        if tmp is not None and os.path.exists(tmp):
            os.remove(tmp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
