"""nextPolish2 command line mirror (src/utils/option.rs:45-292, src/main.rs:1689-1856).

Usage: nextPolish2 [OPTIONS] <HiFi.map.bam|HiFi.map.sam[.gz]|-> <genome.fa[.gz]> <short.read.yak>...
Same positionals, flags, defaults and output format as the reference; contigs are polished on the GPU and written in
input order.  The first positional may also be the mapper's SAM text, unsorted (plain or gzip, any name; `-` is standard
input): it is parsed and coordinate-sorted on the GPU (io.Sam), so no samtools sort / index step is needed.  `-t N` (N >= 2) keeps two front ends (BGZF inflate + record walk on the host pool or the device, GPU
columnariser) and two polish workers going side by side; a worker polishes the contigs that are resident by its turn as
ONE batch (np2_batch_polish: one launch per pipeline step for all of them), and the host-side phases of one batch (the
phasing vote's Louvain) overlap the GPU phases of the other; the k-mer dumps are streamed into their HBM tables next to
the first front ends."""
import argparse
import os
import resource
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import io as np2io
from ._types import Opts
from .api import Np2Error, Polisher, fasta_record

VERSION = "np2-mi355x 0.1 (reference semantics: NextPolish2 v0.2.2)"


def _existing(path):
    p = os.path.abspath(path)
    if not os.path.exists(p):
        raise argparse.ArgumentTypeError(f"{p!r} does not exist!")
    return p


def _existing_or_stdin(path):
    return path if path == "-" else _existing(path)


def _map_len(v):
    """-a INT.FLOAT parsed as f32 like the reference (option.rs:232 remove_one::<f32>)."""
    return np.float32(v)


def split_map_len(v):
    """(min_map_len, min_map_fra) = (f32 as usize, f32::fract()) (option.rs:258-259): both in single precision, so
    `-a 500.3` gives fra = 0.29998779 (not 0.3) and (rlen as f32 * fra) as i64 matches the reference to the unit."""
    f = np.float32(v)
    return int(f), float(np.float32(f - np.trunc(f)))


def build_parser():
    p = argparse.ArgumentParser(prog="nextPolish2", description="Repeat-aware polishing genomes assembled using HiFi long reads")
    p.add_argument("bam", type=_existing_or_stdin, metavar="HiFi.map.bam",
                   help="HiFi-to-ref mapping file in sorted BAM format, or the mapper's SAM text, unsorted ([GZIP]; - is standard input)")
    p.add_argument("--sam_tie", choices=np2io.SAM_TIES, default="strand",
                   help="SAM input: records at one position are ordered by strand, as samtools sort orders them, or stay in input order [strand]")
    p.add_argument("--from_reads", action="store_true",
                   help="the first positional is the HiFi reads themselves ([GZIP] FASTA or FASTQ; not sniffed: give the flag): they are "
                        "mapped and aligned against genome.fa on the GPU and the records stay there, no SAM text is written or read "
                        "(what `python -m nextpolish2_amd.map -a` piped into this program computes, in one process; --sam_tie and "
                        "--sorted_bam work, no -S, no --sorted_bam_full, single rank)")
    p.add_argument("--more_reads", type=_existing, action="append", default=[], metavar="FILE",
                   help="--from_reads: a further read file behind the first (repeatable)")
    p.add_argument("--map_opts", type=np2io.map_opts_arg, default={}, metavar="KEY=VAL,...",
                   help="--from_reads: mapper and aligner options, the keys of python -m nextpolish2_amd.map (" +
                        " ".join(list(np2io.MAP_DEFAULTS) + list(np2io.ALIGN_DEFAULTS)) + ")")
    p.add_argument("--map_weights", default=None, metavar="FILE|auto",
                   help="--from_reads: down-weight repetitive k-mers in the mapper's minimizer sampling (winnowmap -W): a list file as "
                        "python -m nextpolish2_amd.repkmers writes it, or `auto`: the assembly's own, counted here (distinct=0.9998, "
                        "k = 15); without k in --map_opts, k is the list's")
    p.add_argument("fa", type=_existing, metavar="genome.fa[.gz]", help="genome assembly file in [GZIP] FASTA format")
    p.add_argument("yak", type=_existing, nargs="*", metavar="short.read.yak", help="one or more k-mer dataset in yak format")
    p.add_argument("--sr", type=_existing, action="append", default=[], metavar="FILE",
                   help="short reads (FASTA / FASTQ[.gz]; may repeat): count their k-mers on the GPU instead of reading yak dumps")
    p.add_argument("--sr_k", default="21,31", metavar="K[,K...]", help="k-mer sizes counted from --sr [21,31]")
    p.add_argument("--sr_min_count", type=int, default=None, metavar="N",
                   help="drop k-mers of --sr counted fewer than N times [2, or -k/--min_kmer_count where that is smaller]")
    p.add_argument("--sr_qc", nargs="?", const=np2io.SrQc(), default=None, type=np2io.sr_qc_arg, metavar="SPEC",
                   help="with --sr: " + np2io.SR_QC_HELP)
    p.add_argument("--sr_adapter", nargs="?", const="", default=None, type=np2io.sr_adapter_arg, metavar="SPEC",
                   help="with --sr: " + np2io.SR_ADAPTER_HELP)
    p.add_argument("-o", "--out", default=None, metavar="FILE", help="output file [stdout]")
    p.add_argument("--qv", default=None, metavar="FILE",
                   help="k-mer QV of every contig as read and as written, per k-mer table, as a TSV (a k-mer the tables do not "
                        "hold is an error; tables without singletons call singletons absent)")
    p.add_argument("--qv_min_count", type=int, default=1, metavar="N", help="--qv reads a k-mer count below N as absent [1]")
    p.add_argument("--qv_bed", default=None, metavar="PREFIX",
                   help="with --qv: intervals covered by absent k-mers, PREFIX.k<K>.in.bed and PREFIX.k<K>.out.bed")
    p.add_argument("--cmp", default=None, metavar="FILE",
                   help="k-mer completeness of the assembly as read and as written, per k-mer table, as a TSV (the share of "
                        "the reliable read k-mers the assembly holds)")
    p.add_argument("--cmp_min_count", type=int, default=2, metavar="N", help="--cmp: a read k-mer counted at least N times is reliable [2]")
    p.add_argument("--cmp_spectra", default=None, metavar="PREFIX",
                   help="with --cmp: copy-number spectra, PREFIX.k<K>.in.tsv and PREFIX.k<K>.out.tsv")
    p.add_argument("--trio", default=None, metavar="FILE",
                   help="switch and Hamming error of every contig as read and as written against parental k-mer tables, as a TSV "
                        "(needs --trio_pat and --trio_mat)")
    p.add_argument("--trio_pat", type=_existing, default=None, metavar="pat.yak", help="--trio: the paternal k-mer dump")
    p.add_argument("--sorted_bam", default=None, metavar="hifi.map.sort.bam",
                   help="SAM input: also write the coordinate-sorted BAM and its .bai (what samtools sort and index would make of "
                        "the mapping), assembled, compressed and indexed on the GPU; single rank")
    p.add_argument("--bam_unsorted", action="store_true",
                   help="the BAM given is read whole, inflated, unpacked and coordinate-sorted on the GPU, as SAM text is: it need "
                        "not be sorted and no .bai is read; what holds for SAM input holds (--sorted_bam allowed, no -S, single rank)")
    p.add_argument("--sorted_bam_full", action="store_true",
                   help="--sorted_bam: carry QUAL, RNEXT, PNEXT, TLEN, the optional fields and the header lines (@RG, @PG, @CO) too; "
                        "about three times the device memory for the resident mapping")
    p.add_argument("--trio_mat", type=_existing, default=None, metavar="mat.yak", help="--trio: the maternal k-mer dump (same k)")
    p.add_argument("--trio_min_count", type=int, default=2, metavar="N", help="--trio: a parent counting a k-mer fewer than N times does not have it [2]")
    p.add_argument("--trio_mid_count", type=int, default=5, metavar="N", help="--trio: a parent counting a k-mer at least N times has it [5]")
    p.add_argument("--trio_bed", default=None, metavar="PREFIX", help="with --trio: switch sites, PREFIX.in.bed and PREFIX.out.bed")
    p.add_argument("--edits", default=None, metavar="FILE.vcf",
                   help="what the polish changed: the edits of every polished contig as VCF 4.2, left-aligned, each with the k-mer "
                        "tables' verdict (regions rewritten the same are no edits)")
    p.add_argument("--edits_summary", default=None, metavar="FILE.tsv", help="edits per contig and kind, bases inserted and deleted, verdicts")
    p.add_argument("--edits_min_count", type=int, default=1, metavar="N", help="--edits reads a k-mer count below N as absent [1]")
    p.add_argument("-u", "--uppercase", action="store_true", help="output in uppercase sequences")
    p.add_argument("--out_pos", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("-k", "--min_kmer_count", type=int, default=5)
    p.add_argument("-t", "--thread", type=int, default=1, help="contigs in flight on the GPU (1-4 np2 contexts)")
    p.add_argument("-i", "--iter_count", type=int, default=2)
    p.add_argument("-m", "--model", default="ref", type=str, help="ref|len (case-insensitive)")
    p.add_argument("-l", "--min_read_len", type=int, default=1000)
    p.add_argument("-L", "--min_ctg_len", type=int, default=1000000)
    p.add_argument("-n", "--max_indel_len", type=int, default=20)
    p.add_argument("-s", "--use_supplementary", action="store_true")
    p.add_argument("-S", "--use_secondary", action="store_true")
    p.add_argument("-a", "--min_map_len", type=_map_len, default=500.5, metavar="INT.FLOAT")
    p.add_argument("-q", "--min_map_qual", type=int, default=1)
    p.add_argument("-c", "--max_clip_len", type=int, default=100)
    p.add_argument("-r", "--use_all_reads", action="store_true")
    p.add_argument("--min_base_cov", type=int, default=1, help=argparse.SUPPRESS)
    p.add_argument("--device", type=int, default=None, help="HIP device index [LOCAL_RANK, else 0]")
    p.add_argument("--shard_min_len", type=int, default=32_000_000,
                   help="under torchrun: contigs at least this long are cut into one reference interval per rank "
                        "(shorter ones go to one rank each)")
    p.add_argument("--shard_halo", type=int, default=65536, help="reads overlapping a rank's interval widened by this are held")
    p.add_argument("--dist_backend", default=None, help="torch.distributed backend under torchrun [nccl]")
    p.add_argument("-V", "--version", action="version", version=VERSION)
    return p


def _report_sr_qc(a):
    """the filter's totals as one [INFO] line (on the thread that counted: the totals are that thread's)"""
    if a.sr_adapter is not None:
        print(f"[INFO] sr_adapter: {np2io.sradapt_stats_text(np2io.sradapt_last_stats())}", file=sys.stderr)
    elif a.sr_qc is not None:
        print(f"[INFO] sr_qc: {np2io.srqc_stats_text(np2io.srqc_last_stats())}", file=sys.stderr)


def _cpu_seconds():
    ru = resource.getrusage(resource.RUSAGE_SELF)
    return ru.ru_utime + ru.ru_stime


def resource_str(t0, argv, cpu0=0.0):
    ru = resource.getrusage(resource.RUSAGE_SELF)
    return (f"[INFO] Version: {VERSION}\n[INFO] CMD: {' '.join(argv)}\n[INFO] Real time: {time.time() - t0:.3f} sec; "
            f"CPU: {ru.ru_utime + ru.ru_stime - cpu0:.3f} sec; Peak RSS: {ru.ru_maxrss / 1048576:.3f} GB")


def _record(a, name, b, first, last, pos=None):
    if a.uppercase:
        b = b.upper()
    if a.out_pos:
        return b"".join(b"%s\t%c\t%d\n" % (name.encode(), b[i:i + 1], int(pos[i])) for i in range(len(b)))
    return b">%s start:%d end:%d\n%s\n" % (name.encode(), first, last, b)


def _record_sequence(rec):
    """the sequence of a FASTA record as written: '>name start:a end:b\\nSEQ\\n'"""
    return rec[rec.index(b"\n") + 1:-1]


def table_ks(a):
    """the k of every table the reports measure against, in table order"""
    return a.sr_ks if a.sr else sorted(np2io.check_yak_header(y) for y in a.yak)


def _qv_report(a, ks):
    from .qv import QvReport
    return QvReport(ks, a.qv_min_count, want_bed=a.qv_bed is not None)


def _cmp_report(a, ks):
    from .completeness import CmpReport
    return CmpReport(ks, a.cmp_min_count, want_spectra=a.cmp_spectra is not None)


def _cmp_finish(a, creport, pol, seqs_in, seqs_out):
    """--cmp: the whole assembly as read and as written, one call per side and table, after the last contig"""
    creport.add(pol, "in", seqs_in)
    creport.add(pol, "out", seqs_out)
    creport.write_cli(a.cmp, a.cmp_spectra)


def _edits_report(a, ks):
    from .edits import EditsReport
    return EditsReport(ks, a.edits_min_count)


def _trio_report(a):
    from .trio import TrioReport
    return TrioReport(a.trio_k, a.trio_min_count, a.trio_mid_count, want_bed=a.trio_bed is not None)


def _trio_polisher(a):
    """a context of its own that holds the two parental tables: paternal 0, maternal 1 (dumps of one k keep their order)"""
    return np2io.polisher_from_yak_files([a.trio_pat, a.trio_mat], device=a.device)


def _init_distributed(a):
    """torch.distributed process group of a torchrun launch, then the one decision that is rank 0's alone — may the
    output file be written (option.rs:312-316) — shared with every rank.  Returns rank 0's output stream (None elsewhere)."""
    import torch
    import torch.distributed as dist

    from .dist import all_gather_arrays
    rank = int(os.environ["RANK"])
    backend = a.dist_backend or "nccl"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend == "nccl":
        dev_idx = a.device % max(1, torch.cuda.device_count())
        torch.cuda.set_device(dev_idx)
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev_idx))
        xdev = torch.device("cuda", dev_idx)
    else:
        dist.init_process_group(backend=backend)
        xdev = torch.device("cpu")
    out, verdict = None, b""
    if rank == 0:
        out = sys.stdout.buffer
        if a.out is not None and a.out != "stdout":
            path = os.path.abspath(a.out)
            if os.path.exists(path):
                verdict = f"Error: {path!r} already exists!".encode()
            else:
                try:
                    out = _open_out(path, a.device % max(1, torch.cuda.device_count()))
                except SystemExit as e:  # (the other ranks must learn of it)
                    verdict = str(e).encode()
    got = all_gather_arrays(np.frombuffer(verdict, dtype=np.uint8), device=xdev)
    if len(got[0]):
        dist.destroy_process_group()
        raise SystemExit(got[0].tobytes().decode())
    return out


def _open_out(path, device):
    """the output FASTA: a path ending in .gz or .bgz is written as BGZF, compressed on `device`; any other as plain bytes"""
    if np2io.is_bgzf_path(path):
        try:
            return np2io.BgzfWriter(path, device=device)
        except Np2Error as e:
            raise SystemExit(f"Error: {e}")
    return open(path, "wb")


def _main_distributed(a, argv, t0, out, yaks, opts, fopts):
    """One process per GPU (torchrun): the assembly is polished by all ranks and written by rank 0 in input order.

    Contigs of at least --shard_min_len are cut into one reference interval per rank (np2_shard_*: votes all-gathered and
    decided contig-wide per phasing pass, pieces all-gathered and stitched); the others go whole to one rank each,
    longest first (the reference's unit of work, main.rs:1726-1837).  The only collectives are the small vote exchange
    and the all-gather of polished sequences (RCCL over xGMI with the default backend)."""
    import torch
    import torch.distributed as dist

    from .dist import ShardMismatch, all_gather_arrays, all_gather_sequences, assign_contigs, polish_sharded_bam
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    backend = a.dist_backend or "nccl"
    dev_idx = a.device % max(1, torch.cuda.device_count())
    xdev = torch.device("cuda", dev_idx) if backend == "nccl" else torch.device("cpu")  # (group: _init_distributed)
    pol = Polisher(yaks, device=dev_idx)
    bam = np2io.Bam(a.bam)
    contigs = list(np2io.read_fasta(a.fa))  # every rank reads the assembly (cheap next to the BAM)
    records = {}
    for name, seq in contigs:  # main.rs:1707-1711, for every contig whichever way it is polished
        if len(seq) >= 0xFFFFFFFF:
            raise SystemExit(f"{name} is too long!")
    long_ones = [i for i, (_, seq) in enumerate(contigs) if len(seq) >= max(a.min_ctg_len, a.shard_min_len)]
    whole = [i for i, (_, seq) in enumerate(contigs) if len(seq) >= a.min_ctg_len and i not in set(long_ones)]
    # 1. long contigs: one reference interval per rank
    for i in long_ones:
        name, seq = contigs[i]
        try:  # every rank parses only the BAM records overlapping its interval +- halo; the pieces meet on rank 0
            b, p, span = polish_sharded_bam(pol, bam, name, seq, opts, fopts, halo=a.shard_halo, device=xdev,
                                            want_pos=a.out_pos, dst=0, with_span=True)
        except ShardMismatch as e:
            # raised on every rank alike (every exchange carries the ranks' status; the strips around the cuts are seen by
            # all): the shards disagree, a splice cursor got stuck inside one (NP2_E_UNSUPPORTED), or one failed for a
            # reason of its own -> rank 0 polishes the contig unsharded (and reports a genuine error itself)
            print(f"[WARN] {name}: {e}; polishing it unsharded", file=sys.stderr)
            b, fb_err = None, None
            if rank == 0:
                try:
                    c = np2io.contig_from_bam(pol, bam, name, seq, fopts)
                    try:
                        b, p = pol.polish_resident(c, opts, want_pos=a.out_pos)
                        span = (int(p[0]), int(p[-1])) if a.out_pos else (p[0], p[1])
                    finally:
                        c.free()
                except Exception as e2:  # noqa: BLE001 — the other ranks wait below: they must learn of it
                    fb_err = e2
            # a genuine error on rank 0 ends the run on every rank (nobody is left waiting in the next contig's collective)
            verdict = all_gather_arrays(np.array([0 if fb_err is None else 1], dtype=np.uint8), device=xdev)
            if int(verdict[0][0]):
                dist.destroy_process_group()
                raise SystemExit(f"Error: {name}: {fb_err if fb_err is not None else 'the unsharded fallback failed on rank 0'}")
        if rank == 0:
            records[i] = _record(a, name, np.asarray(b).tobytes(), int(span[0]), int(span[1]), p if a.out_pos else None)
    # 2. the other contigs: whole, one rank each, longest first
    mine = assign_contigs([len(contigs[i][1]) for i in whole], world)[rank]
    local = []
    for k in mine:
        i = whole[k]
        name, seq = contigs[i]
        c = np2io.contig_from_bam(pol, bam, name, seq, fopts)
        try:
            bases, pos = pol.polish_resident(c, opts, want_pos=a.out_pos)
        finally:
            c.free()
        b = bases.tobytes()
        local.append((i, _record(a, name, b, *( (int(pos[0]), int(pos[-1]), pos) if a.out_pos else (pos[0], pos[1], None)))))
    got = all_gather_sequences(local, device=xdev)
    if rank == 0:
        records.update(got)
        report, qpol = None, None
        if a.qv is not None:  # rank 0 measures what it writes, on its own device and a context of its own
            report, qpol = _qv_report(a, [y.k for y in yaks]), pol.clone()
        treport, tpol = None, None
        if a.trio is not None:
            treport, tpol = _trio_report(a), _trio_polisher(a)
        creport, cmp_in, cmp_out = None, [], []
        if a.cmp is not None:
            creport = _cmp_report(a, [y.k for y in yaks])
        for i, (name, seq) in enumerate(contigs):
            if i in records:
                rec = records[i]
            else:  # pass-through (main.rs:1727-1730)
                s_ = seq.upper() if a.uppercase else seq
                rec = _record(a, name, s_, 0, len(seq) - 1, range(len(seq)))
            out.write(rec)
            if report is not None:
                report.add(qpol, name, seq, _record_sequence(rec))
            if treport is not None:
                treport.add(tpol, name, seq, _record_sequence(rec))
            if creport is not None:
                cmp_in.append(seq)
                cmp_out.append(_record_sequence(rec))
        out.flush()
        if report is not None:
            qpol.close()
            report.write_cli(a.qv, a.qv_bed)
        if creport is not None:
            cpol = pol.clone()
            try:
                _cmp_finish(a, creport, cpol, cmp_in, cmp_out)
            finally:
                cpol.close()
        if treport is not None:
            tpol.close()
            treport.write_cli(a.trio, a.trio_bed)
        if out is not sys.stdout.buffer:
            out.close()
        print(resource_str(t0, ["nextPolish2"] + argv), file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    t0 = time.time()
    cpu0 = _cpu_seconds()  # (main() may run inside a longer-lived process: report this call's CPU time, not the process's)
    parser = build_parser()
    a = parser.parse_args(argv)
    if not a.sr and not a.yak:  # (what nargs="+" said before --sr made the positional optional)
        parser.error("the following arguments are required: short.read.yak")
    if a.sr and a.yak:
        parser.error("give either short.read.yak files or --sr reads, not both")
    if a.sr_qc is not None and not a.sr:
        parser.error("--sr_qc filters the reads of --sr: give --sr")
    if a.sr_adapter is not None and not a.sr:
        parser.error("--sr_adapter trims the reads of --sr: give --sr")
    np2io.check_sr_adapter(parser, a.sr_adapter, a.sr)
    if a.sr:
        a.sr_ks = np2io.sr_k_arg(parser, a.sr_k)
        if not a.sr_ks or any(k < 2 or k >= 32 for k in a.sr_ks):
            parser.error("--sr_k: only 2 <= k < 32 is supported")
        if a.sr_min_count is None:  # no word the polish would look at is ever dropped
            a.sr_min_count = max(1, min(2, a.min_kmer_count))
    if a.qv is not None and a.out_pos:
        parser.error("--qv measures the sequences of a FASTA output: not with --out_pos")
    if a.qv_bed is not None and a.qv is None:
        parser.error("--qv_bed needs --qv")
    if not 0 <= a.qv_min_count <= 1023:
        parser.error("--qv_min_count: 0 .. 1023")
    if a.cmp is not None and a.out_pos:
        parser.error("--cmp measures the sequences of a FASTA output: not with --out_pos")
    if a.cmp_spectra is not None and a.cmp is None:
        parser.error("--cmp_spectra needs --cmp")
    if not 0 <= a.cmp_min_count <= 1023:
        parser.error("--cmp_min_count: 0 .. 1023")
    if a.trio is not None and (a.trio_pat is None or a.trio_mat is None):
        parser.error("--trio needs both --trio_pat and --trio_mat")
    if a.trio_bed is not None and a.trio is None:
        parser.error("--trio_bed needs --trio")
    if a.trio is not None and a.out_pos:
        parser.error("--trio measures the sequences of a FASTA output: not with --out_pos")
    if not 1 <= a.trio_min_count <= a.trio_mid_count <= 1023:
        parser.error("--trio thresholds: 1 <= --trio_min_count <= --trio_mid_count <= 1023")
    a.want_edits = a.edits is not None or a.edits_summary is not None
    if a.want_edits and a.out_pos:
        parser.error("--edits reports on a FASTA output: not with --out_pos (python -m nextpolish2_amd.edits reads an --out_pos text)")
    if a.want_edits and int(os.environ.get("WORLD_SIZE", "1")) > 1 and "RANK" in os.environ:
        parser.error("--edits runs on one rank: not under torchrun")
    if not 0 <= a.edits_min_count <= 1023:
        parser.error("--edits_min_count: 0 .. 1023")
    if a.model.lower() not in ("ref", "len"):
        raise SystemExit("error: invalid value for --model (ref|len)")
    if (a.more_reads or a.map_opts) and not a.from_reads:
        parser.error("--more_reads and --map_opts go with --from_reads")
    if a.map_weights is not None and not a.from_reads:
        parser.error("--map_weights goes with --from_reads")
    if a.map_weights is not None:  # the mapper's k rule (python -m nextpolish2_amd.map, -W and --rep), before any device work
        from . import map as np2mapcli
        wk = np2mapcli.REP_K if "k" not in a.map_opts else a.map_opts["k"]
        if a.map_weights != "auto":
            try:
                wk = np2mapcli.list_k(a.map_weights)
            except OSError as e:
                raise SystemExit(f"Error: --map_weights: {e}")
        k, bad = np2mapcli.resolve_k(a.map_opts.get("k"), wk, np2io.MAP_DEFAULTS["k"], flag="--map_opts k=")
        if bad:
            raise SystemExit(f"Error: {bad}")
        a.map_opts = dict(a.map_opts, k=k)
    if a.from_reads:  # every refusal before any device work, one line each
        if a.bam == "-":
            raise SystemExit("Error: --from_reads takes read files, not standard input: its reader threads open each file themselves")
        if a.bam_unsorted:
            raise SystemExit("Error: --bam_unsorted says how a BAM is read; --from_reads gives reads, not a mapping")
        if a.sorted_bam_full:
            raise SystemExit("Error: --sorted_bam_full needs the SAM text (NM, AS, cm, s1, s2 are not kept with --from_reads): write it with "
                             "python -m nextpolish2_amd.map -a -o map.sam.gz, then python -m nextpolish2_amd.samsort --full")
        if a.use_secondary:
            raise SystemExit("Error: -S needs secondary records, and the mapper behind --from_reads writes primary ones only ; write them "
                             "with python -m nextpolish2_amd.map -a --secondary 5 --qual ... | python -m nextpolish2_amd.samsort - --full -o x.bam, "
                             "then polish with x.bam ... -S -q -1")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 and "RANK" in os.environ:
            raise SystemExit("Error: --from_reads runs on one rank: interval sharding reads the .bai of a sorted BAM")
        a.sam = True  # the handle is an ordinary resident SAM: every rule of SAM input below holds
    else:
        try:  # (a look at the file's first bytes; standard input cannot be looked at twice and is SAM text)
            a.sam = a.bam == "-" or np2io.mapping_kind(a.bam) == "sam"
        except (ValueError, OSError) as e:
            raise SystemExit(f"Error: {e}")
    if a.bam_unsorted:
        if a.sam:
            raise SystemExit("Error: --bam_unsorted says how a BAM is read; the mapping given is SAM text")
        a.sam = True  # through the same door (io.Sam sniffs the file): every rule of SAM input below holds
    if a.sam and a.use_secondary:
        raise SystemExit("Error: -S needs the SEQ of a read's primary record, which is found by name: not with SAM input, use a sorted BAM "
                         "(python -m nextpolish2_amd.samsort writes one from the SAM text)")
    if a.sorted_bam_full and a.sorted_bam is None:
        raise SystemExit("Error: --sorted_bam_full says what --sorted_bam PATH carries: give --sorted_bam too")
    if a.sorted_bam is not None and not a.sam:
        raise SystemExit("Error: --sorted_bam writes the sorted BAM of SAM input; the mapping given is a BAM already")
    if a.sam and int(os.environ.get("WORLD_SIZE", "1")) > 1 and "RANK" in os.environ:
        raise SystemExit("Error: SAM input runs on one rank: interval sharding reads the .bai of a sorted BAM")
    for y in a.yak:  # (before the output file exists: a broken dump must not leave a partial output behind)
        try:
            np2io.check_yak_header(y)
        except (ValueError, OSError) as e:  # (a malformed dump, or one that cannot be read at all)
            raise SystemExit(f"Error: {e}")
    if a.trio is not None:
        from .trio import parental_k
        try:
            a.trio_k = parental_k(a.trio_pat, a.trio_mat)
        except (ValueError, OSError) as e:
            raise SystemExit(f"Error: {e}")
    out = sys.stdout.buffer
    distributed = int(os.environ.get("WORLD_SIZE", "1")) > 1 and "RANK" in os.environ
    if distributed:
        # under torchrun only rank 0 writes, and whether it may is settled together (a rank that left on its own before
        # the process group exists would leave the others waiting for it): _main_distributed opens the file
        out = None
    elif a.out is not None and a.out != "stdout":  # option.rs:76-79: the literal default "stdout" means stdout
        path = os.path.abspath(a.out)
        if os.path.exists(path):  # option.rs:312-316: refuse to overwrite
            raise SystemExit(f"Error: {path!r} already exists!")
        out = _open_out(path, a.device or 0)
    prof = os.environ.get("NP2_CLI_PROFILE")
    if a.device is None:
        a.device = int(os.environ.get("LOCAL_RANK", "0")) if distributed else 0
    if distributed:
        import torch
        from .dist import note_ranks_per_device
        note_ranks_per_device(int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))), torch.cuda.device_count())
        out = _init_distributed(a)  # process group first; the output-file verdict is rank 0's, shared with everyone
    # main.rs:1547 compares the raw option with "ref" (case-sensitive)
    opts = Opts(min_kmer_count=a.min_kmer_count, max_indel_len=a.max_indel_len, iter_count=a.iter_count,
                model=a.model, use_all_reads=a.use_all_reads)
    map_len, map_fra = split_map_len(a.min_map_len)
    fopts = np2io.FrontOpts(min_read_len=a.min_read_len, min_map_len=map_len,
                            min_map_fra=map_fra, min_map_qual=a.min_map_qual,
                            max_clip_len=a.max_clip_len, use_supplementary=a.use_supplementary,
                            use_secondary=a.use_secondary)

    def load_yaks():
        t_y = time.time()
        if a.sr:  # (under torch.distributed.run every rank counts for itself: the tables are replicated per GPU anyway)
            ys = np2io.count_kmers(a.sr, a.sr_ks, min_count=a.sr_min_count, device=a.device, qc=a.sr_qc, ad=a.sr_adapter)
            _report_sr_qc(a)
            return ys
        with ThreadPoolExecutor(max_workers=max(1, len(a.yak))) as ex:  # (the loader runs outside the GIL: one thread per dump)
            ys = sorted(ex.map(np2io.load_yak, a.yak), key=lambda y: y.k)  # option.rs:238
        if prof:
            print(f"[np2 profile] yak files loaded {time.time() - t_y:.3f} s (at +{time.time() - t0:.3f} s)", file=sys.stderr)
        return ys

    if distributed:
        return _main_distributed(a, argv, t0, out, load_yaks(), opts, fopts)

    # Three stages, each on its own threads, a contig moving through them in input order:
    #   front end  (a.thread capped at 2 threads, each with a table-less context and its own BAM handle): BGZF inflate +
    #              record walk (host pool or device), admission, H2D, GPU columnariser -> the contig's pileup resident in HBM;
    #   polish     (up to 2 workers, each with a batch driver over contexts sharing ONE copy of the k-mer tables): a worker
    #              takes the next contig in input order AND every following one whose pileup is already resident (up to 16
    #              contigs / 64 Mb) and polishes them as ONE batch — one launch per pipeline step for all of them
    #              (np2_batch_polish): the contigs of a many-contig assembly cost a few ms together instead of 2 - 3 ms each;
    #              a long contig goes alone;
    #   output     (this thread): records written in input order.
    # The k-mer dumps are loaded and their HBM tables built next to the first front ends — a resident pileup does not
    # depend on them —, so a run starts reading alignments at once instead of after the tables (main.rs:1698-1853: the
    # reference's reader / workers / writer threads around two bounded channels).
    # (two of each: a front end already spreads its inflate over the host pool, and two polish workers keep the GPU busy
    # through each other's host phases)
    # (NP2_CLI_FRONT / NP2_CLI_WORKERS: experiments with other splits; -t beyond 2 keeps 2 + 2, see above)
    n_workers = int(os.environ.get("NP2_CLI_WORKERS", max(1, min(2, a.thread))))
    n_front = int(os.environ.get("NP2_CLI_FRONT", max(1, min(2, a.thread))))
    BATCH_SLOTS, BATCH_BP = int(os.environ.get("NP2_CLI_BATCH", "16")), 64_000_000
    tls = threading.local()
    base, base_lock = [], threading.Lock()
    yak_pool = ThreadPoolExecutor(max_workers=1)
    base_future = []

    def build_base():
        # dumps -> HBM tables in one go (np2_ctx_create_from_files: each file streamed to the device as it is read, one
        # host thread per dump); the device is not touched before a contig needs polishing
        t_b = time.time()
        if prof:
            print(f"[np2 profile] k-mer dumps: start at +{t_b - t0:.3f} s", file=sys.stderr)
        if a.sr:  # reads -> HBM tables that never visit the host (np2_ctx_create_from_reads)
            pol = np2io.polisher_from_reads(a.sr, a.sr_ks, min_count=a.sr_min_count, device=a.device, qc=a.sr_qc, ad=a.sr_adapter)
            _report_sr_qc(a)
        else:
            pol = np2io.polisher_from_yak_files(a.yak, device=a.device)
        if prof:
            print(f"[np2 profile] k-mer dumps read + tables in HBM {time.time() - t_b:.3f} s (at +{time.time() - t0:.3f} s)", file=sys.stderr)
        return pol

    sam_pool, sam_future, sam_lock = ThreadPoolExecutor(max_workers=1), [], threading.Lock()

    def open_sam():
        """the SAM text parsed and sorted on the device, resident for every front-end thread (np2_sam_open), on a table-less
        context of its own"""
        t_s = time.time()
        spol = Polisher([], device=a.device)
        try:
            if a.from_reads:  # reads -> index -> mapped, aligned, packed and sorted where they lie; the index goes once that is done
                mo = dict(a.map_opts)
                k = mo.pop("k", np2io.MAP_DEFAULTS["k"])
                weights = None
                if a.map_weights == "auto":
                    weights = np2io.MapWeights.from_assembly(a.fa, k=k, device=a.device)
                elif a.map_weights is not None:
                    weights = np2io.MapWeights(a.map_weights)
                with np2io.MapIndex(a.fa, k=k, w=mo.pop("w", np2io.MAP_DEFAULTS["w"]), device=a.device, weights=weights) as ix:
                    if weights is not None:
                        weights.close()
                    sam = np2io.Sam.from_reads(spol, ix, [a.bam] + a.more_reads, tie=a.sam_tie, keep_names=a.sorted_bam is not None, **mo)
            else:
                sam = np2io.Sam(spol, [a.bam], tie=a.sam_tie, keep_names=a.sorted_bam is not None, keep_all=a.sorted_bam_full)
            if a.sorted_bam is not None:  # the mapping is kept from this one pass over a stream that cannot be read twice
                st = sam.write_bam(spol, a.sorted_bam)
                if prof:
                    print(f"[np2 profile] sorted BAM written {time.time() - t_s:.3f} s after the start of the SAM: {st}", file=sys.stderr)
        except BaseException:
            spol.close()
            raise
        if prof:
            print(f"[np2 profile] SAM parsed and sorted {time.time() - t_s:.3f} s: {sam.stats()} (at +{time.time() - t0:.3f} s)", file=sys.stderr)
        return spol, sam

    def front_sam(name, seq):
        """the contig's pileup from the resident SAM (np2_contig_from_sam), on this thread's table-less context"""
        with sam_lock:
            if not sam_future:
                sam_future.append(sam_pool.submit(open_sam))
        sam = sam_future[0].result()[1]
        if getattr(tls, "fpol", None) is None:
            tls.fpol = Polisher([], device=a.device)
        t_f = time.time()
        c = np2io.contig_from_sam(tls.fpol, sam, name, seq, fopts)
        if prof:
            print(f"[np2 profile] {name}: front end {1e3 * (time.time() - t_f):.1f} ms (done at +{time.time() - t0:.3f} s)", file=sys.stderr)
        return c

    def front(name, seq):
        """the contig's pileup, resident in HBM (np2_contig_from_bam) — on this thread's table-less context"""
        if a.sam:
            return front_sam(name, seq)
        if getattr(tls, "fpol", None) is None:
            t_c = time.time()
            tls.fpol = Polisher([], device=a.device)
            t_b = time.time()
            tls.bam = np2io.Bam(a.bam)
            if prof:
                print(f"[np2 profile] front-end thread: context {1e3 * (t_b - t_c):.1f} ms, BAM + index opened {1e3 * (time.time() - t_b):.1f} ms "
                      f"(at +{time.time() - t0:.3f} s)", file=sys.stderr)
        t_f = time.time()
        c = np2io.contig_from_bam(tls.fpol, tls.bam, name, seq, fopts)
        if prof:
            print(f"[np2 profile] {name}: front end {1e3 * (time.time() - t_f):.1f} ms (done at +{time.time() - t0:.3f} s)", file=sys.stderr)
        return c

    def record(name, bases, pos):
        b = bases.tobytes()
        if a.uppercase:
            b = b.upper()
        if a.out_pos:
            return b"".join(b"%s\t%c\t%d\n" % (name.encode(), b[i:i + 1], int(pos[i])) for i in range(len(b)))
        if a.want_edits:  # (every position was fetched for the report: the span is its ends)
            return b">%s start:%d end:%d\n%s\n" % (name.encode(), pos[0], pos[-1], b), bases, pos
        return b">%s start:%d end:%d\n%s\n" % (name.encode(), pos[0], pos[1], b)

    from collections import deque
    from concurrent.futures import Future
    from .api import BatchPolisher
    todo, todo_cv = deque(), threading.Condition()  # (name, length, front-end future, result future) in input order
    closing = []

    def ensure_batch():
        if getattr(tls, "batch", None) is None:
            b0 = base_future[0].result()
            with base_lock:  # one copy of the k-mer tables in HBM: the other worker's contexts share it
                tls.pol = b0 if not base else b0.clone()
                base.append(tls.pol)
            t_b = time.time()
            tls.batch = BatchPolisher(tls.pol, BATCH_SLOTS)
            if prof:
                print(f"[np2 profile] polish worker: batch driver with {BATCH_SLOTS} slot contexts {1e3 * (time.time() - t_b):.1f} ms "
                      f"(at +{time.time() - t0:.3f} s)", file=sys.stderr)

    def polish_worker():
        """takes the head of `todo` and every following contig that is already resident; one batch per turn"""
        while True:
            with todo_cv:
                while not todo and not closing:
                    todo_cv.wait()
                if not todo:
                    return
                items = [todo.popleft()]
            try:
                # this worker's batch driver first (it waits for the k-mer tables, not for a pileup: made while the first front
                # ends are still reading — 7-9 ms that used to sit between the first resident contig and its polish)
                ensure_batch()
            except BaseException:
                pass  # (reported below, by the polish that needs it)
            try:
                items[0][2].exception()  # (waits for the head's front end)
            except BaseException:
                pass
            with todo_cv:
                bp = items[0][1]
                while todo and len(items) < BATCH_SLOTS and todo[0][2].done() and bp + todo[0][1] <= BATCH_BP:
                    items.append(todo.popleft())
                    bp += items[-1][1]
            live, contigs = [], []
            for it in items:  # a contig whose front end failed reports that, in its place of the output order
                e = it[2].exception()
                if e is not None:
                    it[3].set_exception(e)
                else:
                    live.append(it)
                    contigs.append(it[2].result())
            try:
                if not live:
                    continue
                ensure_batch()
                t_p = time.time()
                try:
                    res = tls.batch.polish(contigs, opts, want_pos=a.out_pos or a.want_edits)
                except Exception:
                    if len(contigs) == 1:
                        raise
                    # one contig of the batch failed: each on its own, so that the records before the failing one (in input
                    # order) are still written, as when every contig was polished by itself
                    res = []
                    for it, c in zip(live, contigs):
                        try:
                            res.append(tls.batch.polish([c], opts, want_pos=a.out_pos or a.want_edits)[0])
                        except Exception as e1:
                            it[3].set_exception(e1)
                            res.append(None)
                if prof:
                    print(f"[np2 profile] {', '.join(it[0] for it in live)}: polished as one batch in {1e3 * (time.time() - t_p):.1f} ms "
                          f"(done at +{time.time() - t0:.3f} s)", file=sys.stderr)
                for it, r in zip(live, res):
                    if r is not None:
                        it[3].set_result(record(it[0], r[0], r[1]))
            except BaseException as e:  # (the writer re-raises it in input order)
                for it in live:
                    if not it[3].done():
                        it[3].set_exception(e)
            finally:
                for c in contigs:
                    c.free()

    report, qpol = None, []
    if a.qv is not None:
        report = _qv_report(a, table_ks(a))
        base_future.append(yak_pool.submit(build_base))  # the tables are needed even when every contig passes through

    creport, cmp_in, cmp_out = None, [], []
    if a.cmp is not None:
        creport = _cmp_report(a, table_ks(a))
        if not base_future:
            base_future.append(yak_pool.submit(build_base))  # (as for --qv)

    ereport, epol = None, []
    if a.want_edits:  # (its context is made when the first polished contig is written: the tables are in HBM by then)
        ereport = _edits_report(a, table_ks(a))

    treport, tpol, trio_pool = None, [], None
    if a.trio is not None:  # the parental tables go into HBM next to the polish, in a context of their own
        treport, trio_pool = _trio_report(a), ThreadPoolExecutor(max_workers=1)
        trio_future = trio_pool.submit(_trio_polisher, a)

    workers = []
    try:
        with ThreadPoolExecutor(max_workers=n_front) as fpool:
            workers = [threading.Thread(target=polish_worker, name=f"np2-polish-{w}", daemon=True) for w in range(n_workers)]
            for w in workers:
                w.start()
            pending, pending_len = [], []  # records in input order: bytes or futures; the contigs' lengths
            pending_in = []  # --qv: (name, sequence as read) of the same contigs
            pending_trio = []  # --trio: the same
            pending_ed = []  # --edits: the same

            def drain(keep):
                while len(pending) > keep:
                    rec = pending.pop(0)
                    pending_len.pop(0)
                    rec = rec if isinstance(rec, bytes) else rec.result()
                    if ereport is not None:  # found on this thread's own context over the shared tables, from the fetched positions
                        e_name, e_seq = pending_ed.pop(0)
                        if isinstance(rec, tuple):
                            if not epol:
                                b0 = base_future[0].result()
                                with base_lock:
                                    epol.append(b0.clone())
                            ereport.add(epol[0], e_name, e_seq, rec[1], rec[2])
                            rec = rec[0]
                        else:
                            ereport.add_unpolished(e_name, len(e_seq))
                    out.write(rec)
                    if report is not None:  # measured as written, on this thread's own context over the shared tables
                        if not qpol:
                            b0 = base_future[0].result()
                            with base_lock:
                                qpol.append(b0.clone())
                        report.add(qpol[0], *pending_in.pop(0), _record_sequence(rec))
                    if treport is not None:
                        if not tpol:
                            tpol.append(trio_future.result())
                        treport.add(tpol[0], *pending_trio.pop(0), _record_sequence(rec))
                    if creport is not None:
                        cmp_out.append(_record_sequence(rec))

            try:
                for name, seq in np2io.read_fasta(a.fa):
                    if len(seq) >= 0xFFFFFFFF:
                        raise SystemExit(f"{name} is too long!")
                    if report is not None:
                        pending_in.append((name, seq))
                    if treport is not None:
                        pending_trio.append((name, seq))
                    if ereport is not None:
                        pending_ed.append((name, seq))
                    if creport is not None:
                        cmp_in.append(seq)
                    if len(seq) < a.min_ctg_len:  # pass-through (main.rs:1727-1730)
                        s = seq.upper() if a.uppercase else seq
                        if a.out_pos:
                            pending.append(b"".join(b"%s\t%c\t%d\n" % (name.encode(), s[i:i + 1], i) for i in range(len(s))))
                        else:
                            pending.append(b">%s start:0 end:%d\n%s\n" % (name.encode(), len(seq) - 1, s))
                        pending_len.append(len(seq))
                    else:
                        if not base_future:  # the first contig to polish: tables into HBM next to its front end
                            base_future.append(yak_pool.submit(build_base))
                        res = Future()
                        with todo_cv:
                            todo.append((name, len(seq), fpool.submit(front, name, seq), res))
                            todo_cv.notify()
                        pending.append(res)
                        pending_len.append(len(seq))
                    # bounded look-ahead: that many contigs held in memory at most — and at most ~2 Gb of contig in flight
                    # (a resident 30x pileup is ~16 bytes per base of HBM: three chromosomes, not six); short contigs may
                    # queue up to fill the workers' batches
                    keep = n_workers * BATCH_SLOTS + n_front
                    while keep > 1 and sum(pending_len[-keep:]) > 2_000_000_000:
                        keep -= 1
                    drain(keep)
                drain(0)
            finally:
                with todo_cv:
                    closing.append(True)
                    todo_cv.notify_all()
                for w in workers:
                    w.join()
            out.flush()
            if report is not None:
                report.write_cli(a.qv, a.qv_bed)
            if treport is not None:
                treport.write_cli(a.trio, a.trio_bed)
            if ereport is not None:
                ereport.write_cli(a.edits, a.edits_summary)
            if creport is not None:  # the whole assembly, on this thread's own context over the shared tables
                b0 = base_future[0].result()
                with base_lock:
                    cpol = b0.clone()
                try:
                    _cmp_finish(a, creport, cpol, cmp_in, cmp_out)
                finally:
                    cpol.close()
            if prof:
                print(f"[np2 profile] last record written at +{time.time() - t0:.3f} s", file=sys.stderr)
        if not base_future and not a.sr:
            load_yaks()  # (an assembly of pass-through contigs only: a broken dump must still be reported)
        if prof:
            print(f"[np2 profile] contexts released at +{time.time() - t0:.3f} s", file=sys.stderr)
    finally:
        for q in qpol + epol:  # (the QV and the edits context, on the error paths too)
            q.close()
        if trio_pool is not None:
            trio_pool.shutdown(wait=True)
            if not tpol and trio_future.exception() is None:
                tpol.append(trio_future.result())
            for q in tpol:
                q.close()
        yak_pool.shutdown(wait=False)
        if a.sorted_bam is not None and not sam_future and sys.exc_info()[0] is None:  # (an assembly without a contig)
            sam_future.append(sam_pool.submit(open_sam))
        sam_pool.shutdown(wait=True)
        if sam_future and sam_future[0].exception() is None:  # (after the front ends: nothing reads the resident SAM any more)
            spol, sam = sam_future[0].result()
            sam.close()
            spol.close()
        if out is not None and out is not sys.stdout.buffer:
            out.close()
    print(resource_str(t0, ["nextPolish2"] + argv, cpu0), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
