"""ctypes binding of include/np2_io.h: FASTA[.gz] / yak / indexed BAM readers and the GPU columnariser."""
import ctypes as C
import os

import numpy as np

from ._types import (READ_DTYPE, SRADAPT_READ_DTYPE, SRADAPT_STATS, SRQC_READ_DTYPE, SRQC_STATS, Pileup, Yak, np2_read_t,
                     np2_sradapt_opts_t, np2_sradapt_stats_t, np2_srqc_opts_t, np2_srqc_stats_t, np2_yak_t)
from .api import Np2Error, ResidentContig, lib

BAMREC_DTYPE = np.dtype([("pos", "<i4"), ("flag", "<u2"), ("mapq", "u1"), ("pad", "u1"), ("n_cigar", "<u4"),
                         ("pad2", "<u4"), ("cigar_off", "<u8"), ("l_seq", "<u4"), ("pad3", "<u4"), ("seq_off", "<u8")])
assert BAMREC_DTYPE.itemsize == 40

IO_SYMBOLS = ["np2_fasta_open", "np2_fasta_next", "np2_fasta_close", "np2_yak_load", "np2_yak_free", "np2_bam_open",
              "np2_bam_close", "np2_bam_n_refs", "np2_bam_ref_name", "np2_io_last_error", "np2_contig_from_records",
              "np2_contig_from_bam", "np2_contig_export", "np2_ctx_create_from_files", "np2_bgzf_inflate_device", "np2_crc32_device",
              "np2_kcount_files", "np2_kcount_bytes", "np2_kcount_files_to_dumps", "np2_ctx_create_from_reads", "np2_kcount_last_stats",
              "np2_seqfile_stream", "np2_bin_files", "np2_seqfile_reads", "np2_depth_from_records", "np2_depth_from_bam",
              "np2_srqc_bytes", "np2_srqc_files", "np2_srqc_last_stats", "np2_srqc_last_kernel_ms", "np2_kcount_files_qc",
              "np2_kcount_files_to_dumps_qc", "np2_ctx_create_from_reads_qc", "np2_seqfile_stream_qual", "np2_sam_open", "np2_sam_close",
              "np2_sam_n_refs", "np2_sam_ref_name", "np2_sam_stats", "np2_contig_from_sam", "np2_sam_parse_bytes", "np2_sam_export",
              "np2_sradapt_bytes", "np2_sradapt_files", "np2_sradapt_last_stats", "np2_sradapt_last_kernel_ms", "np2_kcount_files_ad",
              "np2_kcount_files_to_dumps_ad", "np2_ctx_create_from_reads_ad", "np2_bgzf_deflate_device", "np2_bgzf_deflate_host",
              "np2_bgzf_writer_open", "np2_bgzf_writer_write", "np2_bgzf_writer_close", "np2_sam_open_ex", "np2_sam_write_bam",
              "np2_sam_bam_stream", "np2_bamout_host", "np2_sam_export_names", "np2_sam_export_tails", "np2_sam_header_text",
              "np2_sam_tail_stats", "np2_bamout_host_full", "np2_sam_tails_host", "np2_sam_bamin_stats", "np2_bamin_host"]


class np2_front_opts_t(C.Structure):
    _fields_ = [("min_read_len", C.c_uint32), ("min_map_len", C.c_uint32), ("min_map_fra", C.c_float),
                ("min_map_qual", C.c_int16), ("max_clip_len", C.c_uint32), ("use_supplementary", C.c_uint8),
                ("use_secondary", C.c_uint8)]


class np2_kcount_opts_t(C.Structure):
    _fields_ = [("min_count", C.c_uint16), ("mem_bytes", C.c_uint64)]


class np2_bin_out_t(C.Structure):
    _fields_ = [("tsv", C.c_char_p), ("pat_list", C.c_char_p), ("mat_list", C.c_char_p), ("pat_fa", C.c_char_p), ("mat_fa", C.c_char_p)]


class np2_sam_opts_t(C.Structure):
    _fields_ = [("tie_by_strand", C.c_uint32)]


class np2_sam_stats_t(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("lines", "records", "unmapped", "kept", "cigar_words", "seq_bytes")] + \
               [(n, C.c_float) for n in ("parse_ms", "pack_ms", "sort_ms", "read_ms")]


class np2_bamout_stats_t(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("records", "stream_bytes", "file_bytes", "blocks", "bins", "chunks")] + \
               [(n, C.c_float) for n in ("sizes_ms", "emit_ms", "deflate_ms", "index_ms")]


class np2_bamin_stats_t(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("files", "blocks", "comp_bytes", "inflated_bytes", "records")] + \
               [(n, C.c_float) for n in ("inflate_ms", "crc_ms", "walk_ms", "fields_ms", "pack_ms")]


NP2_SAM_KEEP_NAMES = 1
NP2_SAM_KEEP_ALL = 2


class np2_map_opts_t(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("k", "w", "max_occ", "lookback", "max_gap", "bandwidth", "min_cnt", "min_score")]


class np2_map_stats_t(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("reads", "mapped", "unmapped", "minimizers", "anchors", "dropped_occ", "index_minimizers")] + \
               [("pieces", C.c_uint32), ("groups", C.c_uint32)] + [(f, C.c_float) for f in ("sketch_ms", "seed_ms", "sort_ms", "chain_ms", "read_ms", "write_ms")]


assert C.sizeof(np2_map_opts_t) == 32 and C.sizeof(np2_map_stats_t) == 88
MAP_DEFAULTS = dict(k=19, w=19, max_occ=200, lookback=64, max_gap=10000, bandwidth=500, min_cnt=3, min_score=40)
# np2_map_hit_t
MAP_HIT_DTYPE = np.dtype([("tid", "<i4")] + [(f, "<u4") for f in ("qlen", "qs", "qe", "rev", "ts", "te", "matches", "block", "mapq", "n", "s1", "s2")])
assert MAP_HIT_DTYPE.itemsize == 52


class np2_map_multi_opts_t(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("max_chains", "supplementary", "secondary_n", "mask_pm", "pri_pm")]


class np2_map_multi_stats_t(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("units", "selections", "dropped_min_cnt", "dropped_secondary", "kept_supplementary", "kept_secondary",
                                          "overflow_units")] + [("more_ms", C.c_float)]


assert C.sizeof(np2_map_multi_opts_t) == 20 and C.sizeof(np2_map_multi_stats_t) == 64
MULTI_DEFAULTS = dict(max_chains=1, supplementary=0, secondary_n=0, mask_pm=500, pri_pm=800)
MAP_CLS = ("primary", "supplementary", "secondary")  # a unit's cls


class np2_align_opts_t(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("match", "mismatch", "gap_open", "gap_ext", "band", "end_bonus", "ext_max", "max_cells")]


class np2_align_stats_t(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("pins", "segments", "equal", "pure_gap", "snv", "cores", "cells", "clipped_bases", "overflow")] + \
               [(f, C.c_float) for f in ("pins_ms", "classify_ms", "dp_ms", "assemble_ms", "write_ms")]


class np2_align_tag_stats_t(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("md_bytes", "cs_bytes", "eqx_words", "qual_reads")] + [("tags_ms", C.c_float)]


assert C.sizeof(np2_align_opts_t) == 32 and C.sizeof(np2_align_stats_t) == 96 and C.sizeof(np2_align_tag_stats_t) == 40
ALN_QUAL, ALN_MD, ALN_CS, ALN_EQX = 1, 2, 4, 8  # NP2_ALN_*
ALIGN_DEFAULTS = dict(match=1, mismatch=4, gap_open=6, gap_ext=2, band=32, end_bonus=5, ext_max=2048, max_cells=1 << 23)
# np2_align_rec_t
# np2_align_slot_t, np2_align_res_t and np2_align_probe_t (np2_align_chains_*)
ALIGN_SLOT_DTYPE = np.dtype([(f, "<u4") for f in ("t0", "q0", "tl", "ql", "pre", "suf", "kind", "W")] + [("lo", "<i4"), ("over", "<u4")])
ALIGN_RES_DTYPE = np.dtype([("score", "<i4"), ("ei", "<u4"), ("ej", "<u4")])
PROBE_SLOTS, PROBE_TB = 1, 2


class np2_align_probe_t(C.Structure):
    _fields_ = [("want", C.c_uint32), ("pad", C.c_uint32), ("n_slots", C.c_uint64), ("slot_off", C.c_void_p), ("slots", C.c_void_p),
                ("res", C.c_void_p), ("tb_off", C.c_void_p), ("tb", C.c_void_p)]


assert ALIGN_SLOT_DTYPE.itemsize == 40 and ALIGN_RES_DTYPE.itemsize == 12 and C.sizeof(np2_align_probe_t) == 56
ALIGN_REC_DTYPE = np.dtype([("tid", "<i4")] + [(f, "<u4") for f in ("flag", "pos", "end", "mapq", "n_cigar", "nm")] + [("as", "<i4")])
assert ALIGN_REC_DTYPE.itemsize == 32


class np2_map_units_t(C.Structure):
    _fields_ = [("n_units", C.c_uint64)] + [(f, C.c_void_p) for f in ("hits", "cls", "parent", "recs", "cigar", "cigar_off", "md", "md_off", "cs",
                                                                      "cs_off")]


class FrontOpts:
    """Read-admission options with the reference defaults (src/utils/option.rs:267-292; -a 500.5 splits into
    min_map_len = 500 and min_map_fra = 0.5, option.rs:232,258-259)."""

    def __init__(self, min_read_len=1000, min_map_len=500, min_map_fra=0.5, min_map_qual=1, max_clip_len=100,
                 use_supplementary=False, use_secondary=False):
        self.min_read_len, self.min_map_len, self.min_map_fra = min_read_len, min_map_len, min_map_fra
        self.min_map_qual, self.max_clip_len = min_map_qual, max_clip_len
        self.use_supplementary, self.use_secondary = use_supplementary, use_secondary

    def c(self):
        return np2_front_opts_t(self.min_read_len, self.min_map_len, self.min_map_fra, self.min_map_qual,
                                self.max_clip_len, 1 if self.use_supplementary else 0, 1 if self.use_secondary else 0)


class SrQc:
    """Options of the short-read quality filter that runs in front of the k-mer counter (include/np2_io.h has the rule: fixed
    trims, a sliding window from each end, N / unqualified-base / length filters).  The rule is this project's own, built on
    the options of the reference README's fastp recipe; it is not pinned against the fastp binary.  Reads are judged one by
    one (paired files are not kept in step); there is no adapter, poly-G / poly-X, complexity or average-quality filter.
    SrQc() and SrQc.recipe() are the recipe: -5 -3 -n 0 -f 5 -F 5 -t 5 -T 5 -q 20."""

    # key of the option text -> (attribute, lowest, highest)
    KEYS = {"front": ("trim_front", 0, 2 ** 32 - 1), "tail": ("trim_tail", 0, 2 ** 32 - 1), "cut5": ("cut_front", 0, 1),
            "cut3": ("cut_tail", 0, 1), "window": ("cut_window", 1, 1000), "mean": ("cut_mean_q", 0, 93),
            "n": ("n_base_limit", 0, 2 ** 32 - 1), "q": ("qualified_q", 0, 93), "u": ("unqualified_percent", 0, 100),
            "len": ("min_len", 0, 2 ** 32 - 1)}

    def __init__(self, trim_front=5, trim_tail=5, cut_front=True, cut_tail=True, cut_window=4, cut_mean_q=20, n_base_limit=0,
                 qualified_q=20, unqualified_percent=40, min_len=15):
        given = dict(trim_front=trim_front, trim_tail=trim_tail, cut_front=cut_front, cut_tail=cut_tail, cut_window=cut_window,
                     cut_mean_q=cut_mean_q, n_base_limit=n_base_limit, qualified_q=qualified_q,
                     unqualified_percent=unqualified_percent, min_len=min_len)
        for key, (attr, lo, hi) in self.KEYS.items():
            v = int(given[attr])
            if not lo <= v <= hi:
                raise ValueError(f"{attr} ({key}) must be in [{lo}, {hi}], not {given[attr]}")
            setattr(self, attr, bool(v) if attr in ("cut_front", "cut_tail") else v)

    @classmethod
    def recipe(cls):
        return cls()

    @classmethod
    def parse(cls, text):
        """The option text of the command lines: "" or None is the recipe, "key=value,..." overrides single keys of it
        (front tail cut5 cut3 window mean n q u len).  ValueError names what is wrong."""
        kw = {}
        for item in (text or "").split(","):
            if not item.strip():
                continue
            key, eq, val = item.partition("=")
            key = key.strip()
            if key not in cls.KEYS or not eq:
                raise ValueError(f"{item.strip()!r}: expected key=value with a key of {' '.join(cls.KEYS)}")
            if key in kw:
                raise ValueError(f"{key} is given twice")
            try:
                kw[key] = int(val.strip())
            except ValueError:
                raise ValueError(f"{key}={val.strip()}: not an integer") from None
        return cls(**{cls.KEYS[k][0]: v for k, v in kw.items()})

    def c(self):
        return np2_srqc_opts_t(self.trim_front, self.trim_tail, self.cut_window, self.cut_mean_q, self.n_base_limit, self.qualified_q,
                               self.unqualified_percent, self.min_len, (1 if self.cut_front else 0) | (2 if self.cut_tail else 0))

    def __repr__(self):
        return "SrQc(" + ", ".join(f"{k}={int(getattr(self, a))}" for k, (a, _, _) in self.KEYS.items()) + ")"


def sr_qc_arg(text):
    """argparse type of --sr_qc [SPEC], shared by the command lines: a bad key or value ends the parser (exit 2) before the
    library is loaded"""
    import argparse
    try:
        return SrQc.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


SR_QC_HELP = ("quality-trim and filter the reads on the GPU before their k-mers are counted (FASTQ input). Alone: the recipe "
              "front=5,tail=5,cut5=1,cut3=1,window=4,mean=20,n=0,q=20,u=40,len=15 (the options of fastp -5 -3 -n 0 -f 5 -F 5 -t 5 -T 5 "
              "-q 20; the rule is this project's own, reads are judged one by one, no adapter / poly-G / complexity filter). "
              "SPEC overrides single keys, e.g. front=0,tail=0,mean=25")


def srqc_stats_text(st):
    return ", ".join(f"{k} {st[k]}" for k in SRQC_STATS)


class SrAdapt:
    """Options of the short-read adapter trimmer that runs with the quality filter in front of the k-mer counter
    (include/np2_io.h has the rule).  pair: the files are R1 R2 R1 R2 .., the mates' overlap is searched (at least `overlap`
    bases with at most `diff` and at most `diffpct` percent of them different), a read-through adapter is cut off both
    mates, and a pair is dropped as soon as one mate fails.  seq / seq2: adapter sequences (4 - 64 letters of ACGT) cut
    off single reads and off the mates of pairs without an overlap; seq2 is mate 2's (default: seq).  The rule is this
    project's own, built on fastp's documented options; equality with the fastp binary is not claimed.  Out of scope:
    interleaved FASTQ, read-name checks, fastp's base correction inside the overlap, merging mates, poly-G / poly-X,
    adapter auto-detection for single-end input."""

    # key of the option text -> (attribute, lowest, highest)
    KEYS = {"pair": ("pair", 0, 1), "overlap": ("overlap", 1, 1024), "diff": ("diff", 0, 1024), "diffpct": ("diffpct", 0, 100)}
    SEQ_KEYS = ("seq", "seq2")

    def __init__(self, pair=False, overlap=30, diff=5, diffpct=20, seq=None, seq2=None):
        given = dict(pair=pair, overlap=overlap, diff=diff, diffpct=diffpct)
        for key, (attr, lo, hi) in self.KEYS.items():
            v = int(given[attr])
            if not lo <= v <= hi:
                raise ValueError(f"{key} must be in [{lo}, {hi}], not {given[attr]}")
            setattr(self, attr, bool(v) if attr == "pair" else v)
        for key, s in (("seq", seq), ("seq2", seq2)):
            if s is not None and (not isinstance(s, str) or not 4 <= len(s) <= 64 or set(s) - set("ACGT")):
                raise ValueError(f"{key}={s}: an adapter sequence is 4 to 64 letters of ACGT")
        if seq2 is not None and seq is None:
            raise ValueError("seq2 needs seq")
        if not self.pair and seq is None:
            raise ValueError("pair=0 trims by sequence: give seq=ADAPTER")
        self.seq, self.seq2 = seq, seq2

    @classmethod
    def parse(cls, text):
        """The option text of the command lines: "" or None is pair=1 with the defaults and no sequences, "key=value,..."
        sets single keys (pair overlap diff diffpct seq seq2).  ValueError names what is wrong."""
        kw = {"pair": 1}
        seen = set()
        for item in (text or "").split(","):
            if not item.strip():
                continue
            key, eq, val = item.partition("=")
            key, val = key.strip(), val.strip()
            if (key not in cls.KEYS and key not in cls.SEQ_KEYS) or not eq:
                raise ValueError(f"{item.strip()!r}: expected key=value with a key of {' '.join(list(cls.KEYS) + list(cls.SEQ_KEYS))}")
            if key in seen:
                raise ValueError(f"{key} is given twice")
            seen.add(key)
            if key in cls.SEQ_KEYS:
                kw[key] = val
            else:
                try:
                    kw[key] = int(val)
                except ValueError:
                    raise ValueError(f"{key}={val}: not an integer") from None
        return cls(**kw)

    def c(self):
        return np2_sradapt_opts_t(1 if self.pair else 0, self.overlap, self.diff, self.diffpct, None if self.seq is None else self.seq.encode(),
                                  None if self.seq2 is None else self.seq2.encode())

    def __repr__(self):
        return (f"SrAdapt(pair={int(self.pair)}, overlap={self.overlap}, diff={self.diff}, diffpct={self.diffpct}, seq={self.seq}, "
                f"seq2={self.seq2})")


def sr_adapter_arg(text):
    """argparse type of --sr_adapter [SPEC], as sr_qc_arg"""
    import argparse
    try:
        return SrAdapt.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def check_sr_adapter(parser, ad, files):
    """pair mode takes the read files two by two: an odd number is the parser's error, before the library loads"""
    if ad is not None and ad.pair and len(files) % 2:
        parser.error(f"--sr_adapter with pair=1 takes the read files as R1 R2 R1 R2 ..: {len(files)} file(s) given")


SR_ADAPTER_HELP = ("trim adapters off the reads on the GPU before their k-mers are counted (FASTQ input). Alone: pair=1,overlap=30,"
                   "diff=5,diffpct=20: the files are R1 R2 R1 R2 .., the mates' overlap is searched, a read-through adapter is cut "
                   "off both, and a pair is dropped when one mate fails. seq=ACGT..[,seq2=ACGT..] also trims by sequence; "
                   "pair=0,seq=AGATCGGAAGAGC trims single-end reads. The rule is this project's own, on fastp's documented options; "
                   "equality with the fastp binary is not claimed. Not done: interleaved FASTQ, read-name checks, base correction "
                   "in the overlap, merging, poly-G / poly-X, adapter auto-detection")


def sradapt_stats_text(st):
    return ", ".join(f"{k} {st[k]}" for k in SRADAPT_STATS)


_BOUND = False


_BIND_LOCK = __import__("threading").Lock()


def _bind():
    """The library with the argument types of include/np2_io.h declared.  Under a lock: the command line's stages call in
    from several threads at start-up, and a function called while another thread is still declaring its argtypes gets
    its pointers truncated to C ints."""
    global _BOUND
    L = lib()
    if _BOUND:
        return L
    with _BIND_LOCK:
        if _BOUND:
            return L
        _bind_locked(L)
        _BOUND = True
    return L


def _bind_locked(L):
    if True:
        vp = C.c_void_p
        L.np2_fasta_open.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.np2_fasta_next.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.np2_fasta_close.argtypes = [vp]
        L.np2_yak_load.argtypes = [C.c_char_p, C.POINTER(np2_yak_t)]
        L.np2_yak_free.argtypes = [C.POINTER(np2_yak_t)]
        L.np2_ctx_create_from_files.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_char_p), C.c_int]
        L.np2_bam_open.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.np2_bam_close.argtypes = [vp]
        L.np2_bam_n_refs.argtypes = [vp]
        L.np2_bam_ref_name.restype = C.c_char_p
        L.np2_bam_ref_name.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32)]
        L.np2_io_last_error.restype = C.c_char_p
        L.np2_contig_from_records.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.POINTER(np2_front_opts_t),
                                              C.POINTER(vp)]
        L.np2_contig_from_bam.argtypes = [vp, vp, C.c_char_p, vp, C.c_uint32, C.POINTER(np2_front_opts_t), C.POINTER(vp)]
        L.np2_contig_export.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.np2_bgzf_inflate_device.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        L.np2_crc32_device.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.POINTER(C.c_float)]
        L.np2_bgzf_deflate_device.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        L.np2_bgzf_deflate_host.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.np2_bgzf_writer_open.argtypes = [C.c_int, C.c_char_p, C.POINTER(vp)]
        L.np2_bgzf_writer_write.argtypes = [vp, vp, C.c_uint64]
        L.np2_bgzf_writer_close.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        _bind_shard(L)
        _bind_kcount(L)
        _bind_sam(L)
        _bind_map(L)


def _bind_map(L):
    vp, u64, mo = C.c_void_p, C.c_uint64, C.POINTER(np2_map_opts_t)
    L.np2_map_index_bytes.argtypes = [C.c_int, vp, u64, C.c_char_p, mo, C.POINTER(vp)]
    L.np2_map_index_files.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, mo, C.POINTER(vp)]
    L.np2_map_index_free.argtypes = [vp]
    L.np2_map_index_free.restype = None
    L.np2_map_index_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float)]
    L.np2_map_index_seq.argtypes = [vp, u64, C.POINTER(C.c_char_p), C.POINTER(u64)]
    L.np2_map_bytes.argtypes = [vp, vp, u64, u64, mo, vp, C.POINTER(vp), vp]
    L.np2_map_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, mo, C.c_char_p, C.POINTER(np2_map_stats_t)]
    L.np2_map_host.argtypes = [vp, u64, vp, u64, u64, mo, vp, C.POINTER(vp), vp]
    L.np2_map_last_stats.argtypes = [C.POINTER(np2_map_stats_t)]
    mm, pvp = C.POINTER(np2_map_multi_opts_t), C.POINTER(vp)
    L.np2_map_bytes_m.argtypes = [vp, vp, u64, u64, mo, mm, vp, pvp, pvp, pvp, pvp, pvp]
    L.np2_map_files_m.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, mo, mm, C.c_char_p, C.POINTER(np2_map_stats_t)]
    L.np2_map_host_m.argtypes = [vp, u64, vp, u64, u64, mo, mm, vp, vp, pvp, pvp, pvp, pvp, pvp]
    L.np2_map_last_multi_stats.argtypes = [C.POINTER(np2_map_multi_stats_t)]
    L.np2_map_weights_from_indices.argtypes = [C.c_uint32, vp, u64, C.POINTER(vp)]
    L.np2_map_weights_from_file.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.np2_map_weights_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(u64)]
    L.np2_map_weights_free.argtypes = [vp]
    L.np2_map_weights_free.restype = None
    L.np2_map_index_bytes_w.argtypes = [C.c_int, vp, u64, C.c_char_p, mo, vp, C.POINTER(vp)]
    L.np2_map_index_files_w.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, mo, vp, C.POINTER(vp)]
    L.np2_map_index_weights.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(u64)]
    L.np2_map_host_w.argtypes = [vp, u64, vp, u64, u64, mo, vp, vp, C.POINTER(vp), vp]
    ao = C.POINTER(np2_align_opts_t)
    L.np2_map_align_bytes.argtypes = [vp, vp, u64, u64, mo, ao, vp, vp, C.POINTER(vp), vp]
    L.np2_map_align_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, mo, ao, C.c_char_p, C.POINTER(np2_map_stats_t)]
    L.np2_map_align_host.argtypes = [vp, u64, vp, u64, u64, mo, ao, vp, vp, C.POINTER(vp), vp]
    L.np2_map_align_last_stats.argtypes = [C.POINTER(np2_align_stats_t)]
    L.np2_map_align_host_w.argtypes = [vp, u64, vp, u64, u64, mo, ao, vp, vp, vp, C.POINTER(vp), vp]
    u32 = C.c_uint32
    L.np2_map_align_bytes_x.argtypes = [vp, vp, vp, u64, u64, mo, ao, u32, vp, vp, C.POINTER(vp), vp, C.POINTER(vp), vp, C.POINTER(vp), vp]
    L.np2_map_align_files_x.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, mo, ao, u32, C.c_char_p, C.POINTER(np2_map_stats_t)]
    mm_, pu = C.POINTER(np2_map_multi_opts_t), C.POINTER(np2_map_units_t)
    L.np2_map_align_bytes_m.argtypes = [vp, vp, vp, u64, u64, mo, mm_, ao, u32, vp, pu]
    L.np2_map_align_files_m.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, mo, mm_, ao, u32, C.c_char_p, C.POINTER(np2_map_stats_t)]
    L.np2_map_align_host_m.argtypes = [vp, u64, vp, u64, u64, mo, mm_, ao, vp, u32, vp, pu]
    L.np2_map_align_host_x.argtypes = [vp, u64, vp, u64, u64, mo, ao, vp, u32, vp, vp, C.POINTER(vp), vp, C.POINTER(vp), vp, C.POINTER(vp), vp]
    L.np2_align_tags_device.argtypes = [C.c_int, vp, u64, vp, u64, u64, vp, vp, vp, vp, u32] + [C.POINTER(vp), vp] * 3
    L.np2_align_tags_host.argtypes = [vp, u64, vp, u64, u64, vp, vp, vp, vp, u32] + [C.POINTER(vp), vp] * 3
    L.np2_map_align_last_tag_stats.argtypes = [C.POINTER(np2_align_tag_stats_t)]
    pp = C.POINTER(np2_align_probe_t)
    L.np2_align_chains_device.argtypes = [vp, vp, u64, u64, u32, vp, vp, vp, ao, vp, C.POINTER(vp), vp, pp]
    L.np2_align_chains_host.argtypes = [vp, u64, vp, u64, u64, u32, vp, vp, vp, ao, vp, C.POINTER(vp), vp, pp]
    so, pvp = C.POINTER(np2_sam_opts_t), C.POINTER(vp)
    L.np2_sam_from_reads.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_int, mo, ao, so, C.c_uint32, pvp]
    L.np2_sam_from_read_bytes.argtypes = [vp, vp, vp, u64, u64, C.c_char_p, mo, ao, so, C.c_uint32, pvp]
    L.np2_align_pack_host.argtypes = [vp, vp, vp, vp, u64, u64, so, pvp, pvp, pvp, pvp, C.POINTER(u64)]


def _bind_shard(L):
    from ._types import np2_shard_plan_t
    vp = C.c_void_p
    L.np2_shard_bam_begin.argtypes = [vp, vp, C.c_char_p, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.np2_shard_bam_finish.argtypes = [vp, vp, C.c_uint64, C.POINTER(np2_shard_plan_t), C.POINTER(vp), C.POINTER(C.c_uint32)]
    L.np2_shard_bam_abort.argtypes = [vp]
    L.np2_shard_bam_abort.restype = None


def _bind_sam(L):
    vp, so, ss = C.c_void_p, C.POINTER(np2_sam_opts_t), C.POINTER(np2_sam_stats_t)
    L.np2_sam_open.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, so, C.POINTER(vp)]
    L.np2_sam_close.argtypes = [vp]
    L.np2_sam_close.restype = None
    L.np2_sam_n_refs.argtypes = [vp]
    L.np2_sam_ref_name.restype = C.c_char_p
    L.np2_sam_ref_name.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32)]
    L.np2_sam_stats.argtypes = [vp, ss]
    L.np2_contig_from_sam.argtypes = [vp, vp, C.c_char_p, vp, C.c_uint32, C.POINTER(np2_front_opts_t), C.POINTER(vp)]
    L.np2_sam_parse_bytes.argtypes = [C.c_int, vp, C.c_uint64, so, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                      C.POINTER(C.c_uint64), ss]
    L.np2_sam_export.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    u64p, bs = C.POINTER(C.c_uint64), C.POINTER(np2_bamout_stats_t)
    L.np2_sam_open_ex.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, so, C.c_uint32, C.POINTER(vp)]
    L.np2_sam_write_bam.argtypes = [vp, vp, C.c_char_p, C.c_char_p, bs]
    L.np2_sam_bam_stream.argtypes = [vp, vp, C.POINTER(vp), u64p]
    L.np2_sam_export_names.argtypes = [vp, vp, C.POINTER(vp), u64p, C.POINTER(vp), u64p]
    L.np2_bamout_host.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, C.POINTER(C.c_char_p), vp,
                                  C.c_int, C.c_char_p, C.c_char_p, C.POINTER(vp), u64p, bs]
    L.np2_sam_export_tails.argtypes = [vp, vp, C.POINTER(vp), u64p, C.POINTER(vp), u64p]
    L.np2_sam_header_text.argtypes = [vp, C.POINTER(vp), u64p]
    L.np2_sam_tail_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p]
    L.np2_bamout_host_full.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.c_uint64,
                                       C.POINTER(C.c_char_p), vp, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(vp), u64p, bs]
    L.np2_sam_tails_host.argtypes = [vp, C.c_uint64, C.POINTER(vp), u64p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), u64p, C.POINTER(vp), u64p]
    L.np2_sam_bamin_stats.argtypes = [vp, C.POINTER(np2_bamin_stats_t)]
    pvp = C.POINTER(vp)
    L.np2_bamin_host.argtypes = [vp, C.c_uint64, C.c_uint32, so, pvp, pvp, u64p, pvp, pvp, pvp, u64p, pvp, u64p, pvp, u64p, pvp, pvp, u64p, pvp, u64p]


def _bind_kcount(L):
    vp, ko, cpp = C.c_void_p, C.POINTER(np2_kcount_opts_t), C.POINTER(C.c_char_p)
    L.np2_kcount_files.argtypes = [C.c_int, cpp, C.c_int, vp, C.c_int, ko, C.POINTER(np2_yak_t)]
    L.np2_kcount_bytes.argtypes = [C.c_int, vp, C.c_uint64, vp, C.c_int, ko, C.POINTER(np2_yak_t)]
    L.np2_kcount_files_to_dumps.argtypes = [C.c_int, cpp, C.c_int, vp, C.c_int, ko, cpp]
    L.np2_ctx_create_from_reads.argtypes = [C.POINTER(vp), C.c_int, cpp, C.c_int, vp, C.c_int, ko]
    L.np2_kcount_last_stats.argtypes = [C.POINTER(C.c_uint64)] * 3 + [C.POINTER(C.c_uint32)] * 2 + [C.POINTER(C.c_float)] * 2
    L.np2_seqfile_stream.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_uint64)]
    from .api import np2_bin_opts_t
    L.np2_bin_files.argtypes = [vp, C.c_int, C.c_int, cpp, C.c_int, C.POINTER(np2_bin_opts_t), C.POINTER(np2_bin_out_t), vp, C.POINTER(C.c_float)]
    L.np2_seqfile_reads.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(C.c_uint64)]
    qo, qs = C.POINTER(np2_srqc_opts_t), C.POINTER(np2_srqc_stats_t)
    L.np2_kcount_files_qc.argtypes = [C.c_int, cpp, C.c_int, vp, C.c_int, ko, qo, C.POINTER(np2_yak_t)]
    L.np2_kcount_files_to_dumps_qc.argtypes = [C.c_int, cpp, C.c_int, vp, C.c_int, ko, qo, cpp]
    L.np2_ctx_create_from_reads_qc.argtypes = [C.POINTER(vp), C.c_int, cpp, C.c_int, vp, C.c_int, ko, qo]
    L.np2_srqc_bytes.argtypes = [C.c_int, vp, vp, C.c_uint64, qo, vp, vp, C.c_uint64, qs]
    L.np2_srqc_files.argtypes = [C.c_int, cpp, C.c_int, qo, cpp, qs]
    L.np2_srqc_last_stats.argtypes = [qs]
    L.np2_srqc_last_kernel_ms.argtypes = [C.POINTER(C.c_float)]
    L.np2_seqfile_stream_qual.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    ao, as_ = C.POINTER(np2_sradapt_opts_t), C.POINTER(np2_sradapt_stats_t)
    L.np2_kcount_files_ad.argtypes = [C.c_int, cpp, C.c_int, vp, C.c_int, ko, qo, ao, C.POINTER(np2_yak_t)]
    L.np2_kcount_files_to_dumps_ad.argtypes = [C.c_int, cpp, C.c_int, vp, C.c_int, ko, qo, ao, cpp]
    L.np2_ctx_create_from_reads_ad.argtypes = [C.POINTER(vp), C.c_int, cpp, C.c_int, vp, C.c_int, ko, qo, ao]
    L.np2_sradapt_bytes.argtypes = [C.c_int, vp, vp, C.c_uint64, qo, ao, vp, vp, C.c_uint64, as_]
    L.np2_sradapt_files.argtypes = [C.c_int, cpp, C.c_int, qo, ao, cpp, as_]
    L.np2_sradapt_last_stats.argtypes = [as_]
    L.np2_sradapt_last_kernel_ms.argtypes = [C.POINTER(C.c_float)]


def _io_check(rc):
    if rc != 0:
        raise Np2Error(rc, _bind().np2_io_last_error().decode())


def read_fasta(path):
    """Yield (name, sequence bytes) like kseq (src/main.rs:1705-1714): name = header up to the first whitespace."""
    L = _bind()
    h = C.c_void_p()
    _io_check(L.np2_fasta_open(path.encode(), C.byref(h)))
    try:
        name, seq, n = C.c_char_p(), C.c_void_p(), C.c_uint64()
        while True:
            rc = L.np2_fasta_next(h, C.byref(name), C.byref(seq), C.byref(n))
            if rc == 0:
                break
            if rc < 0:
                _io_check(rc)
            yield name.value.decode(), C.string_at(seq.value, n.value) if n.value else b""
    finally:
        L.np2_fasta_close(h)


def load_yak(path):
    """yak v2 dump -> Yak (src/utils/kmer.rs:72-170)."""
    import weakref
    L = _bind()
    y = np2_yak_t()
    _io_check(L.np2_yak_load(path.encode(), C.byref(y)))
    nb = (1 << y.pre) + 1
    off = np.ctypeslib.as_array(y.bucket_off, shape=(nb,)).copy()
    # the words are used where the loader put them (no second copy of a dump of tens of GB): np2_yak_free runs when the
    # array is collected
    base = np.ctypeslib.as_array(y.words, shape=(max(int(y.n_words), 1),))
    yk = Yak(y.k, base[: int(y.n_words)], off, pre=y.pre)
    # (tied to the Yak object, not to `base`: a view's .base is the memory's owner, not the intermediate array, so `base`
    # itself may be collected while its views live on)
    weakref.finalize(yk, L.np2_yak_free, y)
    return yk


def check_yak_header(path):
    """The cheap part of a dump's validation (kmer.rs:73-90: magic, counter bits; what this implementation supports:
    k < 32, pre == 10) without reading its words: the command line runs it on every dump BEFORE it opens its output, like
    the reference, which loads its yak files before the first contig.  Returns k; raises ValueError with the message."""
    import struct
    with open(path, "rb") as f:
        hd = f.read(16)
    if len(hd) != 16 or hd[:4] != b"YAK\x02":
        raise ValueError("The input binary k-mer dump file is incompatible.")
    k, pre, cbits = struct.unpack("<III", hd[4:])
    if cbits != 10:
        raise ValueError("different YAK_COUNTER_BITS")
    if k >= 32 or k < 2 or pre != 10:
        raise ValueError(f"{path}: k = {k}, prefix bits = {pre}: only k < 32 with the default 10 prefix bits is supported")
    return k


def polisher_from_yak_files(paths, device=0):
    """np2_ctx_create_from_files: a Polisher whose HBM k-mer tables are built from the dumps as they are read (no host
    copy of the words; tables ordered by k, option.rs:238)."""
    from .api import Polisher
    L = _bind()
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    h = C.c_void_p()
    _io_check(L.np2_ctx_create_from_files(C.byref(h), device, arr, len(paths)))
    p = Polisher.__new__(Polisher)
    p._yaks = []
    p._h = h
    p.device = device
    return p


def _paths(paths):
    paths = [paths] if isinstance(paths, (str, os.PathLike)) else list(paths)
    return (C.c_char_p * len(paths))(*[os.fspath(p).encode() for p in paths]), len(paths)


def _ks(ks):
    return np.ascontiguousarray(list(ks), dtype=np.uint32)


def seqfile_stream(path):
    """np2_seqfile_stream (host only): the separator stream the counter's reader makes of one FASTA / FASTQ /
    one-sequence-per-line file, plain or gzip: every read's bytes followed by one newline."""
    L = _bind()
    p, n = C.c_void_p(), C.c_uint64()
    _io_check(L.np2_seqfile_stream(os.fspath(path).encode(), C.byref(p), C.byref(n)))
    try:
        return C.string_at(p.value, n.value) if n.value else b""
    finally:
        L.np2_free(p)


def seqfile_reads(path):
    """np2_seqfile_reads (host only): (names, ends) of one sequence file as the read binner's reader sees it: the reads'
    names (header up to the first whitespace, without '>' / '@') and, per read, the offset of its separator in the
    file's separator stream (seqfile_stream)."""
    L = _bind()
    names, nb, ends, n = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    _io_check(L.np2_seqfile_reads(os.fspath(path).encode(), C.byref(names), C.byref(nb), C.byref(ends), C.byref(n)))
    try:
        text = C.string_at(names.value, nb.value) if nb.value else b""
        e = np.ctypeslib.as_array(C.cast(ends, C.POINTER(C.c_uint64)), shape=(max(1, n.value),))[:n.value].copy()
        return [x.decode() for x in text.split(b"\n")[:-1]], e
    finally:
        L.np2_free(names)
        L.np2_free(ends)


def bin_files(pol, paths, pat_idx=0, mat_idx=1, min_count=2, mid_count=5, min_score=2, minor_permille=330, tsv=None, pat_list=None,
              mat_list=None, pat_fa=None, mat_fa=None):
    """np2_bin_files: read files -> classes on the device of Polisher `pol`, written natively (every output path may be
    None) -> ({"p": n, "m": n, "a": n, "0": n}, kernel_ms)."""
    from .api import np2_bin_opts_t
    L = _bind()
    arr, n = _paths(paths)
    enc = lambda p: None if p is None else os.fspath(p).encode()
    out = np2_bin_out_t(enc(tsv), enc(pat_list), enc(mat_list), enc(pat_fa), enc(mat_fa))
    o = np2_bin_opts_t(min_count, mid_count, min_score, minor_permille)
    counts = np.zeros(4, np.uint64)
    ms = C.c_float()
    pol._check(L.np2_bin_files(pol._h, pat_idx, mat_idx, arr, n, C.byref(o), C.byref(out), counts.ctypes.data, C.byref(ms)))
    return dict(zip("pma0", (int(x) for x in counts))), ms.value


def _qc(qc):
    return None if qc is None else C.byref(qc.c())


def _ad(ad):
    return None if ad is None else C.byref(ad.c())


def count_kmers(inputs, ks, min_count=1, device=0, mem_bytes=0, qc=None, ad=None):
    """Canonical k-mers of short reads counted on the device -> one Yak per k (np2_kcount_files / np2_kcount_bytes).
    `inputs`: sequence file paths (FASTA / FASTQ / one sequence per line, plain or gzip), or ONE bytes object holding a
    separator stream (the reads' bytes with a newline, or any non-base byte, between reads).  Words with a count below
    `min_count` are left out (an exact threshold); counts saturate at 1023.  `qc` (an SrQc; files only, FASTQ): the reads
    are quality-trimmed and filtered on the device before they are counted; srqc_last_stats() has the totals.  `ad` (an
    SrAdapt; files only, FASTQ; with pair=True the files are R1 R2 R1 R2 ..): adapters are trimmed as well, and
    sradapt_last_stats() has the totals instead."""
    import weakref
    L = _bind()
    kk = _ks(ks)
    o = np2_kcount_opts_t(min_count, mem_bytes)
    out = (np2_yak_t * max(1, len(kk)))()
    if isinstance(inputs, (bytes, bytearray, memoryview)):
        if qc is not None or ad is not None:
            raise ValueError("qc and ad need FASTQ files: a separator stream has no qualities")
        buf = np.frombuffer(inputs, dtype=np.uint8)
        _io_check(L.np2_kcount_bytes(device, buf.ctypes.data if len(buf) else None, len(buf), kk.ctypes.data, len(kk), C.byref(o), out))
    else:
        arr, n = _paths(inputs)
        _io_check(L.np2_kcount_files_ad(device, arr, n, kk.ctypes.data, len(kk), C.byref(o), _qc(qc), _ad(ad), out))
    yaks = []
    for i in range(len(kk)):
        y = np2_yak_t.from_buffer_copy(out[i])
        off = np.ctypeslib.as_array(y.bucket_off, shape=((1 << y.pre) + 1,)).copy()
        base = np.ctypeslib.as_array(y.words, shape=(max(int(y.n_words), 1),))
        yk = Yak(y.k, base[: int(y.n_words)], off, pre=y.pre)
        weakref.finalize(yk, L.np2_yak_free, y)  # (as in load_yak: the words are used where the library put them)
        yaks.append(yk)
    return yaks


def count_kmers_to_files(paths, ks, out_paths, min_count=1, device=0, mem_bytes=0, qc=None, ad=None):
    """np2_kcount_files_to_dumps: sequence files -> one yak v2 dump per k, written bucket by bucket (qc, ad: as count_kmers)."""
    L = _bind()
    kk = _ks(ks)
    if len(out_paths) != len(kk):
        raise ValueError("one output path per k")
    arr, n = _paths(paths)
    outs, _ = _paths(out_paths)
    o = np2_kcount_opts_t(min_count, mem_bytes)
    _io_check(L.np2_kcount_files_to_dumps_ad(device, arr, n, kk.ctypes.data, len(kk), C.byref(o), _qc(qc), _ad(ad), outs))


def polisher_from_reads(paths, ks, min_count=1, device=0, mem_bytes=0, qc=None, ad=None):
    """np2_ctx_create_from_reads: a Polisher whose HBM k-mer tables are counted from the reads and never visit the host
    (tables ordered by k, option.rs:238).  Single-pass runs only.  qc, ad: as count_kmers."""
    from .api import Polisher
    L = _bind()
    kk = _ks(ks)
    arr, n = _paths(paths)
    o = np2_kcount_opts_t(min_count, mem_bytes)
    h = C.c_void_p()
    _io_check(L.np2_ctx_create_from_reads_ad(C.byref(h), device, arr, n, kk.ctypes.data, len(kk), C.byref(o), _qc(qc), _ad(ad)))
    p = Polisher.__new__(Polisher)
    p._yaks = []
    p._h = h
    p.device = device
    return p


def sr_k_arg(parser, text):
    """--sr_k's comma-separated k values, ascending (tables are ordered by k); anything else is the parser's error"""
    try:
        return sorted(int(k) for k in text.split(","))
    except ValueError:
        parser.error("--sr_k takes comma-separated integers")


def add_table_args(p):
    """where a report module's k-mer tables come from: yak dumps, or short reads counted on the device"""
    p.add_argument("yak", nargs="*", metavar="k.yak", help="k-mer dumps in yak format")
    p.add_argument("--sr", action="append", default=[], metavar="FILE", help="short reads (may repeat): count their k-mers on the GPU instead")
    p.add_argument("--sr_k", default="21,31", metavar="K[,K...]", help="k-mer sizes counted from --sr [21,31]")
    p.add_argument("--sr_min_count", type=int, default=2, metavar="N", help="drop k-mers of --sr counted fewer than N times [2]")


def open_tables(parser, a):
    """the arguments of add_table_args (and --device) -> (a Polisher with the tables in HBM, their k values in table order)"""
    if a.sr:
        ks = sr_k_arg(parser, a.sr_k)
        return polisher_from_reads(a.sr, ks, min_count=a.sr_min_count, device=a.device), ks
    try:
        ks = sorted(check_yak_header(y) for y in a.yak)
    except (ValueError, OSError) as e:
        raise SystemExit(f"Error: {e}")
    return polisher_from_yak_files([os.path.abspath(y) for y in a.yak], device=a.device), ks


def kcount_last_stats():
    """np2_kcount_last_stats: figures of the last successful counting call on this thread."""
    L = _bind()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    g, p = C.c_uint32(), C.c_uint32()
    km, rm = C.c_float(), C.c_float()
    L.np2_kcount_last_stats(C.byref(a), C.byref(b), C.byref(c), C.byref(g), C.byref(p), C.byref(km), C.byref(rm))
    return {"kmers": a.value, "distinct": b.value, "spilled": c.value, "growths": g.value, "passes": p.value,
            "kernel_ms": km.value, "read_ms": rm.value}


def _stats_dict(st):
    return dict(zip(SRQC_STATS, (int(getattr(st, f)) for f, _ in np2_srqc_stats_t._fields_)))


def srqc_last_stats():
    """np2_srqc_last_stats: the totals of the last quality-filtering call on this thread (of a multi-pass count: one pass's)
    plus kernel_ms, the filter kernel's time in that call."""
    L = _bind()
    st, ms = np2_srqc_stats_t(), C.c_float()
    L.np2_srqc_last_stats(C.byref(st))
    L.np2_srqc_last_kernel_ms(C.byref(ms))
    return dict(_stats_dict(st), kernel_ms=ms.value)


def srqc_bytes(seq, qual, qc=None, device=0, want_masked=True, want_reads=True):
    """np2_srqc_bytes: one pair of streams (the reads' bases / quality bytes, every read followed by a newline in both)
    through the filter -> (masked stream or None, per-read array of (begin, end, cls) or None, totals dict)."""
    L = _bind()
    s, q = np.frombuffer(seq, dtype=np.uint8), np.frombuffer(qual, dtype=np.uint8)
    if len(s) != len(q):
        raise ValueError("the two streams differ in length")
    n_reads = int((s == 10).sum())
    masked = np.empty(max(1, len(s)), np.uint8) if want_masked else None
    reads = np.zeros(max(1, n_reads), SRQC_READ_DTYPE) if want_reads else None
    st = np2_srqc_stats_t()
    o = (qc or SrQc()).c()
    _io_check(L.np2_srqc_bytes(device, s.ctypes.data if len(s) else None, q.ctypes.data if len(s) else None, len(s), C.byref(o),
                               masked.ctypes.data if want_masked else None, reads.ctypes.data if want_reads else None, n_reads, C.byref(st)))
    return (masked[:len(s)].tobytes() if want_masked else None), (reads[:n_reads] if want_reads else None), _stats_dict(st)


def srqc_files(paths, qc=None, out_paths=None, device=0):
    """np2_srqc_files: FASTQ files through the filter -> [totals dict per file] + [their sum]; out_paths (one per input,
    entries may be None): the cleaned plain-text FASTQ files."""
    L = _bind()
    arr, n = _paths(paths)
    outs = None
    if out_paths is not None:
        if len(out_paths) != n:
            raise ValueError("one output path per input")
        outs = (C.c_char_p * n)(*[None if p is None else os.fspath(p).encode() for p in out_paths])
    st = (np2_srqc_stats_t * (n + 1))()
    o = (qc or SrQc()).c()
    _io_check(L.np2_srqc_files(device, arr, n, C.byref(o), outs, st))
    return [_stats_dict(x) for x in st]


def _ad_stats_dict(st):
    return dict(zip(SRADAPT_STATS, (int(getattr(st, f)) for f, _ in np2_sradapt_stats_t._fields_)))


def sradapt_last_stats():
    """np2_sradapt_last_stats: the totals of the last adapter-trimming call on this thread plus kernel_ms"""
    L = _bind()
    st, ms = np2_sradapt_stats_t(), C.c_float()
    L.np2_sradapt_last_stats(C.byref(st))
    L.np2_sradapt_last_kernel_ms(C.byref(ms))
    return dict(_ad_stats_dict(st), kernel_ms=ms.value)


def sradapt_bytes(seq, qual, qc=None, ad=None, device=0, want_masked=True, want_reads=True):
    """np2_sradapt_bytes: srqc_bytes with the adapter rule (ad: an SrAdapt, None: pair mode with the defaults; qc None: every
    quality step off).  In pair mode reads 2r and 2r + 1 are mates.  -> (masked stream or None, per-read array of (begin,
    end, cls, how, insert) or None, totals dict)."""
    L = _bind()
    s, q = np.frombuffer(seq, dtype=np.uint8), np.frombuffer(qual, dtype=np.uint8)
    if len(s) != len(q):
        raise ValueError("the two streams differ in length")
    n_reads = int((s == 10).sum())
    masked = np.empty(max(1, len(s)), np.uint8) if want_masked else None
    reads = np.zeros(max(1, n_reads), SRADAPT_READ_DTYPE) if want_reads else None
    st = np2_sradapt_stats_t()
    _io_check(L.np2_sradapt_bytes(device, s.ctypes.data if len(s) else None, q.ctypes.data if len(s) else None, len(s), _qc(qc), _ad(ad),
                                  masked.ctypes.data if want_masked else None, reads.ctypes.data if want_reads else None, n_reads, C.byref(st)))
    return (masked[:len(s)].tobytes() if want_masked else None), (reads[:n_reads] if want_reads else None), _ad_stats_dict(st)


def sradapt_files(paths, qc=None, ad=None, out_paths=None, device=0):
    """np2_sradapt_files: FASTQ files through quality filter and adapter trimmer -> [totals dict per unit] + [their sum]; a
    unit is a file, or in pair mode (the files R1 R2 R1 R2 ..) a pair of files.  out_paths (one per input): the cleaned
    plain-text FASTQ files; of a pair only what passes in both mates is written."""
    L = _bind()
    arr, n = _paths(paths)
    outs = None
    if out_paths is not None:
        if len(out_paths) != n:
            raise ValueError("one output path per input")
        outs = (C.c_char_p * n)(*[None if p is None else os.fspath(p).encode() for p in out_paths])
    st = (np2_sradapt_stats_t * (n + 1))()
    _io_check(L.np2_sradapt_files(device, arr, n, _qc(qc), _ad(ad), outs, st))
    units = n // 2 if (ad is None or ad.pair) else n
    return [_ad_stats_dict(x) for x in st[:units + 1]]


def seqfile_stream_qual(path):
    """np2_seqfile_stream_qual (host only): (sequence stream, quality stream) the reader makes of one FASTQ file, plain or
    gzip: equal lengths, a newline after every read in both."""
    L = _bind()
    ps, pq, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    _io_check(L.np2_seqfile_stream_qual(os.fspath(path).encode(), C.byref(ps), C.byref(pq), C.byref(n)))
    try:
        return (C.string_at(ps.value, n.value), C.string_at(pq.value, n.value)) if n.value else (b"", b"")
    finally:
        L.np2_free(ps)
        L.np2_free(pq)


def write_yak(path, yak):
    """Write a Yak as a yak v2 dump ("YAK\\2", k, pre, counter_bits = 10, then per bucket: u32, u32 n, n x u64)."""
    import struct
    with open(path, "wb") as f:
        f.write(b"YAK\x02" + struct.pack("<III", yak.k, yak.pre, 10))
        for b in range(1 << yak.pre):
            s, e = int(yak.bucket_off[b]), int(yak.bucket_off[b + 1])
            f.write(struct.pack("<II", 0, e - s))
            f.write(yak.words[s:e].tobytes())


class Bam:
    def __init__(self, path):
        L = _bind()
        self._h = C.c_void_p()
        _io_check(L.np2_bam_open(path.encode(), C.byref(self._h)))

    def refs(self):
        L = _bind()
        out = []
        for i in range(L.np2_bam_n_refs(self._h)):
            n = C.c_uint32()
            out.append((L.np2_bam_ref_name(self._h, i, C.byref(n)).decode(), n.value))
        return out

    def close(self):
        if self._h:
            _bind().np2_bam_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SAM_TIES = ("strand", "input")


def _sam_opts(tie):
    if tie not in SAM_TIES:
        raise ValueError(f"tie must be one of {' '.join(SAM_TIES)}, not {tie!r}")
    return np2_sam_opts_t(1 if tie == "strand" else 0)


def _sam_stats_dict(st):
    return {n: (int if t is C.c_uint64 else float)(getattr(st, n)) for n, t in np2_sam_stats_t._fields_}


class Sam:
    """np2_sam_open: the mapper's SAM text (one or more files, plain or gzip; "-" is standard input) or BAM files (sorted or
    not, no index is read; each path is sniffed on its own, and both kinds may be mixed), parsed or unpacked and
    coordinate-sorted on the device of Polisher `pol`, the sorted records, their CIGAR words and the packed SEQ left resident
    there (include/np2_io.h has the rule).  tie: "strand" orders records at one position by strand, as samtools sort does;
    "input" leaves them in input order.  Read-only once open: contig_from_sam may be called from several threads, each with
    a Polisher of its own on that device.  keep_names=True (np2_sam_open_ex, NP2_SAM_KEEP_NAMES) keeps the QNAMEs resident too:
    write_bam needs them.  keep_all=True (NP2_SAM_KEEP_ALL, which implies the names) keeps QUAL, RNEXT, PNEXT, TLEN, the optional
    fields and the header lines as well: write_bam and bam_stream then write the full BAM (about three times the device memory)."""

    def __init__(self, pol, paths, tie="strand", keep_names=False, keep_all=False):
        L = _bind()
        o = _sam_opts(tie)
        arr, n = _paths(paths)
        self._h = C.c_void_p()
        if keep_all:
            _io_check(L.np2_sam_open_ex(pol._h, arr, n, C.byref(o), NP2_SAM_KEEP_ALL, C.byref(self._h)))
        elif keep_names:  # np2_sam_open_ex: the QNAMEs stay resident too, for write_bam
            _io_check(L.np2_sam_open_ex(pol._h, arr, n, C.byref(o), NP2_SAM_KEEP_NAMES, C.byref(self._h)))
        else:
            _io_check(L.np2_sam_open(pol._h, arr, n, C.byref(o), C.byref(self._h)))

    @classmethod
    def from_reads(cls, pol, index, paths_or_reads, tie="strand", keep_names=False, names=None, **map_and_align_kw):
        """np2_sam_from_reads / np2_sam_from_read_bytes: HiFi reads mapped and aligned against the MapIndex `index` (on pol's
        device), the records packed and coordinate-sorted where they lie: an ordinary Sam that holds what Sam(pol, [the SAM
        map_align_files writes for the same call]) would hold, without the text.  paths_or_reads: a list of read files (FASTA or
        FASTQ, plain or gzip), or a list of sequences (bytes) / a separator stream as MapIndex.align takes, then with `names` (one
        per read) or numbered from 1.  Options: MAP_DEFAULTS and ALIGN_DEFAULTS."""
        L = _bind()
        kw = dict(map_and_align_kw)
        akw = {f: kw.pop(f) for f in list(kw) if f in ALIGN_DEFAULTS}
        o, ao, so = index._opts(kw), align_opts(**akw), _sam_opts(tie)
        flags = NP2_SAM_KEEP_NAMES if keep_names else 0
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        in_memory = isinstance(paths_or_reads, (bytes, bytearray, memoryview, np.ndarray)) or (
            len(paths_or_reads) > 0 and all(isinstance(x, (bytes, bytearray)) for x in paths_or_reads))
        if in_memory:
            s, n = _stream_of(paths_or_reads)
            nm = None if names is None else "".join(x + "\n" for x in names).encode()
            _io_check(L.np2_sam_from_read_bytes(pol._h, index._h, s.ctypes.data if len(s) else None, len(s), n, nm, C.byref(o), C.byref(ao),
                                                C.byref(so), flags, C.byref(self._h)))
        else:
            if names is not None:
                raise TypeError("names go with reads in memory: read files carry their own")
            arr, n = _paths(paths_or_reads)
            _io_check(L.np2_sam_from_reads(pol._h, index._h, arr, n, C.byref(o), C.byref(ao), C.byref(so), flags, C.byref(self._h)))
        return self

    def refs(self):
        L = _bind()
        out = []
        for i in range(L.np2_sam_n_refs(self._h)):
            n = C.c_uint32()
            out.append((L.np2_sam_ref_name(self._h, i, C.byref(n)).decode(), n.value))
        return out

    def stats(self):
        st = np2_sam_stats_t()
        _io_check(_bind().np2_sam_stats(self._h, C.byref(st)))
        return _sam_stats_dict(st)

    def export(self, pol):
        """np2_sam_export: (recs, tids, cigar, seq4) as sam_parse_bytes returns them (parity tests)"""
        L = _bind()
        pr, pt, pc, ps, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        _io_check(L.np2_sam_export(pol._h, self._h, C.byref(pr), C.byref(pt), C.byref(pc), C.byref(ps), C.byref(n)))
        return _sam_arrays(L, pr, pt, pc, ps, n.value, self.stats())

    def write_bam(self, pol, path, bai=None):
        """np2_sam_write_bam: the coordinate-sorted BAM `path` and its index (`bai`, default path + ".bai"), assembled,
        compressed and indexed on the device; needs keep_names=True.  -> the np2_bamout_stats_t fields as a dict."""
        st = np2_bamout_stats_t()
        _io_check(_bind().np2_sam_write_bam(pol._h, self._h, os.fspath(path).encode(), os.fspath(bai).encode() if bai is not None else None,
                                            C.byref(st)))
        return _bamout_stats_dict(st)

    def bam_stream(self, pol):
        """np2_sam_bam_stream: the uncompressed BAM stream as bytes (tests)"""
        L = _bind()
        p, n = C.c_void_p(), C.c_uint64()
        _io_check(L.np2_sam_bam_stream(pol._h, self._h, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p.value, n.value)
        finally:
            L.np2_free(p)

    def export_names(self, pol):
        """np2_sam_export_names: (names uint8, name_ref uint64: offset << 8 | length per record in sorted order)"""
        L = _bind()
        pn, pr, nb, n = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        _io_check(L.np2_sam_export_names(pol._h, self._h, C.byref(pn), C.byref(nb), C.byref(pr), C.byref(n)))
        try:
            return (np.frombuffer(C.string_at(pn.value, nb.value), dtype=np.uint8).copy(),
                    np.frombuffer(C.string_at(pr.value, n.value * 8), dtype=np.uint64).copy())
        finally:
            L.np2_free(pn), L.np2_free(pr)

    def export_tails(self, pol):
        """np2_sam_export_tails (needs keep_all=True): (tails uint8, tail_ref uint64: offset << 1 | has_qual per record in sorted
        order).  A tail: next_refID, next_pos, tlen, aux_len (four words), the quality bytes if has_qual, the optional fields."""
        L = _bind()
        pt, pr, nb, n = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        _io_check(L.np2_sam_export_tails(pol._h, self._h, C.byref(pt), C.byref(nb), C.byref(pr), C.byref(n)))
        try:
            return (np.frombuffer(C.string_at(pt.value, nb.value), dtype=np.uint8).copy(),
                    np.frombuffer(C.string_at(pr.value, n.value * 8), dtype=np.uint64).copy())
        finally:
            L.np2_free(pt), L.np2_free(pr)

    def header_text(self):
        """np2_sam_header_text (needs keep_all=True): the header text of the full BAM as bytes"""
        p, n = C.c_void_p(), C.c_uint64()
        _io_check(_bind().np2_sam_header_text(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)

    def bamin_stats(self):
        """np2_sam_bamin_stats: of the inputs that were BAM: files, blocks, comp_bytes, inflated_bytes, records, and the HIP-event
        times inflate_ms, crc_ms, walk_ms, fields_ms, pack_ms summed over the pieces (zeros when no input was a BAM)"""
        st = np2_bamin_stats_t()
        _io_check(_bind().np2_sam_bamin_stats(self._h, C.byref(st)))
        return {n: (int if t is C.c_uint64 else float)(getattr(st, n)) for n, t in np2_bamin_stats_t._fields_}

    def tail_stats(self):
        """np2_sam_tail_stats: {tail_len_ms, tail_emit_ms, tail_bytes} of the two kernels keep_all=True adds"""
        a, b, n = C.c_float(), C.c_float(), C.c_uint64()
        _io_check(_bind().np2_sam_tail_stats(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return {"tail_len_ms": a.value, "tail_emit_ms": b.value, "tail_bytes": n.value}

    def close(self):
        if self._h:
            _bind().np2_sam_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bamout_stats_dict(st):
    return {n: (int if t is C.c_uint64 else float)(getattr(st, n)) for n, t in np2_bamout_stats_t._fields_}


def bamout_host(recs, tids, cigar, seq4, names, name_ref, refs, path=None, bai=None, want_stream=True, tails=None, tail_ref=None,
                header_text=None):
    """np2_bamout_host, the host twin of Sam.write_bam (no device): recs (BAMREC_DTYPE), tids, cigar and seq4 as Sam.export
    returns them, names / name_ref as Sam.export_names does, refs [(name, length)].  Writes `path` and its index when path is
    given.  tails / tail_ref (as Sam.export_tails returns them) and header_text (bytes, as Sam.header_text does), any of which
    is given: np2_bamout_host_full, the full stream.  -> (stream bytes or None, stats dict)."""
    L = _bind()
    full = tails is not None or tail_ref is not None or header_text is not None
    recs = np.ascontiguousarray(recs, dtype=BAMREC_DTYPE)
    tids, cigar = np.ascontiguousarray(tids, dtype=np.int32), np.ascontiguousarray(cigar, dtype=np.uint32)
    seq4, names = np.ascontiguousarray(seq4, dtype=np.uint8), np.ascontiguousarray(names, dtype=np.uint8)
    name_ref = np.ascontiguousarray(name_ref, dtype=np.uint64)
    if not (len(recs) == len(tids) == len(name_ref)):
        raise ValueError("recs, tids and name_ref must have one entry per record")
    rn = (C.c_char_p * max(len(refs), 1))(*[n.encode() for n, _ in refs])
    rl = np.ascontiguousarray([l for _, l in refs], dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if len(a) else None
    p, n, st = C.c_void_p(), C.c_uint64(), np2_bamout_stats_t()
    rest = (rn, ptr(rl), len(refs), os.fspath(path).encode() if path is not None else None,
            os.fspath(bai).encode() if bai is not None else None, C.byref(p) if want_stream else None,
            C.byref(n) if want_stream else None, C.byref(st))
    head = (ptr(recs), ptr(tids), ptr(cigar), ptr(seq4), len(recs), len(cigar), len(seq4), ptr(names), len(names), ptr(name_ref))
    if full:
        tails = np.ascontiguousarray(tails if tails is not None else [], dtype=np.uint8)
        tail_ref = np.ascontiguousarray(tail_ref, dtype=np.uint64) if tail_ref is not None else None
        if tail_ref is not None and len(tail_ref) != len(recs):
            raise ValueError("tail_ref must have one entry per record")
        ht = C.create_string_buffer(header_text, len(header_text)) if header_text is not None else None
        _io_check(L.np2_bamout_host_full(*head, ptr(tails), len(tails), tail_ref.ctypes.data if tail_ref is not None else None,
                                         C.addressof(ht) if ht is not None else None, len(header_text or b""), *rest))
    else:
        _io_check(L.np2_bamout_host(*head, *rest))
    try:
        return (C.string_at(p.value, n.value) if want_stream else None), _bamout_stats_dict(st)
    finally:
        L.np2_free(p)


def sam_tails_host(text):
    """np2_sam_tails_host (no device): SAM text (bytes, header included) walked by the one-lane text of the rule.  -> dict:
    tails (uint8), tail_ref (uint64), status (int32) and where (uint32), one entry per alignment line that is not empty;
    header_text (bytes); code and message: 0 and "" when no line is refused, else the status and message of the line that
    speaks.  A bad header raises Np2Error."""
    L = _bind()
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    pt, pr, ps, pw, ph = (C.c_void_p() for _ in range(5))
    nb, n, hb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = L.np2_sam_tails_host(buf.ctypes.data if len(buf) else None, len(buf), C.byref(pt), C.byref(nb), C.byref(pr), C.byref(ps), C.byref(pw),
                              C.byref(n), C.byref(ph), C.byref(hb))
    if not pr.value:
        _io_check(rc)
    try:
        take = lambda p, nbytes, dt: np.frombuffer(C.string_at(p.value, nbytes), dtype=dt).copy() if nbytes else np.zeros(0, dt)
        return dict(tails=take(pt, nb.value, np.uint8), tail_ref=take(pr, n.value * 8, np.uint64), status=take(ps, n.value * 4, np.int32),
                    where=take(pw, n.value * 4, np.uint32), header_text=C.string_at(ph.value, hb.value), code=rc,
                    message=L.np2_io_last_error().decode(errors="replace") if rc else "")
    finally:
        for p in (pt, pr, ps, pw, ph):
            L.np2_free(p)


def bamin_host(stream, keep_names=False, keep_all=False, tie="strand"):
    """np2_bamin_host (no device): an inflated BAM stream (bytes, header included) walked by the one-lane text of the rule.
    -> dict: status (int32) and where (uint32) per record in input order; of the kept records, in input order, recs
    (BAMREC_DTYPE), tids, cigar, seq4, names, name_ref, tails, tail_ref; code and message: 0 and "" when no record is refused,
    else the status and message of the first refused one.  A bad header raises Np2Error."""
    L = _bind()
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    o = _sam_opts(tie)
    flags = NP2_SAM_KEEP_ALL if keep_all else NP2_SAM_KEEP_NAMES if keep_names else 0
    p = {k: C.c_void_p() for k in ("status", "where", "recs", "tids", "cigar", "seq4", "names", "name_ref", "tails", "tail_ref")}
    n = {k: C.c_uint64() for k in ("records", "cigar", "seq4", "names", "tails", "kept")}
    rc = L.np2_bamin_host(buf.ctypes.data if len(buf) else None, len(buf), flags, C.byref(o), C.byref(p["status"]), C.byref(p["where"]),
                          C.byref(n["records"]), C.byref(p["recs"]), C.byref(p["tids"]), C.byref(p["cigar"]), C.byref(n["cigar"]),
                          C.byref(p["seq4"]), C.byref(n["seq4"]), C.byref(p["names"]), C.byref(n["names"]), C.byref(p["name_ref"]),
                          C.byref(p["tails"]), C.byref(n["tails"]), C.byref(p["tail_ref"]), C.byref(n["kept"]))
    if rc and not n["records"].value:
        _io_check(rc)
    try:
        take = lambda k, count, dt: (np.frombuffer(C.string_at(p[k].value, count * np.dtype(dt).itemsize), dtype=dt).copy()
                                     if count and p[k].value else np.zeros(0, dt))
        nr, nk = n["records"].value, n["kept"].value
        return dict(status=take("status", nr, np.int32), where=take("where", nr, np.uint32), recs=take("recs", nk, BAMREC_DTYPE),
                    tids=take("tids", nk, np.int32), cigar=take("cigar", n["cigar"].value, np.uint32), seq4=take("seq4", n["seq4"].value, np.uint8),
                    names=take("names", n["names"].value, np.uint8), name_ref=take("name_ref", nk if flags else 0, np.uint64),
                    tails=take("tails", n["tails"].value, np.uint8), tail_ref=take("tail_ref", nk if keep_all else 0, np.uint64), code=rc,
                    message=L.np2_io_last_error().decode(errors="replace") if rc else "")
    finally:
        for v in p.values():
            L.np2_free(v)


def _sam_arrays(L, pr, pt, pc, ps, n, stats):
    """the four malloc'ed arrays of np2_sam_parse_bytes / np2_sam_export as numpy arrays of their own; releases them"""
    try:
        take = lambda p, nbytes, dt: np.frombuffer(C.string_at(p.value, nbytes), dtype=dt).copy() if nbytes else np.zeros(0, dt)
        return (take(pr, n * BAMREC_DTYPE.itemsize, BAMREC_DTYPE), take(pt, n * 4, np.int32),
                take(pc, stats["cigar_words"] * 4, np.uint32), take(ps, stats["seq_bytes"], np.uint8))
    finally:
        for p in (pr, pt, pc, ps):
            L.np2_free(p)


def contig_from_sam(pol, sam, name, ref, opts=None):
    """The records of reference `name` of a resident Sam -> packed pileup resident in HBM (GPU columnariser).  -S
    (use_secondary) is not supported from SAM: use a BAM (Sam.write_bam or python -m nextpolish2_amd.samsort writes one)."""
    L = _bind()
    ref = np.frombuffer(ref, dtype=np.uint8) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, dtype=np.uint8)
    o = (opts or FrontOpts()).c()
    h = C.c_void_p()
    _io_check(L.np2_contig_from_sam(pol._h, sam._h, name.encode(), ref.ctypes.data, ref.shape[0], C.byref(o), C.byref(h)))
    return _resident(pol, h, name, int(ref.shape[0]))


def sam_parse_bytes(text, tie="strand", device=0):
    """np2_sam_parse_bytes: SAM text (bytes, header included) -> (recs as a BAMREC_DTYPE array in sorted order, tids int32,
    cigar uint32 in sorted order, seq4 uint8 as the records were met, stats dict).  For parity tests and measurements."""
    L = _bind()
    o = _sam_opts(tie)
    buf = np.frombuffer(text, dtype=np.uint8)
    pr, pt, pc, ps, n, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), np2_sam_stats_t()
    _io_check(L.np2_sam_parse_bytes(device, buf.ctypes.data if len(buf) else None, len(buf), C.byref(o), C.byref(pr), C.byref(pt),
                                    C.byref(pc), C.byref(ps), C.byref(n), C.byref(st)))
    stats = _sam_stats_dict(st)
    return _sam_arrays(L, pr, pt, pc, ps, n.value, stats) + (stats,)


def mapping_kind(path):
    """"bam" or "sam" for an alignment file, from its first bytes (gunzipped when they are gzip): BAM\1 is a BAM; a line
    that begins with @ or holds at least 10 tabs is SAM text.  Anything else is a ValueError naming the file."""
    import zlib
    with open(path, "rb") as f:
        head = f.read(65536)
    if head[:2] == b"\x1f\x8b":
        try:
            head = zlib.decompressobj(31).decompress(head, 65536)
        except zlib.error:
            raise ValueError(f"{path}: damaged gzip") from None
    if head[:4] == b"BAM\x01":
        return "bam"
    first = head.split(b"\n", 1)[0]
    if head[:1] == b"@" or first.count(b"\t") >= 10:
        return "sam"
    raise ValueError(f"{path}: neither a BAM nor SAM text")


def _resident(pol, h, name, L_, n_reads=0, n_cols=0):
    rc = ResidentContig.__new__(ResidentContig)
    rc._p, rc._h, rc.L, rc.n_reads, rc.n_columns, rc.name = pol, h, L_, n_reads, n_cols, name
    return rc


def contig_from_bam(pol, bam, name, ref, opts=None):
    """BAM records of contig `name` -> packed pileup resident in HBM (GPU columnariser)."""
    L = _bind()
    ref = np.frombuffer(ref, dtype=np.uint8) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, dtype=np.uint8)
    o = (opts or FrontOpts()).c()
    h = C.c_void_p()
    pol._check(L.np2_contig_from_bam(pol._h, bam._h, name.encode(), ref.ctypes.data, ref.shape[0], C.byref(o), C.byref(h)))
    return _resident(pol, h, name, int(ref.shape[0]))


def contig_from_records(pol, ref, recs, cigar, seq4, opts=None, name="ctg"):
    L = _bind()
    ref = np.frombuffer(ref, dtype=np.uint8) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, dtype=np.uint8)
    recs = np.ascontiguousarray(recs, dtype=BAMREC_DTYPE)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    seq4 = np.ascontiguousarray(seq4, dtype=np.uint8)
    o = (opts or FrontOpts()).c()
    h = C.c_void_p()
    pol._check(L.np2_contig_from_records(pol._h, ref.ctypes.data, ref.shape[0], recs.ctypes.data, recs.shape[0],
                                         cigar.ctypes.data, seq4.ctypes.data, C.byref(o), C.byref(h)))
    return _resident(pol, h, name, int(ref.shape[0]))


def depth_from_bam(pol, bam, name, L_, **kw):
    """np2_depth_from_bam: mapping depth of contig `name` (`L_` positions) of the indexed BAM `bam` on the device of Polisher
    `pol`, and its runs of depth >= min_depth that are at least min_len long -> (runs as an (n, 2) uint32 array of inclusive
    (s, e), stats dict, per-base depth or None).  Keywords as api.depth_from_records."""
    from .api import depth_call
    L = _bind()
    return depth_call(pol, L_, lambda *a: L.np2_depth_from_bam(pol._h, bam._h, name.encode(), int(L_), *a), **kw)


def shard_cuts(L_, n_shards):
    """The owned intervals np2_shard_plan gives a contig of L_ positions: cuts at L * k / n rounded down to 1024."""
    cuts = [0] + [((L_ * k) // n_shards) & ~1023 for k in range(1, n_shards)] + [L_]
    return list(zip(cuts[:-1], cuts[1:]))


class ShardFromBam:
    """One reference interval of a contig read straight from the BAM (np2_shard_bam_*): begin() fetches, admits and
    columnarises the records overlapping the interval +- halo and returns the file offsets this rank contributes to
    the numbering exchange; finish(all_offsets) returns (np2_contig_t* of the shard, its plan, the contig's read count)."""

    def __init__(self, pol, bam, name, ref, own_lo, own_hi, halo=65536, opts=None):
        from ._types import np2_shard_plan_t
        L = _bind()
        self._pol = pol
        ref = np.frombuffer(ref, dtype=np.uint8) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, dtype=np.uint8)
        self._ref = ref
        o = (opts or FrontOpts()).c()
        self._io = C.c_void_p()
        pv, n = C.c_void_p(), C.c_uint64()
        pol._check(L.np2_shard_bam_begin(pol._h, bam._h, name.encode(), ref.ctypes.data, ref.shape[0], own_lo, own_hi, halo,
                                         C.byref(o), C.byref(self._io), C.byref(pv), C.byref(n)))
        self.own_offsets = (np.frombuffer((C.c_uint8 * (8 * n.value)).from_address(pv.value), dtype=np.uint64).copy()
                            if n.value else np.zeros(0, dtype=np.uint64))
        self._plan_t = np2_shard_plan_t

    def finish(self, all_offsets):
        L = _bind()
        a = np.ascontiguousarray(all_offsets, dtype=np.uint64)
        plan = self._plan_t()
        h = C.c_void_p()
        n_total = C.c_uint32()
        io, self._io = self._io, None
        self._pol._check(L.np2_shard_bam_finish(io, a.ctypes.data, len(a), C.byref(plan), C.byref(h), C.byref(n_total)))
        return h, plan, n_total.value

    def abort(self):
        """Give the half-built shard up (another rank's shard failed: the contig is polished unsharded)."""
        if getattr(self, "_io", None):
            _bind().np2_shard_bam_abort(self._io)
            self._io = None

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


def export_contig(pol, contig, ref):
    """Copy a resident packed pileup back to the host as a Pileup (parity tests)."""
    L = _bind()
    pr, pn, nr, nb = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint64()
    pol._check(L.np2_contig_export(pol._h, contig._h, C.byref(pr), C.byref(nr), C.byref(pn), C.byref(nb)))
    reads = np.frombuffer(C.string_at(pr.value, nr.value * C.sizeof(np2_read_t)), dtype=READ_DTYPE).copy()
    nib = np.frombuffer(C.string_at(pn.value, nb.value), dtype=np.uint8).copy()
    L.np2_free(pr)
    L.np2_free(pn)
    return Pileup(ref, reads, nib)


def bgzf_inflate_device(pol, data):
    """np2_bgzf_inflate_device: a run of whole BGZF blocks (bytes / uint8 array) inflated on the polisher's device by the
    kernel np2_contig_from_bam uses -> (inflated bytes as a uint8 array, kernel milliseconds)."""
    L = _bind()
    src = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)
    # ISIZE of every block bounds the output: 64 KiB a block, a block is at least 28 bytes
    cap = max(1, (len(src) // 28 + 1)) * 65536
    cap = min(cap, max(1 << 20, len(src) * 1100))  # (deflate expands at most ~1032 x)
    out = np.empty(cap, dtype=np.uint8)
    n, ms = C.c_uint64(), C.c_float()
    rc = L.np2_bgzf_inflate_device(pol._h, src.ctypes.data, len(src), out.ctypes.data, cap, C.byref(n), C.byref(ms))
    if rc != 0:
        raise Np2Error(rc, "np2_bgzf_inflate_device: " + (L.np2_io_last_error() or b"").decode())
    return out[: n.value].copy(), float(ms.value)


def _u8(data):
    return np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)


def _bgzf_bound(n, block_bytes):
    """the most a BGZF stream of n bytes takes: every block stored (5 + 26 bytes around it), and the EOF block"""
    bb = block_bytes or 65280
    return n + (n + bb - 1) // bb * 31 + 28


def bgzf_deflate_device(pol, data, block_bytes=0):
    """np2_bgzf_deflate_device: bytes -> a whole BGZF stream (blocks of block_bytes input bytes, 0: 65280; then the EOF
    block), compressed on the polisher's device -> (the stream as bytes, milliseconds in the deflate kernel)."""
    L = _bind()
    src = _u8(data)
    cap = _bgzf_bound(len(src), block_bytes)
    out = np.empty(cap, dtype=np.uint8)
    n, ms = C.c_uint64(), C.c_float()
    rc = L.np2_bgzf_deflate_device(pol._h, src.ctypes.data if len(src) else None, len(src), block_bytes, out.ctypes.data, cap, C.byref(n), C.byref(ms))
    if rc != 0:
        raise Np2Error(rc, "np2_bgzf_deflate_device: " + (L.np2_io_last_error() or b"").decode())
    return out[: n.value].tobytes(), float(ms.value)


def bgzf_deflate_host(data, block_bytes=0):
    """np2_bgzf_deflate_host: the same stream computed on the CPU by the code the kernel's lanes run (no device)."""
    L = _bind()
    src = _u8(data)
    cap = _bgzf_bound(len(src), block_bytes)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_uint64()
    rc = L.np2_bgzf_deflate_host(src.ctypes.data if len(src) else None, len(src), block_bytes, out.ctypes.data, cap, C.byref(n))
    if rc != 0:
        raise Np2Error(rc, "np2_bgzf_deflate_host: " + (L.np2_io_last_error() or b"").decode())
    return out[: n.value].tobytes()


def is_bgzf_path(path):
    """the rule of every writer here: a path ending in .gz or .bgz is written as BGZF, any other as plain bytes"""
    return str(path).endswith((".gz", ".bgz"))


class BgzfWriter:
    """np2_bgzf_writer_*: a BGZF file compressed on `device`, blocks cut every 65280 bytes whatever the sizes of the
    writes.  close() appends the EOF block; a writer that failed leaves the file without it.  After close(): bytes_in,
    bytes_out, kernel_ms."""

    def __init__(self, path, device=0):
        self._L = _bind()
        self._h = C.c_void_p()
        self.bytes_in = self.bytes_out = 0
        self.kernel_ms = 0.0
        rc = self._L.np2_bgzf_writer_open(device, os.fsencode(path), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise Np2Error(rc, "np2_bgzf_writer_open: " + (self._L.np2_io_last_error() or b"").decode())

    def write(self, data):
        if not self._h:
            raise ValueError("write to a closed BgzfWriter")
        src = _u8(data.encode() if isinstance(data, str) else data)
        if len(src):
            rc = self._L.np2_bgzf_writer_write(self._h, src.ctypes.data, len(src))
            if rc != 0:
                raise Np2Error(rc, "np2_bgzf_writer_write: " + (self._L.np2_io_last_error() or b"").decode())
        return len(src)

    def close(self):
        if not self._h:
            return
        h, self._h = self._h, C.c_void_p()
        a, b, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        rc = self._L.np2_bgzf_writer_close(h, C.byref(a), C.byref(b), C.byref(ms))
        if rc != 0:
            raise Np2Error(rc, "np2_bgzf_writer_close: " + (self._L.np2_io_last_error() or b"").decode())
        self.bytes_in, self.bytes_out, self.kernel_ms = a.value, b.value, float(ms.value)

    def flush(self):
        """(a file object's: the blocks leave with their batch and at close())"""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def crc32_device(pol, data, offsets):
    """np2_crc32_device: CRC-32 (gzip) of the pieces data[offsets[i]:offsets[i + 1]] (each at most 65536 bytes) on the
    polisher's device, by the kernel that checks every inflated BGZF block -> (uint32 array, kernel milliseconds)."""
    L = _bind()
    src = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_pieces = max(0, len(off) - 1)
    out = np.zeros(max(1, n_pieces), dtype=np.uint32)
    ms = C.c_float()
    rc = L.np2_crc32_device(pol._h, src.ctypes.data if len(src) else None, len(src), off.ctypes.data if len(off) else None, n_pieces,
                            out.ctypes.data, C.byref(ms))
    if rc != 0:
        raise Np2Error(rc, "np2_crc32_device: " + (L.np2_io_last_error() or b"").decode())
    return out[:n_pieces].copy(), float(ms.value)


# ---- the mapper (include/np2_io.h: np2_map_*) -------------------------------------------------------------------------------
def map_opts(**kw):
    """np2_map_opts_t from keyword options; what is not given takes its default (MAP_DEFAULTS)"""
    unknown = set(kw) - set(MAP_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown mapping option(s): {sorted(unknown)}")
    vals = {**MAP_DEFAULTS, **{k: v for k, v in kw.items() if v is not None}}
    for k, v in vals.items():
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{k}: 0 .. 2^32 - 1")
    return np2_map_opts_t(*[int(vals[f]) for f, _ in np2_map_opts_t._fields_])


def map_opts_arg(text):
    """argparse type of --map_opts KEY=VAL,...: the keys of map_opts and align_opts (MAP_DEFAULTS, ALIGN_DEFAULTS) with
    non-negative integer values -> a dict; an unknown key or a bad value ends the parser (exit 2) before the library is loaded"""
    import argparse
    out = {}
    for item in filter(None, (x.strip() for x in text.split(","))):
        key, eq, val = item.partition("=")
        if key not in MAP_DEFAULTS and key not in ALIGN_DEFAULTS:
            raise argparse.ArgumentTypeError(f"unknown key {key!r} (the keys: {' '.join(list(MAP_DEFAULTS) + list(ALIGN_DEFAULTS))})")
        if not eq or not val.isdigit() or int(val) > 0xFFFFFFFF:
            raise argparse.ArgumentTypeError(f"{key}: a whole number in 0 .. 2^32 - 1 is expected, as in {key}={({**MAP_DEFAULTS, **ALIGN_DEFAULTS})[key]}")
        out[key] = int(val)
    return out


def _map_stats_dict(st):
    return {f: getattr(st, f) for f, _ in np2_map_stats_t._fields_}


def map_last_stats():
    """counts and stage times (HIP events, ms) of this thread's last mapping call"""
    st = np2_map_stats_t()
    _io_check(_bind().np2_map_last_stats(C.byref(st)))
    return _map_stats_dict(st)


def _stream_of(seqs):
    """a separator stream (bytes) or a list of sequences -> (uint8 array, number of sequences)"""
    if isinstance(seqs, (bytes, bytearray, memoryview, np.ndarray)):
        s = np.frombuffer(bytes(seqs), dtype=np.uint8) if not isinstance(seqs, np.ndarray) else np.ascontiguousarray(seqs, np.uint8)
        return s, int(np.count_nonzero(s == 10))
    seqs = [bytes(x) if not isinstance(x, str) else x.encode() for x in seqs]
    return np.frombuffer(b"".join(x + b"\n" for x in seqs), dtype=np.uint8), len(seqs)


def _map_result(L, call, s, n, want_chains):
    hits = np.zeros(n, MAP_HIT_DTYPE)
    if not want_chains:
        _io_check(call(s.ctypes.data if len(s) else None, len(s), n, hits.ctypes.data if n else None, None, None))
        return hits, None, None
    pc, off = C.c_void_p(), np.zeros(n + 1, np.uint64)
    _io_check(call(s.ctypes.data if len(s) else None, len(s), n, hits.ctypes.data if n else None, C.byref(pc), off.ctypes.data))
    try:
        m = int(off[n])
        from .api import _Raw
        chain = np.asarray(_Raw(pc.value, 2 * m, "<u4")).copy().reshape(m, 2) if m else np.zeros((0, 2), np.uint32)
    finally:
        L.np2_free(pc)
    return hits, chain, off


class MapWeights:
    """A weight set of the mapper (np2_map_weights_*; winnowmap -W): the repetitive k-mers that are made less likely to win a
    minimizer window.  `source`: a list file (one k-mer a line, as python -m nextpolish2_amd.repkmers writes it; plain or
    gzip), or canonical k-mer indices (api.rep_bytes' `index`) with their `k`.  Host memory only; `.k` (0: the empty set) and
    `.n_listed`.  A context manager."""

    def __init__(self, source, k=None):
        L = _bind()
        self._L, self._h = L, C.c_void_p()
        if isinstance(source, (str, bytes, os.PathLike)):
            if k is not None:
                raise TypeError("k is the list file's own: it is given with indices only")
            _io_check(L.np2_map_weights_from_file(os.fsencode(source), C.byref(self._h)))
        else:
            if k is None:
                raise TypeError("indices need their k")
            v = np.asarray(source)
            if v.size and (v.min() < 0 or v.max() > 0xFFFFFFFF):
                raise ValueError("an index is 0 .. 2^32 - 1")
            v = np.ascontiguousarray(v, np.uint32)
            _io_check(L.np2_map_weights_from_indices(int(k), v.ctypes.data if len(v) else None, len(v), C.byref(self._h)))
        k_, n_ = C.c_uint32(), C.c_uint64()
        _io_check(L.np2_map_weights_info(self._h, C.byref(k_), C.byref(n_)))
        self.k, self.n_listed = k_.value, n_.value

    @classmethod
    def from_assembly(cls, asm, k=15, distinct=0.9998, min_count=None, device=0):
        """the assembly's own repetitive k-mers, counted on `device` with repkmers' rule (api.rep_bytes).  asm: a FASTA path or
        a list of paths, or a separator stream (bytes) / a list of sequences in memory"""
        from . import api
        if isinstance(asm, (str, os.PathLike)):
            asm = [asm]
        if isinstance(asm, (list, tuple)) and asm and all(isinstance(x, (str, os.PathLike)) for x in asm):
            stream = b"".join(bytes(seqfile_stream(p)) for p in asm)
        else:
            stream = bytes(_stream_of(asm)[0])
        index, _, _ = api.rep_bytes(stream, k=k, distinct=distinct, min_count=min_count, device=device)
        return cls(index, k=k)

    def close(self):
        if self._h:
            self._L.np2_map_weights_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _weights_handle(weights):
    if weights is None:
        return None
    if not isinstance(weights, MapWeights):
        raise TypeError("weights: a MapWeights is expected")
    return weights._h


class MapIndex:
    """An assembly's minimizer index, resident on `device` (np2_map_index_*).  `asm`: a FASTA path or a list of paths, or
    (with stream=True) a separator stream / a list of sequences in memory, with `names` or numbered from 1.  `weights`: a
    MapWeights; the index copies what it needs and sketches the assembly and every read under it (`.weights_k`,
    `.weights_listed`; 0, 0 without)."""

    def __init__(self, asm, k=19, w=19, device=0, stream=False, names=None, weights=None):
        L = _bind()
        self._L, self._h = L, C.c_void_p()
        o = map_opts(k=k, w=w)
        wh = _weights_handle(weights)
        if stream:
            s, n = _stream_of(asm)
            nm = None if names is None else "".join(x + "\n" for x in names).encode()
            if wh is None:
                _io_check(L.np2_map_index_bytes(device, s.ctypes.data if len(s) else None, len(s), nm, C.byref(o), C.byref(self._h)))
            else:
                _io_check(L.np2_map_index_bytes_w(device, s.ctypes.data if len(s) else None, len(s), nm, C.byref(o), wh, C.byref(self._h)))
        else:
            arr, n = _paths(asm)
            if wh is None:
                _io_check(L.np2_map_index_files(device, arr, n, C.byref(o), C.byref(self._h)))
            else:
                _io_check(L.np2_map_index_files_w(device, arr, n, C.byref(o), wh, C.byref(self._h)))
        wk, wn = C.c_uint32(), C.c_uint64()
        _io_check(L.np2_map_index_weights(self._h, C.byref(wk), C.byref(wn)))
        self.weights_k, self.weights_listed = wk.value, wn.value
        k_, w_, ns, nm_, ms = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_float()
        _io_check(L.np2_map_index_info(self._h, C.byref(k_), C.byref(w_), C.byref(ns), C.byref(nm_), C.byref(ms)))
        self.k, self.w, self.n_minimizers, self.build_ms, self.device = k_.value, w_.value, nm_.value, ms.value, device
        self.names, self.lens = [], []
        for i in range(ns.value):
            name, ln = C.c_char_p(), C.c_uint64()
            _io_check(L.np2_map_index_seq(self._h, i, C.byref(name), C.byref(ln)))
            self.names.append(name.value.decode()), self.lens.append(ln.value)

    def close(self):
        if self._h:
            self._L.np2_map_index_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _opts(self, kw):
        return map_opts(k=self.k, w=self.w, **kw)

    def map(self, reads, chains=False, **kw):
        """map_reads(self, ...)"""
        return map_reads(self, reads, chains=chains, **kw)

    def align(self, reads, **kw):
        """np2_map_align_bytes: reads (a separator stream or a list of sequences) -> (hits, recs, cigar, cigar_off): recs an
        ALIGN_REC_DTYPE array, read i's CIGAR words (len << 4 | op) cigar[cigar_off[i] : cigar_off[i + 1]].  Options: MAP_DEFAULTS
        and ALIGN_DEFAULTS."""
        L = self._L
        s, n = _stream_of(reads)
        akw = {f: kw.pop(f) for f in list(kw) if f in ALIGN_DEFAULTS}
        o, ao = self._opts(kw), align_opts(**akw)
        return _align_result(L, lambda *a: L.np2_map_align_bytes(self._h, a[0], a[1], a[2], C.byref(o), C.byref(ao), a[3], a[4], a[5], a[6]), s, n)

    def align_x(self, reads, quals=None, md=False, cs=False, eqx=False, **kw):
        """np2_map_align_bytes_x: align() with the opt-in outputs (np2_io.h, "Tags") -> (hits, recs, cigar, cigar_off, md, cs): with
        eqx the CIGAR words hold = (7) and X (8) in place of M; md and cs are lists of bytes, one per read (b"" for an unaligned
        read), or None when not asked for.  quals: a quality stream of the reads' shape or a list with one entry per read (None or
        b"": that read has none); it is checked, and counted in align_last_tag_stats()."""
        L = self._L
        s, n = _stream_of(reads)
        akw = {f: kw.pop(f) for f in list(kw) if f in ALIGN_DEFAULTS}
        o, ao = self._opts(kw), align_opts(**akw)
        flags = (ALN_MD if md else 0) | (ALN_CS if cs else 0) | (ALN_EQX if eqx else 0)
        qs = None
        if quals is not None:
            flags |= ALN_QUAL
            qs = _qual_stream(quals, s, n)
            if len(qs) != len(s):
                raise ValueError(f"the quality stream has {len(qs)} bytes, the read stream {len(s)}")
        return _align_result_x(L, lambda *a: L.np2_map_align_bytes_x(self._h, a[0], None if qs is None or not len(qs) else qs.ctypes.data, a[1], a[2],
                                                                     C.byref(o), C.byref(ao), flags, *a[3:]), s, n, md, cs)


def multi_opts(multi=None, **kw):
    """np2_map_multi_opts_t (np2_io.h, "More chains") from a dict and / or keyword options; what is not given takes its
    default (MULTI_DEFAULTS: one chain per read, the plain mapper)"""
    if isinstance(multi, np2_map_multi_opts_t):
        return multi
    kw = {**(multi or {}), **kw}
    unknown = set(kw) - set(MULTI_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown multi-chain option(s): {sorted(unknown)}")
    vals = {**MULTI_DEFAULTS, **{k: v for k, v in kw.items() if v is not None}}
    for k, v in vals.items():
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{k}: 0 .. 2^32 - 1")
    return np2_map_multi_opts_t(*[int(vals[f]) for f, _ in np2_map_multi_opts_t._fields_])


def multi_chains_default(supplementary, secondary_n):
    """the command line's --max_chains when it is not given: 1 + N + 4 * supp, 16 at the most"""
    return min(16, 1 + int(secondary_n) + 4 * int(bool(supplementary)))


def map_last_multi_stats():
    """counts and the selection kernels' time (HIP events, ms) of this thread's last call with multi="""
    st = np2_map_multi_stats_t()
    _io_check(_bind().np2_map_last_multi_stats(C.byref(st)))
    return {f: getattr(st, f) for f, _ in np2_map_multi_stats_t._fields_}


def _units_result(L, call, s, n, want_chains):
    """an _m door's outputs -> (unit_off, hits, cls, parent[, chain, chain_off]): read i's units are unit_off[i] ..
    unit_off[i + 1], the primary first; chain rows of unit u are chain_off[u] .. chain_off[u + 1]"""
    from .api import _Raw
    unit_off = np.zeros(n + 1, np.uint64)
    ph, pc, pp, pch, pco = (C.c_void_p() for _ in range(5))
    try:
        _io_check(call(s.ctypes.data if len(s) else None, len(s), n, unit_off.ctypes.data, C.byref(ph), C.byref(pc), C.byref(pp),
                       C.byref(pch) if want_chains else None, C.byref(pco) if want_chains else None))
        m = int(unit_off[n])
        take = lambda p, cnt, dt: np.asarray(_Raw(p.value, cnt, dt)).copy() if cnt else np.zeros(0, dt)
        hits = take(ph, m * MAP_HIT_DTYPE.itemsize, "u1").view(MAP_HIT_DTYPE) if m else np.zeros(0, MAP_HIT_DTYPE)
        cls, parent = take(pc, m, "u1"), take(pp, m, "<u4")
        if not want_chains:
            return unit_off, hits, cls, parent
        off = take(pco, m + 1, "<u8")
        rows = int(off[m])
        chain = take(pch, 2 * rows, "<u4").reshape(rows, 2)
        return unit_off, hits, cls, parent, chain, off
    finally:
        for p in (ph, pc, pp, pch, pco):
            if p.value:
                L.np2_free(p)


def map_reads(index, reads, chains=False, multi=None, **kw):
    """np2_map_bytes: reads (a separator stream or a list of sequences) against a MapIndex -> hits, a MAP_HIT_DTYPE array
    with one entry per read (tid -1: unmapped); with chains=True -> (hits, chain, chain_off): the primary chains' anchors
    (r, q) as a uint32 [m, 2] array and read i's rows chain_off[i] .. chain_off[i + 1].  Options: MAP_DEFAULTS.
    With multi= (a dict of MULTI_DEFAULTS' keys): np2_map_bytes_m, per unit -> (unit_off, hits, cls, parent[, chain,
    chain_off]) as _units_result describes them."""
    L = _bind()
    s, n = _stream_of(reads)
    o = index._opts(kw)
    if multi is not None:
        m = multi_opts(multi)
        return _units_result(L, lambda *a: L.np2_map_bytes_m(index._h, a[0], a[1], a[2], C.byref(o), C.byref(m), *a[3:]), s, n, chains)
    hits, chain, off = _map_result(L, lambda *a: L.np2_map_bytes(index._h, a[0], a[1], a[2], C.byref(o), a[3], a[4], a[5]), s, n, chains)
    return (hits, chain, off) if chains else hits


def map_files(index, paths, out_path, multi=None, **kw):
    """np2_map_files: read files -> the PAF file out_path (BGZF when it ends in .gz / .bgz) -> the stats dict.  With multi=
    (a dict of MULTI_DEFAULTS' keys): np2_map_files_m, the further chains' lines behind each read's primary line"""
    L = _bind()
    arr, n = _paths(paths)
    o, st = index._opts(kw), np2_map_stats_t()
    out = None if out_path is None else os.fspath(out_path).encode()
    if multi is not None:
        m = multi_opts(multi)
        _io_check(L.np2_map_files_m(index._h, arr, n, C.byref(o), C.byref(m), out, C.byref(st)))
    else:
        _io_check(L.np2_map_files(index._h, arr, n, C.byref(o), out, C.byref(st)))
    return _map_stats_dict(st)


def map_host(asm, reads, chains=False, weights=None, multi=None, **kw):
    """np2_map_host / np2_map_host_w (no device): the same rule on the CPU -> what map_reads returns.  weights: a MapWeights.
    With multi=: np2_map_host_m, per unit, as map_reads returns it"""
    L = _bind()
    a, _ = _stream_of(asm)
    s, n = _stream_of(reads)
    o = map_opts(**kw)
    wh = _weights_handle(weights)
    ap = a.ctypes.data if len(a) else None
    if multi is not None:
        m = multi_opts(multi)
        return _units_result(L, lambda *x: L.np2_map_host_m(ap, len(a), x[0], x[1], x[2], C.byref(o), C.byref(m), wh, *x[3:]), s, n, chains)
    if wh is None:
        call = lambda *x: L.np2_map_host(ap, len(a), x[0], x[1], x[2], C.byref(o), x[3], x[4], x[5])
    else:
        call = lambda *x: L.np2_map_host_w(ap, len(a), x[0], x[1], x[2], C.byref(o), wh, x[3], x[4], x[5])
    hits, chain, off = _map_result(L, call, s, n, chains)
    return (hits, chain, off) if chains else hits


# ---- the aligner (include/np2_io.h: np2_map_align_*) --------------------------------------------------------------------------
def align_opts(**kw):
    """np2_align_opts_t from keyword options; what is not given takes its default (ALIGN_DEFAULTS)"""
    unknown = set(kw) - set(ALIGN_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown alignment option(s): {sorted(unknown)}")
    vals = {**ALIGN_DEFAULTS, **{k: v for k, v in kw.items() if v is not None}}
    for k, v in vals.items():
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{k}: 0 .. 2^32 - 1")
    return np2_align_opts_t(*[int(vals[f]) for f, _ in np2_align_opts_t._fields_])


def align_last_stats():
    """alignment counts and stage times (HIP events, ms) of this thread's last np2_map_align_* call"""
    st = np2_align_stats_t()
    _io_check(_bind().np2_map_align_last_stats(C.byref(st)))
    return {f: getattr(st, f) for f, _ in np2_align_stats_t._fields_}


def align_last_tag_stats():
    """np2_map_align_last_tag_stats: bytes and words of the opt-in outputs, reads that had qualities and the tag kernels' time (HIP
    events, ms) of this thread's last np2_map_align_*_x / np2_align_tags_* call"""
    st = np2_align_tag_stats_t()
    _io_check(_bind().np2_map_align_last_tag_stats(C.byref(st)))
    return {f: getattr(st, f) for f, _ in np2_align_tag_stats_t._fields_}


def _qual_stream(quals, s, n):
    """a quality stream beside the read stream s: as it is, or from a list with one entry per read (None / b"": 0xFF bytes)"""
    if not isinstance(quals, (list, tuple)):
        return np.frombuffer(bytes(quals), np.uint8)
    if len(quals) != n:
        raise ValueError(f"{n} reads and {len(quals)} quality strings")
    ends = np.flatnonzero(s == 10)
    out, start = [], 0
    for q, e in zip(quals, ends):
        out.append(bytes(q) if q else b"\xff" * int(e - start))
        out.append(b"\n")
        start = int(e) + 1
    return np.frombuffer(b"".join(out), np.uint8)


def _texts(L, pc, off, n):
    """a malloc'ed text block and its offsets -> a list of n bytes objects; the block is released"""
    try:
        whole = C.string_at(pc.value, int(off[n])) if int(off[n]) else b""
    finally:
        L.np2_free(pc)
    return [whole[int(off[i]):int(off[i + 1])] for i in range(n)]


def _align_result_x(L, call, s, n, md, cs):
    hits, recs = np.zeros(n, MAP_HIT_DTYPE), np.zeros(n, ALIGN_REC_DTYPE)
    pc, off = C.c_void_p(), np.zeros(n + 1, np.uint64)
    pm, moff, px, xoff = C.c_void_p(), np.zeros(n + 1, np.uint64), C.c_void_p(), np.zeros(n + 1, np.uint64)
    _io_check(call(s.ctypes.data if len(s) else None, len(s), n, hits.ctypes.data if n else None, recs.ctypes.data if n else None, C.byref(pc),
                   off.ctypes.data, C.byref(pm) if md else None, moff.ctypes.data if md else None, C.byref(px) if cs else None,
                   xoff.ctypes.data if cs else None))
    try:
        m = int(off[n])
        from .api import _Raw
        cigar = np.asarray(_Raw(pc.value, m, "<u4")).copy() if m else np.zeros(0, np.uint32)
    finally:
        L.np2_free(pc)
    return hits, recs, cigar, off, (_texts(L, pm, moff, n) if md else None), (_texts(L, px, xoff, n) if cs else None)


def _align_tags(L, call, ref, reads, t_off, q_off, cigars, md, cs, eqx):
    ref, reads = np.frombuffer(bytes(ref), np.uint8), np.frombuffer(bytes(reads), np.uint8)
    n = len(cigars)
    t_off, q_off = np.ascontiguousarray(t_off, np.uint64), np.ascontiguousarray(q_off, np.uint64)
    if len(t_off) != n or len(q_off) != n:
        raise ValueError(f"{n} CIGARs, {len(t_off)} t_off and {len(q_off)} q_off")
    coff = np.zeros(n + 1, np.uint64)
    coff[1:] = np.cumsum([len(c) for c in cigars])
    words = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint32).reshape(-1) for c in cigars]) if n else np.zeros(0), np.uint32)
    flags = (ALN_MD if md else 0) | (ALN_CS if cs else 0) | (ALN_EQX if eqx else 0)
    pm, moff, px, xoff, pe, eoff = C.c_void_p(), np.zeros(n + 1, np.uint64), C.c_void_p(), np.zeros(n + 1, np.uint64), C.c_void_p(), np.zeros(n + 1, np.uint64)
    _io_check(call(ref.ctypes.data if len(ref) else None, len(ref), reads.ctypes.data if len(reads) else None, len(reads), n,
                   t_off.ctypes.data if n else None, q_off.ctypes.data if n else None, words.ctypes.data if len(words) else None, coff.ctypes.data, flags,
                   C.byref(pm) if md else None, moff.ctypes.data if md else None, C.byref(px) if cs else None, xoff.ctypes.data if cs else None,
                   C.byref(pe) if eqx else None, eoff.ctypes.data if eqx else None))
    split = None
    if eqx:
        try:
            from .api import _Raw
            whole = np.asarray(_Raw(pe.value, int(eoff[n]), "<u4")).copy() if int(eoff[n]) else np.zeros(0, np.uint32)
        finally:
            L.np2_free(pe)
        split = [whole[int(eoff[i]):int(eoff[i + 1])] for i in range(n)]
    return (_texts(L, pm, moff, n) if md else None), (_texts(L, px, xoff, n) if cs else None), split


def align_tags_host(ref, reads, t_off, q_off, cigars, md=True, cs=True, eqx=True):
    """np2_align_tags_host (no device): the tag walk on caller-built records -> (md, cs, eqx), each a list with one entry per
    record (bytes, bytes, a uint32 array of CIGAR words) or None when not asked for.  ref, reads: byte buffers; record i's
    reference columns begin at ref[t_off[i]], its read, already oriented, at reads[q_off[i]]; cigars[i]: its words (len << 4 | op)."""
    L = _bind()
    return _align_tags(L, L.np2_align_tags_host, ref, reads, t_off, q_off, cigars, md, cs, eqx)


def align_tags_device(ref, reads, t_off, q_off, cigars, md=True, cs=True, eqx=True, device=0):
    """np2_align_tags_device: align_tags_host's records through the tag kernels"""
    L = _bind()
    return _align_tags(L, lambda *a: L.np2_align_tags_device(device, *a), ref, reads, t_off, q_off, cigars, md, cs, eqx)


def _chains_args(reads, hits, chains):
    """reads, hits (a MAP_HIT_DTYPE array, or a list of dicts with None for an unmapped read) and chains (a list of (n, 2)
    arrays, or the pair (chain, chain_off)) -> what np2_align_chains_* take"""
    s, n = _stream_of(reads)
    if not isinstance(hits, np.ndarray):
        h = np.zeros(len(hits), MAP_HIT_DTYPE)
        ends = np.flatnonzero(s == 10)
        starts = np.concatenate([[0], ends[:-1] + 1]) if len(ends) else ends
        for i, x in enumerate(hits):
            if x is None:
                h[i]["tid"], h[i]["qlen"] = -1, int(ends[i] - starts[i]) if i < len(ends) else 0
                continue
            for f in MAP_HIT_DTYPE.names:
                if f in x:
                    h[i][f] = x[f]
        hits = h
    hits = np.ascontiguousarray(hits, MAP_HIT_DTYPE)
    if isinstance(chains, tuple):
        chain, off = np.ascontiguousarray(chains[0], np.uint32).reshape(-1), np.ascontiguousarray(chains[1], np.uint64)
    else:
        parts = [np.asarray(c, np.uint32).reshape(-1, 2) for c in chains]
        off = np.zeros(len(parts) + 1, np.uint64)
        off[1:] = np.cumsum([len(c) for c in parts])
        chain = np.ascontiguousarray(np.concatenate(parts).reshape(-1) if parts else np.zeros(0), np.uint32)
    return s, n, hits, chain, off


def _chains_result(L, call, s, n, hits, chain, off, k, ao, probe):
    from .api import _Raw
    recs = np.zeros(n, ALIGN_REC_DTYPE)
    pc, coff = C.c_void_p(), np.zeros(n + 1, np.uint64)
    want = 0 if not probe else PROBE_SLOTS | PROBE_TB if probe is True else int(probe)
    pr = np2_align_probe_t(want=want)
    _io_check(call(s.ctypes.data if len(s) else None, len(s), n, k, hits.ctypes.data if len(hits) else None, chain.ctypes.data if len(chain) else None,
                   off.ctypes.data, C.byref(ao), recs.ctypes.data if n else None, C.byref(pc), coff.ctypes.data, C.byref(pr) if want else None))
    owned = [pc.value, pr.slot_off, pr.slots, pr.res, pr.tb_off, pr.tb]
    try:
        take = lambda p, m, dt: np.asarray(_Raw(p, m, dt)).copy() if p and m else np.zeros(0, dt)
        cigar = take(pc.value, int(coff[n]), "<u4")
        out = None
        if want:
            out, ns = {}, int(pr.n_slots)
            if want & PROBE_SLOTS:
                out["slot_off"] = take(pr.slot_off, n + 1, "<u8")
                out["slots"] = take(pr.slots, ns * 40, "|u1").view(ALIGN_SLOT_DTYPE)
                out["res"] = take(pr.res, ns * 12, "|u1").view(ALIGN_RES_DTYPE)
            if want & PROBE_TB:
                out["tb_off"] = take(pr.tb_off, ns + 1, "<u8")
                out["tb"] = take(pr.tb, int(out["tb_off"][ns]), "|u1")
    finally:
        for p in owned:
            if p:
                L.np2_free(C.c_void_p(p))
    return (recs, cigar, coff, out) if want else (recs, cigar, coff)


def align_chains_device(index, reads, hits, chains, probe=False, **kw):
    """np2_align_chains_device: the aligner's kernels on caller-built hits and chains against the index's assembly; nothing is
    sketched, seeded or chained -> (recs, cigar, cigar_off) and, with probe (True, or a sum of PROBE_SLOTS and PROBE_TB), a dict of
    slot_off, slots (ALIGN_SLOT_DTYPE), res (ALIGN_RES_DTYPE), tb_off and tb.  hits, chains: see _chains_args.  Options:
    ALIGN_DEFAULTS, and k (the index's)."""
    L = index._L
    k = int(kw.pop("k", index.k))
    s, n, hits, chain, off = _chains_args(reads, hits, chains)
    ao = align_opts(**kw)
    return _chains_result(L, lambda *a: L.np2_align_chains_device(index._h, *a), s, n, hits, chain, off, k, ao, probe)


def align_chains_host(asm, reads, hits, chains, k=19, probe=False, **kw):
    """np2_align_chains_host (no device): align_chains_device through the host aligner, against an assembly in memory"""
    L = _bind()
    a, _ = _stream_of(asm)
    s, n, hits, chain, off = _chains_args(reads, hits, chains)
    ao = align_opts(**kw)
    return _chains_result(L, lambda *x: L.np2_align_chains_host(a.ctypes.data if len(a) else None, len(a), *x), s, n, hits, chain, off, int(k), ao, probe)


def _align_result(L, call, s, n):
    hits, recs = np.zeros(n, MAP_HIT_DTYPE), np.zeros(n, ALIGN_REC_DTYPE)
    pc, off = C.c_void_p(), np.zeros(n + 1, np.uint64)
    _io_check(call(s.ctypes.data if len(s) else None, len(s), n, hits.ctypes.data if n else None, recs.ctypes.data if n else None, C.byref(pc),
                   off.ctypes.data))
    try:
        m = int(off[n])
        from .api import _Raw
        cigar = np.asarray(_Raw(pc.value, m, "<u4")).copy() if m else np.zeros(0, np.uint32)
    finally:
        L.np2_free(pc)
    return hits, recs, cigar, off


def _aligned_units(L, call, n, md, cs):
    """an aligned _m door's outputs -> a dict: unit_off, hits, cls, parent, recs, cigar, cigar_off and, when asked for, md and cs
    as lists of bytes, one per unit"""
    from .api import _Raw
    unit_off, out = np.zeros(n + 1, np.uint64), np2_map_units_t()
    try:
        _io_check(call(unit_off.ctypes.data, C.byref(out)))
        m = int(out.n_units)
        take = lambda p, cnt, dt: np.asarray(_Raw(p, cnt, dt)).copy() if cnt else np.zeros(0, dt)
        r = dict(unit_off=unit_off, hits=take(out.hits, m * MAP_HIT_DTYPE.itemsize, "u1").view(MAP_HIT_DTYPE),
                 cls=take(out.cls, m, "u1"), parent=take(out.parent, m, "<u4"),
                 recs=take(out.recs, m * ALIGN_REC_DTYPE.itemsize, "u1").view(ALIGN_REC_DTYPE), cigar_off=take(out.cigar_off, m + 1, "<u8"))
        r["cigar"] = take(out.cigar, int(r["cigar_off"][m]), "<u4")
        for key, want, p, po in (("md", md, out.md, out.md_off), ("cs", cs, out.cs, out.cs_off)):
            r[key] = None
            if want:
                off = take(po, m + 1, "<u8")
                text = bytes(take(p, int(off[m]), "u1"))
                r[key] = [text[int(off[i]):int(off[i + 1])] for i in range(m)]
        return r
    finally:
        for f, _ in np2_map_units_t._fields_[1:]:
            if getattr(out, f):
                L.np2_free(getattr(out, f))


def map_align_reads_m(index, reads, multi, quals=None, md=False, cs=False, eqx=False, **kw):
    """np2_map_align_bytes_m: MapIndex.align_x per unit (np2_io.h, "More chains") -> the dict of _aligned_units"""
    L = _bind()
    s, n = _stream_of(reads)
    akw = {f: kw.pop(f) for f in list(kw) if f in ALIGN_DEFAULTS}
    o, ao, m = index._opts(kw), align_opts(**akw), multi_opts(multi)
    flags = (ALN_MD if md else 0) | (ALN_CS if cs else 0) | (ALN_EQX if eqx else 0)
    qs = None
    if quals is not None:
        flags |= ALN_QUAL
        qs = _qual_stream(quals, s, n)
    return _aligned_units(L, lambda uo, out: L.np2_map_align_bytes_m(index._h, s.ctypes.data if len(s) else None,
                                                                     None if qs is None or not len(qs) else qs.ctypes.data, len(s), n, C.byref(o),
                                                                     C.byref(m), C.byref(ao), flags, uo, out), n, md, cs)


def map_align_host_m(asm, reads, multi, weights=None, md=False, cs=False, eqx=False, **kw):
    """np2_map_align_host_m (no device): map_align_host_x per unit -> the dict of _aligned_units"""
    L = _bind()
    a, _ = _stream_of(asm)
    s, n = _stream_of(reads)
    akw = {f: kw.pop(f) for f in list(kw) if f in ALIGN_DEFAULTS}
    o, ao, m = map_opts(**kw), align_opts(**akw), multi_opts(multi)
    flags = (ALN_MD if md else 0) | (ALN_CS if cs else 0) | (ALN_EQX if eqx else 0)
    return _aligned_units(L, lambda uo, out: L.np2_map_align_host_m(a.ctypes.data if len(a) else None, len(a), s.ctypes.data if len(s) else None, len(s),
                                                                    n, C.byref(o), C.byref(m), C.byref(ao), _weights_handle(weights), flags, uo, out),
                          n, md, cs)


def map_align_files(index, paths, out_path, qual=False, md=False, cs=False, eqx=False, multi=None, **kw):
    """np2_map_align_files: read files -> the SAM file out_path (BGZF when it ends in .gz / .bgz) -> the mapper's stats dict.
    With qual / md / cs / eqx (np2_map_align_files_x; np2_io.h, "Tags"): QUAL from FASTQ input, MD:Z: and cs:Z: behind s2:i:,
    = and X in the CIGAR.  With multi= (np2_map_align_files_m; "More chains"): the further units' records behind each primary."""
    L = _bind()
    arr, n = _paths(paths)
    akw = {f: kw.pop(f) for f in list(kw) if f in ALIGN_DEFAULTS}
    o, ao, st = index._opts(kw), align_opts(**akw), np2_map_stats_t()
    flags = (ALN_QUAL if qual else 0) | (ALN_MD if md else 0) | (ALN_CS if cs else 0) | (ALN_EQX if eqx else 0)
    if multi is not None:
        m = multi_opts(multi)
        _io_check(L.np2_map_align_files_m(index._h, arr, n, C.byref(o), C.byref(m), C.byref(ao), flags,
                                          None if out_path is None else os.fspath(out_path).encode(), C.byref(st)))
        return _map_stats_dict(st)
    if flags:
        _io_check(L.np2_map_align_files_x(index._h, arr, n, C.byref(o), C.byref(ao), flags, None if out_path is None else os.fspath(out_path).encode(),
                                          C.byref(st)))
        return _map_stats_dict(st)
    _io_check(L.np2_map_align_files(index._h, arr, n, C.byref(o), C.byref(ao), None if out_path is None else os.fspath(out_path).encode(),
                                    C.byref(st)))
    return _map_stats_dict(st)


def align_pack_host(recs, cigar, cigar_off, reads, tie="strand"):
    """np2_align_pack_host (no device): the aligner's output for `reads` (what MapIndex.align or map_align_host returns: recs,
    cigar, cigar_off) -> (recs as a BAMREC_DTYPE array in sorted order, tids, cigar in sorted order, seq4 as the reads were met):
    what Sam.from_reads(...).export() returns, from the same rule text as the kernels."""
    L = _bind()
    s, n = _stream_of(reads)
    recs = np.ascontiguousarray(recs, ALIGN_REC_DTYPE)
    cigar, off = np.ascontiguousarray(cigar, np.uint32), np.ascontiguousarray(cigar_off, np.uint64)
    if len(recs) != n or len(off) != n + 1:
        raise ValueError(f"{n} reads, {len(recs)} records and {len(off)} CIGAR offsets")
    o = _sam_opts(tie)
    pr, pt, pc, ps, m = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    _io_check(L.np2_align_pack_host(recs.ctypes.data if n else None, cigar.ctypes.data if len(cigar) else None, off.ctypes.data,
                                    s.ctypes.data if len(s) else None, len(s), n, C.byref(o), C.byref(pr), C.byref(pt), C.byref(pc), C.byref(ps),
                                    C.byref(m)))
    out = np.frombuffer(C.string_at(pr.value, m.value * BAMREC_DTYPE.itemsize), dtype=BAMREC_DTYPE) if m.value else np.zeros(0, BAMREC_DTYPE)
    sizes = {"cigar_words": int(out["n_cigar"].sum()), "seq_bytes": int(((out["l_seq"].astype(np.int64) + 1) // 2).sum())}
    return _sam_arrays(L, pr, pt, pc, ps, m.value, sizes)


def map_align_host(asm, reads, weights=None, **kw):
    """np2_map_align_host / np2_map_align_host_w (no device): the same rule on the CPU -> what MapIndex.align returns"""
    L = _bind()
    a, _ = _stream_of(asm)
    s, n = _stream_of(reads)
    akw = {f: kw.pop(f) for f in list(kw) if f in ALIGN_DEFAULTS}
    o, ao = map_opts(**kw), align_opts(**akw)
    wh = _weights_handle(weights)
    if wh is not None:
        return _align_result(L, lambda *x: L.np2_map_align_host_w(a.ctypes.data if len(a) else None, len(a), x[0], x[1], x[2], C.byref(o),
                                                                  C.byref(ao), wh, x[3], x[4], x[5], x[6]), s, n)
    return _align_result(L, lambda *x: L.np2_map_align_host(a.ctypes.data if len(a) else None, len(a), x[0], x[1], x[2], C.byref(o), C.byref(ao),
                                                            x[3], x[4], x[5], x[6]), s, n)


def map_align_host_x(asm, reads, weights=None, md=False, cs=False, eqx=False, **kw):
    """np2_map_align_host_x (no device): map_align_host with the opt-in outputs -> what MapIndex.align_x returns"""
    L = _bind()
    a, _ = _stream_of(asm)
    s, n = _stream_of(reads)
    akw = {f: kw.pop(f) for f in list(kw) if f in ALIGN_DEFAULTS}
    o, ao = map_opts(**kw), align_opts(**akw)
    wh = _weights_handle(weights)
    flags = (ALN_MD if md else 0) | (ALN_CS if cs else 0) | (ALN_EQX if eqx else 0)
    return _align_result_x(L, lambda *x: L.np2_map_align_host_x(a.ctypes.data if len(a) else None, len(a), x[0], x[1], x[2], C.byref(o), C.byref(ao),
                                                                wh, flags, *x[3:]), s, n, md, cs)
