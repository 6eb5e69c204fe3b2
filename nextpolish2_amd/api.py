"""ctypes binding of libnp2_hip.so — the C-ABI of include/np2.h.

There is no CPU fallback: importing is fine without a GPU (symbols can be inspected), but
creating a Polisher requires the in-tree HIP library and a visible MI355X device.
"""
import contextlib
import ctypes as C
import os
import weakref

import numpy as np

from ._types import (Opts, Pileup, np2_opts_t, np2_read_t, np2_shard_piece_t, np2_shard_plan_t, np2_vote_t, np2_yak_t,
                     yaks_array)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NP2_LIB_PATH") or os.path.join(_HERE, "libnp2_hip.so")  # override: A/B builds
_LIB = None

# every symbol include/np2.h declares
ABI_SYMBOLS = [
    "np2_ctx_create", "np2_ctx_destroy", "np2_last_error", "np2_ctx_stream", "np2_contig_upload",
    "np2_contig_free", "np2_polish_resident", "np2_polish_contig", "np2_free", "np2_score_strings",
    "np2_lookup_hashes", "np2_ctx_set_trace", "np2_ctx_set_timing", "np2_trace_get", "np2_last_timings", "np2_last_span", "np2_last_result_device", "np2_result_fetch_begin", "np2_result_fetch_end", "np2_phase_vote",
    "np2_ctx_create_shared", "np2_batch_create", "np2_batch_destroy", "np2_batch_slots", "np2_batch_slot_ctx", "np2_batch_set_sink",
    "np2_batch_last_error", "np2_batch_polish", "np2_batch_flush_log", "np2_shard_plan", "np2_shard_upload",
    "np2_shard_begin", "np2_shard_passes_left", "np2_shard_vote", "np2_vote_decide", "np2_shard_apply", "np2_shard_final",
    "np2_shard_final_device", "np2_shard_fetch", "np2_alloc_pinned", "np2_trim_device_cache",
    "np2_shard_end", "np2_swiss_order", "np2_debug_poison", "np2_debug_poison_stats", "np2_batch_set_timing", "np2_batch_set_priority", "np2_batch_last_diff_ms", "np2_batch_stats", "np2_batch_last_call_ms",
    "np2_qv_strings", "np2_qv_device", "np2_trio_strings", "np2_trio_device", "np2_bin_stream",
    "np2_cmp_strings",
    "np2_edits_buffers", "np2_edits_last", "np2_edits_free",
]

# include/np2_io.h (input side; bound by nextpolish2_amd.io)
IO_ABI_SYMBOLS = [
    "np2_fasta_open", "np2_fasta_next", "np2_fasta_close", "np2_yak_load", "np2_yak_free", "np2_bam_open", "np2_bam_close",
    "np2_bam_n_refs", "np2_bam_ref_name", "np2_io_last_error", "np2_contig_from_records", "np2_contig_from_bam",
    "np2_contig_export", "np2_shard_bam_begin", "np2_shard_bam_finish", "np2_shard_bam_abort", "np2_ctx_create_from_files",
    "np2_bgzf_inflate_device", "np2_crc32_device",
    "np2_bgzf_deflate_device", "np2_bgzf_deflate_host", "np2_bgzf_writer_open", "np2_bgzf_writer_write", "np2_bgzf_writer_close",
    "np2_kcount_files", "np2_kcount_bytes", "np2_kcount_files_to_dumps", "np2_ctx_create_from_reads", "np2_kcount_last_stats",
    "np2_seqfile_stream", "np2_bin_files", "np2_seqfile_reads",
    "np2_depth_from_records", "np2_depth_from_bam",
    "np2_varcall_from_records", "np2_varcall_from_bam", "np2_varcall_host",
    "np2_asmcall", "np2_asmcall_host",
    "np2_srqc_bytes", "np2_srqc_files", "np2_srqc_last_stats", "np2_srqc_last_kernel_ms", "np2_kcount_files_qc",
    "np2_kcount_files_to_dumps_qc", "np2_ctx_create_from_reads_qc", "np2_seqfile_stream_qual",
    "np2_sradapt_bytes", "np2_sradapt_files", "np2_sradapt_last_stats", "np2_sradapt_last_kernel_ms", "np2_kcount_files_ad",
    "np2_kcount_files_to_dumps_ad", "np2_ctx_create_from_reads_ad",
    "np2_rep_bytes", "np2_rep_files",
    "np2_map_index_bytes", "np2_map_index_files", "np2_map_index_free", "np2_map_index_info", "np2_map_index_seq", "np2_map_bytes",
    "np2_map_files", "np2_map_host", "np2_map_last_stats",
    "np2_map_bytes_m", "np2_map_files_m", "np2_map_host_m", "np2_map_last_multi_stats",
    "np2_map_align_bytes_m", "np2_map_align_files_m", "np2_map_align_host_m",
    "np2_map_weights_from_indices", "np2_map_weights_from_file", "np2_map_weights_info", "np2_map_weights_free",
    "np2_map_index_bytes_w", "np2_map_index_files_w", "np2_map_index_weights", "np2_map_host_w", "np2_map_align_host_w",
    "np2_map_align_bytes", "np2_map_align_files", "np2_map_align_host", "np2_map_align_last_stats",
    "np2_map_align_bytes_x", "np2_map_align_files_x", "np2_map_align_host_x", "np2_align_tags_device", "np2_align_tags_host",
    "np2_map_align_last_tag_stats", "np2_align_chains_device", "np2_align_chains_host",
    "np2_sam_open", "np2_sam_close", "np2_sam_n_refs", "np2_sam_ref_name", "np2_sam_stats", "np2_contig_from_sam",
    "np2_sam_parse_bytes", "np2_sam_export", "np2_sam_from_reads", "np2_sam_from_read_bytes", "np2_align_pack_host",
    "np2_sam_open_ex", "np2_sam_write_bam", "np2_sam_bam_stream", "np2_bamout_host", "np2_sam_export_names",
    "np2_sam_export_tails", "np2_sam_header_text", "np2_sam_tail_stats", "np2_bamout_host_full", "np2_sam_tails_host", "np2_sam_bamin_stats", "np2_bamin_host",
]

ERRORS = {-1: "NP2_E_ARG", -2: "NP2_E_DEVICE", -3: "NP2_E_NOMEM", -4: "NP2_E_UNSUPPORTED", -5: "NP2_E_REFPANIC"}


class np2_bin_opts_t(C.Structure):
    _fields_ = [("min_count", C.c_uint16), ("mid_count", C.c_uint16), ("min_score", C.c_uint32), ("minor_permille", C.c_uint32)]


class np2_depth_opts_t(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_len", C.c_uint32), ("min_aligned_fra", C.c_double), ("exclude_flags", C.c_uint16),
                ("min_mapq", C.c_uint8)]


class np2_depth_stats_t(C.Structure):
    _fields_ = [("records_seen", C.c_uint64), ("records_counted", C.c_uint64), ("sum_depth", C.c_uint64), ("bases_kept", C.c_uint64),
                ("max_depth", C.c_uint32), ("bases_ok", C.c_uint32), ("runs", C.c_uint32), ("runs_kept", C.c_uint32),
                ("kernel_ms", C.c_float)]


assert C.sizeof(np2_depth_opts_t) == 24 and C.sizeof(np2_depth_stats_t) == 56


class np2_varcall_opts_t(C.Structure):
    _fields_ = [("min_aligned_fra", C.c_double), ("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("hom_pm", C.c_uint32),
                ("het_pm", C.c_uint32), ("max_indel", C.c_uint32), ("exclude_flags", C.c_uint16), ("min_mapq", C.c_uint8)]


class np2_varcall_stats_t(C.Structure):
    _fields_ = [("records_seen", C.c_uint64), ("records_counted", C.c_uint64), ("records_no_seq", C.c_uint64),
                ("records_skipped", C.c_uint64), ("events", C.c_uint64), ("alleles", C.c_uint64), ("callable", C.c_uint64),
                ("calls", C.c_uint64 * 6), ("kernel_ms", C.c_float), ("stage_ms", C.c_float * 6), ("pad", C.c_uint32)]


VARCALL_DTYPE = np.dtype([("pos", "<u4"), ("depth", "<u4"), ("count", "<u4"), ("pad0", "<u4"), ("bases", "<u8"), ("kind", "u1"),
                          ("gt", "u1"), ("len", "u1"), ("alt_code", "u1"), ("pad1", "<u4")])  # np2_varcall_t
VARCALL_KINDS = ("SNV", "DEL", "INS")
VARCALL_STAGES = ("records", "scan", "sorts", "alleles", "count", "emit")  # np2_varcall_stats_t.stage_ms
VARCALL_CALLS = ("snv_het", "snv_hom", "del_het", "del_hom", "ins_het", "ins_hom")  # np2_varcall_stats_t.calls
assert C.sizeof(np2_varcall_opts_t) == 32 and C.sizeof(np2_varcall_stats_t) == 136 and VARCALL_DTYPE.itemsize == 32


class np2_asmcall_opts_t(C.Structure):
    _fields_ = [("min_mapq", C.c_uint32), ("min_aln", C.c_uint32)]


class np2_asmcall_stats_t(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("alns_seen", "alns_admitted", "alns_skipped", "alns_low_mapq", "alns_short", "alns_unaligned", "runs",
                                          "r_bases", "cov0_bases", "cov2_bases")] + \
               [("found", C.c_uint64 * 3), ("kept", C.c_uint64 * 3), ("ins_bases", C.c_uint64), ("del_bases", C.c_uint64),
                ("kernel_ms", C.c_float), ("stage_ms", C.c_float * 9)]


ASMALN_DTYPE = np.dtype([("tid", "<i4")] + [(f, "<u4") for f in ("pos", "flag", "mapq", "n_cigar", "q_len", "own_lo", "own_hi", "q_id", "q_base")] +
                        [("cigar_off", "<u8"), ("q_off", "<u8")])  # np2_asmaln_t
ASMRUN_DTYPE = np.dtype([("tid", "<u4"), ("start", "<u4"), ("end", "<u4")])  # np2_asmrun_t
ASMVAR_DTYPE = np.dtype([(f, "<u4") for f in ("tid", "pos", "aln", "len", "q_pos")] +
                        [(f, "u1") for f in ("kind", "ref_code", "alt_code", "rev")])  # np2_asmvar_t
ASMCALL_KINDS = ("SNV", "DEL", "INS")
ASMCALL_STAGES = ("count", "cov_scan", "ones", "offsets", "emit", "runs", "filter", "sort", "gather")  # np2_asmcall_stats_t.stage_ms
assert C.sizeof(np2_asmcall_opts_t) == 8 and C.sizeof(np2_asmcall_stats_t) == 184
assert ASMALN_DTYPE.itemsize == 56 and ASMRUN_DTYPE.itemsize == 12 and ASMVAR_DTYPE.itemsize == 24


class np2_rep_opts_t(C.Structure):
    _fields_ = [("k", C.c_uint32), ("use_min_count", C.c_uint32), ("min_count", C.c_uint32), ("distinct", C.c_double)]


class np2_rep_stats_t(C.Structure):
    _fields_ = [("kmers", C.c_uint64), ("distinct", C.c_uint64), ("listed", C.c_uint64), ("listed_occurrences", C.c_uint64),
                ("threshold", C.c_uint32), ("max_count", C.c_uint32), ("count_ms", C.c_float), ("select_ms", C.c_float),
                ("emit_ms", C.c_float)]


assert C.sizeof(np2_rep_opts_t) == 24 and np2_rep_opts_t.distinct.offset == 16 and C.sizeof(np2_rep_stats_t) == 56

class np2_edits_opts_t(C.Structure):
    _fields_ = [("min_count", C.c_uint16), ("tables", C.c_int32)]


class np2_edits_t(C.Structure):
    _fields_ = [("n_edits", C.c_uint32), ("n_tables", C.c_uint32), ("edits", C.c_void_p), ("ref_off", C.c_void_p),
                ("alt_off", C.c_void_p), ("ref_pool", C.c_void_p), ("alt_pool", C.c_void_p), ("support", C.c_void_p),
                ("table_idx", C.c_uint32 * 8), ("table_k", C.c_uint32 * 8), ("has_span", C.c_uint32), ("first_pos", C.c_uint32),
                ("last_pos", C.c_uint32), ("pad", C.c_uint32), ("raw_runs", C.c_uint64), ("same_runs", C.c_uint64),
                ("n_kind", C.c_uint64 * 5), ("bases_inserted", C.c_uint64), ("bases_deleted", C.c_uint64),
                ("outside_span", C.c_uint64), ("kernel_ms", C.c_float * 6)]


assert C.sizeof(np2_edits_opts_t) == 8 and C.sizeof(np2_edits_t) == 240 and np2_edits_t.raw_runs.offset == 136

EDIT_DTYPE = np.dtype([("ref_pos", "<u4"), ("ref_len", "<u4"), ("out_off", "<u4"), ("alt_len", "<u4"), ("kind", "<u4")])  # np2_edit_t
EDIT_KINDS = ("SNV", "MNV", "INS", "DEL", "CPX")
EDIT_STAGES = ("flags", "runs", "trim", "shift", "emit", "support")
BIN_DTYPE = np.dtype([("n_kmers", "<u4"), ("n_pat", "<u4"), ("n_mat", "<u4"), ("pairs", "<u4", (4,))])  # np2_bin_t
assert BIN_DTYPE.itemsize == 28


class Np2Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


_LIB_LOCK = __import__("threading").Lock()


def lib():
    """Load libnp2_hip.so; raises loudly if the HIP extension has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LIB_LOCK:
        return _lib_locked()


def _lib_locked():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with nextpolish2_amd/csrc/build.sh "
                "(the np2 hot path has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        vp, u32, u64, u16 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint16
        L.np2_ctx_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(np2_yak_t), C.c_int]
        L.np2_ctx_destroy.argtypes = [vp]
        L.np2_last_error.restype = C.c_char_p
        L.np2_last_error.argtypes = [vp]
        L.np2_ctx_stream.restype = vp
        L.np2_ctx_stream.argtypes = [vp]
        L.np2_contig_upload.argtypes = [vp, vp, u32, vp, u32, vp, u64, C.POINTER(vp)]
        L.np2_contig_free.argtypes = [vp, vp]
        L.np2_polish_resident.argtypes = [vp, vp, C.POINTER(np2_opts_t), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
        L.np2_polish_contig.argtypes = [vp, vp, u32, vp, u32, vp, u64, C.POINTER(np2_opts_t), C.POINTER(vp),
                                        C.POINTER(vp), C.POINTER(u64)]
        L.np2_free.argtypes = [vp]
        L.np2_score_strings.argtypes = [vp, C.c_int, vp, vp, u64, u16, vp]
        L.np2_lookup_hashes.argtypes = [vp, C.c_int, vp, u64, u16, vp]
        L.np2_qv_strings.argtypes = [vp, C.c_int, vp, vp, u64, u16, vp, vp, vp, C.POINTER(C.c_float)]
        L.np2_qv_device.argtypes = [vp, C.c_int, vp, u64, u16, vp, vp, vp, C.POINTER(C.c_float)]
        L.np2_trio_strings.argtypes = [vp, C.c_int, C.c_int, vp, vp, u64, u16, u16, vp, vp, vp, C.POINTER(C.c_float)]
        L.np2_trio_device.argtypes = [vp, C.c_int, C.c_int, vp, u64, u16, u16, vp, vp, vp, C.POINTER(C.c_float)]
        L.np2_bin_stream.argtypes = [vp, C.c_int, C.c_int, vp, u64, u64, C.POINTER(np2_bin_opts_t), vp, vp, C.POINTER(C.c_float)]
        L.np2_cmp_strings.argtypes = [vp, C.c_int, vp, vp, u64, u16, vp, vp, vp, C.POINTER(C.c_float)]
        L.np2_edits_buffers.argtypes = [vp, vp, u32, vp, vp, u64, C.POINTER(np2_edits_opts_t), C.POINTER(np2_edits_t)]
        L.np2_edits_last.argtypes = [vp, vp, C.POINTER(np2_edits_opts_t), C.POINTER(np2_edits_t)]
        L.np2_edits_free.argtypes = [C.POINTER(np2_edits_t)]
        L.np2_edits_free.restype = None
        L.np2_depth_from_records.argtypes = [vp, u32, vp, u32, vp, C.POINTER(np2_depth_opts_t), C.POINTER(vp), C.POINTER(vp),
                                             C.POINTER(u32), vp, C.POINTER(np2_depth_stats_t)]
        L.np2_depth_from_bam.argtypes = [vp, vp, C.c_char_p, u32, C.POINTER(np2_depth_opts_t), C.POINTER(vp), C.POINTER(vp),
                                         C.POINTER(u32), vp, C.POINTER(np2_depth_stats_t)]
        vc_out = [C.POINTER(np2_varcall_opts_t), C.POINTER(vp), C.POINTER(u32), vp, vp, C.POINTER(np2_varcall_stats_t)]
        L.np2_varcall_from_records.argtypes = [vp, vp, u32, vp, u32, vp, vp] + vc_out
        L.np2_varcall_from_bam.argtypes = [vp, vp, C.c_char_p, vp, u32] + vc_out
        L.np2_varcall_host.argtypes = [vp, u32, vp, u32, vp, u64, vp, u64] + vc_out
        ac = [vp, vp, u32, vp, u64, vp, u32, vp, u64, C.POINTER(np2_asmcall_opts_t), C.POINTER(vp), C.POINTER(u32), C.POINTER(vp), C.POINTER(u32), vp,
              C.POINTER(np2_asmcall_stats_t)]
        L.np2_asmcall.argtypes = [vp] + ac
        L.np2_asmcall_host.argtypes = ac
        L.np2_ctx_set_trace.argtypes = [vp, C.c_int]
        L.np2_ctx_set_timing.argtypes = [vp, C.c_int]
        L.np2_ctx_set_timing.restype = None
        L.np2_trace_get.argtypes = [vp, C.c_int, C.c_char_p, C.POINTER(vp), C.POINTER(u64)]
        L.np2_last_timings.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
        L.np2_last_span.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.np2_last_result_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.np2_result_fetch_begin.argtypes = [vp]
        L.np2_result_fetch_end.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.np2_phase_vote.argtypes = [vp, u32, vp, vp, vp, u64, vp, vp, u32, C.c_int, vp, C.POINTER(u32)]
        L.np2_ctx_create_shared.argtypes = [C.POINTER(vp), vp]
        L.np2_batch_create.argtypes = [C.POINTER(vp), vp, C.c_int]
        L.np2_batch_destroy.argtypes = [vp]
        L.np2_batch_destroy.restype = None
        L.np2_batch_slots.argtypes = [vp]
        L.np2_batch_set_sink.argtypes = [vp, C.c_int, vp, C.c_uint64]
        L.np2_batch_slot_ctx.argtypes = [vp, C.c_int]
        L.np2_batch_slot_ctx.restype = vp
        L.np2_batch_last_error.argtypes = [vp]
        L.np2_batch_last_error.restype = C.c_char_p
        L.np2_batch_polish.argtypes = [vp, vp, C.c_int, C.POINTER(np2_opts_t), vp, vp, vp, vp, vp]
        L.np2_batch_set_timing.argtypes = [vp, C.c_int]
        L.np2_batch_set_timing.restype = None
        L.np2_batch_set_priority.argtypes = [vp, C.c_int]
        L.np2_batch_set_priority.restype = C.c_int
        L.np2_batch_last_diff_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.np2_batch_last_call_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.np2_batch_flush_log.argtypes = [vp, C.POINTER(vp)]
        L.np2_shard_plan.argtypes = [vp, u32, u32, u32, u32, C.POINTER(np2_shard_plan_t)]
        L.np2_shard_upload.argtypes = [vp, vp, u32, vp, u32, vp, u64, C.POINTER(np2_shard_plan_t), C.POINTER(vp)]
        L.np2_shard_begin.argtypes = [vp, vp, C.POINTER(np2_shard_plan_t), C.POINTER(np2_opts_t), u32, C.POINTER(vp)]
        L.np2_shard_passes_left.argtypes = [vp]
        L.np2_shard_vote.argtypes = [vp, C.POINTER(np2_vote_t)]
        L.np2_vote_decide.argtypes = [C.POINTER(np2_vote_t), C.c_int, u32, C.POINTER(np2_opts_t), vp, C.POINTER(u32)]
        L.np2_shard_apply.argtypes = [vp, vp, u32]
        L.np2_shard_final.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
        L.np2_shard_final_device.argtypes = [vp, C.POINTER(np2_shard_piece_t)]
        L.np2_shard_fetch.argtypes = [vp, vp, vp]
        L.np2_alloc_pinned.argtypes = [u64]
        L.np2_alloc_pinned.restype = vp
        L.np2_trim_device_cache.argtypes = []
        L.np2_trim_device_cache.restype = None
        L.np2_shard_end.argtypes = [vp]
        L.np2_shard_end.restype = None
        L.np2_swiss_order.argtypes = [vp, vp, u32, vp, C.POINTER(u32)]
        L.np2_debug_poison.argtypes = [C.c_int]
        L.np2_debug_poison.restype = C.c_int
        L.np2_debug_poison_stats.argtypes = [C.POINTER(u64), C.POINTER(u64)]
        L.np2_debug_poison_stats.restype = None
        L.np2_batch_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.np2_io_last_error.restype = C.c_char_p
        L.np2_rep_bytes.argtypes = [C.c_int, vp, u64, C.POINTER(np2_rep_opts_t), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64),
                                    C.POINTER(np2_rep_stats_t)]
        L.np2_rep_files.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(np2_rep_opts_t), C.c_char_p, C.c_int,
                                    C.POINTER(np2_rep_stats_t)]
        _LIB = L
    return _LIB


TRACE_DTYPES = {
    "graph.off": np.uint32, "graph.bases": np.uint16, "graph.delta": np.uint16, "graph.count": np.uint32,
    "lq.start": np.uint32, "lq.end": np.uint32, "invalid_ids": np.uint32,
    # the graph a phasing pass's vote is decided on: CSR offsets per read, rows of (neighbour, weight)
    "vote.row_off": np.uint32, "vote.rows": np.dtype([("nbr", "<u4"), ("w", "<f4")]),
}
for _t in ("cand", "seed", "hete", "rech0", "rech1", "rech2"):
    TRACE_DTYPES.update({
        f"{_t}.start": np.uint32, f"{_t}.end": np.uint32, f"{_t}.lable": np.uint8, f"{_t}.sudo_off": np.uint32,
        f"{_t}.sudo": np.uint8, f"{_t}.cand_off": np.uint32, f"{_t}.order": np.uint32, f"{_t}.kscore": np.uint16,
        f"{_t}.kmer": np.uint64, f"{_t}.seq_off": np.uint32, f"{_t}.seq": np.uint8,
    })
for _t in ("cns_raw", "cns_succ", "cns_rech0", "cns_rech1", "cns_rech2"):
    TRACE_DTYPES.update({f"{_t}.pos": np.uint32, f"{_t}.base": np.uint8})


class _Raw:
    """`n` elements at a raw address, for np.asarray (array-interface protocol: 3.5 us where np.ctypeslib.as_array on a cast
    pointer takes 33 — seventeen results per step of a batched assembly, on threads that share the interpreter lock)"""
    __slots__ = ("__array_interface__",)

    def __init__(self, addr, n, typestr):
        self.__array_interface__ = {"shape": (n,), "typestr": typestr, "data": (addr, False), "version": 3}


_TYPESTR = {C.c_uint8: "|u1", C.c_uint32: "<u4", C.c_uint64: "<u8", C.c_uint16: "<u2", C.c_int32: "<i4"}


def _owned(ptr, n, ctype):
    """Zero-copy numpy view of a callee-allocated result buffer; np2_free runs when the array is collected."""
    base = np.asarray(_Raw(ptr.value, max(n, 1), _TYPESTR[ctype]))
    weakref.finalize(base, lib().np2_free, C.c_void_p(ptr.value))
    return base[:n]


def depth_call(pol, L_, call, min_depth=3, min_len=1000, min_aligned_fra=0.8, exclude_flags=0x4, min_mapq=0, want_depth=False):
    """One np2_depth_* call: `call(opts, starts, ends, n_runs, depth, stats)` is the entry point with its leading arguments
    bound -> (kept runs as an (n, 2) uint32 array of inclusive (s, e), stats dict, per-base uint32 depth or None)."""
    o = np2_depth_opts_t(min_depth, min_len, min_aligned_fra, exclude_flags, min_mapq)
    ps, pe, n, st = C.c_void_p(), C.c_void_p(), C.c_uint32(), np2_depth_stats_t()
    depth = np.zeros(max(int(L_), 1), dtype=np.uint32) if want_depth else None
    try:
        pol._check(call(C.byref(o), C.byref(ps), C.byref(pe), C.byref(n), depth.ctypes.data if want_depth else None, C.byref(st)))
        runs = np.zeros((n.value, 2), dtype=np.uint32)
        if n.value:
            runs[:, 0] = np.asarray(_Raw(ps.value, n.value, "<u4"))
            runs[:, 1] = np.asarray(_Raw(pe.value, n.value, "<u4"))
    finally:
        if ps.value:
            lib().np2_free(ps)
        if pe.value:
            lib().np2_free(pe)
    stats = {f: getattr(st, f) for f, _ in np2_depth_stats_t._fields_}
    return runs, stats, (depth[:int(L_)] if want_depth else None)


def depth_from_records(pol, L_, recs, cigar, **kw):
    """np2_depth_from_records: mapping depth of a contig of `L_` positions from alignment records (`recs`: np2_bamrec_t as
    io.BAMREC_DTYPE, `cigar`: the BAM CIGAR words their cigar_off index) and its runs of depth >= min_depth that are at
    least min_len long.  Keywords: min_depth=3, min_len=1000, min_aligned_fra=0.8, exclude_flags=0x4, min_mapq=0,
    want_depth=False.  See depth_call for what comes back."""
    recs = np.ascontiguousarray(recs)
    if recs.ndim != 1 or (len(recs) and recs.dtype.itemsize != 40):
        raise ValueError("recs must be a one-dimensional array of np2_bamrec_t (io.BAMREC_DTYPE)")
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    L = lib()
    return depth_call(pol, L_, lambda *a: L.np2_depth_from_records(pol._h, int(L_), recs.ctypes.data if len(recs) else None, len(recs),
                                                                   cigar.ctypes.data if len(cigar) else None, *a), **kw)


def varcall_call(check, L_, call, min_depth=8, min_alt=3, hom_pm=800, het_pm=250, max_indel=28, min_aligned_fra=0.0, exclude_flags=0xF04,
                 min_mapq=5, want_counts=False):
    """One np2_varcall_* call: `call(opts, calls, n_calls, cov, alt, stats)` is the entry point with its leading arguments
    bound, `check` raises on its status -> (calls as a VARCALL_DTYPE array, stats dict — the six call totals under the names
    of VARCALL_CALLS —, cov as uint32 [L] or None, alt as uint32 [L, 4] or None)."""
    o = np2_varcall_opts_t(min_aligned_fra, min_depth, min_alt, hom_pm, het_pm, max_indel, exclude_flags, min_mapq)
    pc, n, st = C.c_void_p(), C.c_uint32(), np2_varcall_stats_t()
    n_pos = int(L_)
    cov = np.zeros(max(n_pos, 1), dtype=np.uint32) if want_counts else None
    alt = np.zeros((max(n_pos, 1), 4), dtype=np.uint32) if want_counts else None
    try:
        check(call(C.byref(o), C.byref(pc), C.byref(n), cov.ctypes.data if want_counts else None, alt.ctypes.data if want_counts else None,
                   C.byref(st)))
        calls = np.frombuffer(C.string_at(pc.value, n.value * VARCALL_DTYPE.itemsize), dtype=VARCALL_DTYPE) if n.value else np.zeros(0, VARCALL_DTYPE)
    finally:
        if pc.value:
            lib().np2_free(pc)
    stats = {f: getattr(st, f) for f, _ in np2_varcall_stats_t._fields_ if f not in ("calls", "stage_ms", "pad")}
    stats.update({k: int(st.calls[i]) for i, k in enumerate(VARCALL_CALLS)})
    stats["stage_ms"] = {k: float(st.stage_ms[i]) for i, k in enumerate(VARCALL_STAGES)}
    return calls, stats, (cov[:n_pos] if want_counts else None), (alt[:n_pos] if want_counts else None)


def _varcall_arrays(ref, recs, cigar, seq4):
    ref = np.frombuffer(bytes(ref), dtype=np.uint8) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, dtype=np.uint8)
    recs = np.ascontiguousarray(recs)
    if recs.ndim != 1 or (len(recs) and recs.dtype.itemsize != 40):
        raise ValueError("recs must be a one-dimensional array of np2_bamrec_t (io.BAMREC_DTYPE)")
    return ref, recs, np.ascontiguousarray(cigar, dtype=np.uint32), np.ascontiguousarray(seq4, dtype=np.uint8)


def _ptr(a):
    return a.ctypes.data if len(a) else None


def varcall_from_records(pol, ref, recs, cigar, seq4, **kw):
    """np2_varcall_from_records: the read-supported variants of the contig `ref` (bytes or uint8 array) from alignment records
    (`recs`: np2_bamrec_t as io.BAMREC_DTYPE, `cigar`: the BAM CIGAR words, `seq4`: the BAM 4-bit SEQ bytes) on the device of
    Polisher `pol`.  Keywords: min_depth=8, min_alt=3, hom_pm=800, het_pm=250, max_indel=28, min_aligned_fra=0.0,
    exclude_flags=0xF04, min_mapq=5, want_counts=False.  The rule is include/np2_io.h's; see varcall_call for what comes back."""
    ref, recs, cigar, seq4 = _varcall_arrays(ref, recs, cigar, seq4)
    L = lib()
    return varcall_call(pol._check, len(ref), lambda *a: L.np2_varcall_from_records(pol._h, _ptr(ref), len(ref), _ptr(recs), len(recs), _ptr(cigar),
                                                                                      _ptr(seq4), *a), **kw)


def varcall_from_bam(pol, bam, name, ref, **kw):
    """np2_varcall_from_bam: the same over the records of contig `name` of the indexed BAM `bam` (io.Bam), read the way
    io.contig_from_bam reads them (on the device with NP2_INFLATE=gpu, else by the host pool)."""
    ref = _varcall_arrays(ref, np.zeros(0, dtype=[("x", "u1", 40)]), [], [])[0]
    L = lib()
    return varcall_call(pol._check, len(ref), lambda *a: L.np2_varcall_from_bam(pol._h, bam._h, name.encode(), _ptr(ref), len(ref), *a), **kw)


def varcall_host(ref, recs, cigar, seq4, **kw):
    """np2_varcall_host: the host twin of varcall_from_records — the same rule on one CPU thread, no device."""
    ref, recs, cigar, seq4 = _varcall_arrays(ref, recs, cigar, seq4)
    L = lib()

    def check(rc):
        if rc != 0:
            raise Np2Error(rc, (L.np2_io_last_error() or b"").decode())
    return varcall_call(check, len(ref), lambda *a: L.np2_varcall_host(_ptr(ref), len(ref), _ptr(recs), len(recs), _ptr(cigar), len(cigar),
                                                                       _ptr(seq4), len(seq4), *a), **kw)


def _asmcall(check, call, refs, query, alns, cigar, min_mapq=5, min_aln=5000, want_cov=False):
    """One np2_asmcall* call: `call(*arguments)` is the entry point with its context bound, `check` raises on its status.
    refs: a list of reference sequences (bytes); query: the query stream (bytes or uint8 array); alns: an ASMALN_DTYPE array;
    cigar: BAM CIGAR words -> (runs as an ASMRUN_DTYPE array, vars as an ASMVAR_DTYPE array, stats dict, cov as uint32 over the
    concatenated references or None)."""
    refs = [bytes(r) for r in refs]
    ref_off = np.zeros(len(refs) + 1, dtype=np.uint64)
    ref_off[1:] = np.cumsum([len(r) for r in refs], dtype=np.uint64)
    cat = np.frombuffer(b"".join(refs), dtype=np.uint8)
    query = np.frombuffer(bytes(query), dtype=np.uint8) if isinstance(query, (bytes, bytearray, memoryview)) else np.ascontiguousarray(query, dtype=np.uint8)
    alns = np.ascontiguousarray(alns)
    if alns.ndim != 1 or (len(alns) and alns.dtype.itemsize != ASMALN_DTYPE.itemsize):
        raise ValueError("alns must be a one-dimensional array of np2_asmaln_t (api.ASMALN_DTYPE)")
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    o, st = np2_asmcall_opts_t(min_mapq, min_aln), np2_asmcall_stats_t()
    pr, pv, nr, nv = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
    cov = np.zeros(max(len(cat), 1), dtype=np.uint32) if want_cov else None
    try:
        check(call(_ptr(cat), ref_off.ctypes.data, len(refs), _ptr(query), len(query), _ptr(alns), len(alns), _ptr(cigar), len(cigar), C.byref(o),
                   C.byref(pr), C.byref(nr), C.byref(pv), C.byref(nv), cov.ctypes.data if want_cov else None, C.byref(st)))
        runs = np.frombuffer(C.string_at(pr.value, nr.value * ASMRUN_DTYPE.itemsize), dtype=ASMRUN_DTYPE) if nr.value else np.zeros(0, ASMRUN_DTYPE)
        vars_ = np.frombuffer(C.string_at(pv.value, nv.value * ASMVAR_DTYPE.itemsize), dtype=ASMVAR_DTYPE) if nv.value else np.zeros(0, ASMVAR_DTYPE)
    finally:
        for p in (pr, pv):
            if p.value:
                lib().np2_free(p)
    stats = {f: getattr(st, f) for f, _ in np2_asmcall_stats_t._fields_ if f not in ("found", "kept", "stage_ms")}
    for i, k in enumerate(ASMCALL_KINDS):
        stats["found_" + k.lower()], stats["kept_" + k.lower()] = int(st.found[i]), int(st.kept[i])
    stats["stage_ms"] = {k: float(st.stage_ms[i]) for i, k in enumerate(ASMCALL_STAGES)}
    return runs, vars_, stats, (cov[:len(cat)] if want_cov else None)


def asmcall(pol, refs, query, alns, cigar, **kw):
    """np2_asmcall: an assembly's differences from references, from the alignments of its segments, on the device of Polisher
    `pol`: the runs covered exactly once and the SNV / DEL / INS events inside them.  Keywords: min_mapq=5, min_aln=5000,
    want_cov=False.  The rule is include/np2_io.h's (this project's own); see _asmcall for the arguments and what comes back."""
    L = lib()
    return _asmcall(pol._check, lambda *a: L.np2_asmcall(pol._h, *a), refs, query, alns, cigar, **kw)


def asmcall_host(refs, query, alns, cigar, **kw):
    """np2_asmcall_host: the host twin of asmcall — the same rule on one CPU thread, no device."""
    L = lib()

    def check(rc):
        if rc != 0:
            raise Np2Error(rc, (L.np2_io_last_error() or b"").decode())
    return _asmcall(check, lambda *a: L.np2_asmcall_host(*a), refs, query, alns, cigar, **kw)


def _pack_seqs(seqs, to_bytes=True):
    """what the *_strings entry points take: (the sequences, as bytes each unless told otherwise; their n + 1 offsets; the
    bytes themselves, one after the other, with a byte of room behind)"""
    if to_bytes:
        seqs = [bytes(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs])
    return seqs, off, np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)


def _split_bits(raw, nb):
    """the per-sequence bitmaps of `raw`, sequence i's being its next nb[i] bytes (views)"""
    cuts = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    return [raw[cuts[i]:cuts[i + 1]] for i in range(len(nb))]


class QvStats:
    """What np2_qv_strings / np2_qv_device return.  stats: uint64 array (n, 2) of (n_kmers, n_absent) per sequence;
    hist: uint64[1024] (hist[c] = k-mers with count c) or None; bits: one uint8 array per sequence (ceil(len / 8) bytes,
    least significant bit first, bit e = the k-mer ending at base e is valid and absent) or None; kernel_ms: HIP-event time
    of the scan kernel alone."""
    __slots__ = ("stats", "hist", "bits", "kernel_ms")

    def __init__(self, stats, hist, bits, kernel_ms):
        self.stats, self.hist, self.bits, self.kernel_ms = stats, hist, bits, kernel_ms

    @property
    def n_kmers(self):
        return int(self.stats[:, 0].sum())

    @property
    def n_absent(self):
        return int(self.stats[:, 1].sum())


class TrioStats:
    """What np2_trio_strings / np2_trio_device return.  stats: uint64 array (n, 7) per sequence of (n_kmers, n_pat, n_mat,
    pp, pm, mp, mm): k-mers, paternal and maternal markers, consecutive marker pairs as (earlier, later); pat_bits /
    mat_bits: one uint8 array per sequence (ceil(len / 8) bytes, least significant bit first, bit e = the k-mer ending at
    base e is that parent's marker) or None; kernel_ms: HIP-event time of the two kernels."""
    __slots__ = ("stats", "pat_bits", "mat_bits", "kernel_ms")

    def __init__(self, stats, pat_bits, mat_bits, kernel_ms):
        self.stats, self.pat_bits, self.mat_bits, self.kernel_ms = stats, pat_bits, mat_bits, kernel_ms

    @property
    def total(self):
        """the seven counters summed over the sequences"""
        return tuple(int(x) for x in self.stats.sum(axis=0, dtype=np.uint64)) if len(self.stats) else (0,) * 7

    @property
    def n_switch(self):
        return self.total[4] + self.total[5]


class BinResult:
    """What np2_bin_stream returns.  classes: bytes, one of b"pma0" per read; stats: uint32 array (n, 7) per read of
    (n_kmers, n_pat, n_mat, pp, pm, mp, mm) or None; kernel_ms: HIP-event time of the kernels."""
    __slots__ = ("classes", "stats", "kernel_ms")

    def __init__(self, classes, stats, kernel_ms):
        self.classes, self.stats, self.kernel_ms = classes, stats, kernel_ms


class CmpStats:
    """What np2_cmp_strings returns.  stats: (n_read, n_found, n_asm, n_asm_only), distinct k-mers: reliable read k-mers,
    those of them the assembly set holds, the set's k-mers, those of them the reads do not have; spectra: uint64 array
    (6, 1024), spectra[min(cn, 5), c] = reliable read k-mers with stored count c and copy number cn in the set, or None;
    asm_only: uint64[6], the n_asm_only k-mers by min(cn, 5); kernel_ms: HIP-event time of the two join kernels."""
    __slots__ = ("stats", "spectra", "asm_only", "kernel_ms")

    def __init__(self, stats, spectra, asm_only, kernel_ms):
        self.stats, self.spectra, self.asm_only, self.kernel_ms = stats, spectra, asm_only, kernel_ms

    n_read = property(lambda self: self.stats[0])
    n_found = property(lambda self: self.stats[1])
    n_asm = property(lambda self: self.stats[2])
    n_asm_only = property(lambda self: self.stats[3])

    @property
    def completeness(self):
        return self.stats[1] / self.stats[0] if self.stats[0] else float("nan")


class Edits:
    """What np2_edits_buffers / np2_edits_last return, copied out of the library's blocks.  edits: EDIT_DTYPE records after
    the shift, unanchored, ascending ref_pos; ref(i) / alt(i): edit i's strings (bytes); support: uint32 array
    (n_edits, n_tables, 4) of (n_in, absent_in, n_out, absent_out); table_idx / table_k: the tables judged by; totals: dict
    (has_span, first, last, raw_runs, same_runs, n_kind[5], bases_inserted, bases_deleted, outside); kernel_ms: HIP-event
    time per stage (EDIT_STAGES)."""

    def __init__(self, r: np2_edits_t):
        n, nt = r.n_edits, r.n_tables

        def take(addr, count, typestr):
            return np.array(np.asarray(_Raw(addr, count, typestr)), copy=True) if count else np.zeros(0, dtype=np.dtype(typestr))
        self.edits = take(r.edits, n * 5, "<u4").view(EDIT_DTYPE) if n else np.zeros(0, dtype=EDIT_DTYPE)
        self.ref_off, self.alt_off = take(r.ref_off, n + 1, "<u4"), take(r.alt_off, n + 1, "<u4")
        self.ref_pool = take(r.ref_pool, int(self.ref_off[-1]), "|u1").tobytes()
        self.alt_pool = take(r.alt_pool, int(self.alt_off[-1]), "|u1").tobytes()
        self.support = take(r.support, n * nt * 4, "<u4").reshape(n, nt, 4)
        self.table_idx, self.table_k = [int(r.table_idx[i]) for i in range(nt)], [int(r.table_k[i]) for i in range(nt)]
        self.totals = dict(has_span=int(r.has_span), first=int(r.first_pos), last=int(r.last_pos), raw_runs=int(r.raw_runs),
                           same_runs=int(r.same_runs), n_kind=[int(x) for x in r.n_kind], bases_inserted=int(r.bases_inserted),
                           bases_deleted=int(r.bases_deleted), outside=int(r.outside_span))
        self.kernel_ms = {s: float(r.kernel_ms[i]) for i, s in enumerate(EDIT_STAGES)}

    def __len__(self):
        return len(self.edits)

    def ref(self, i):
        return self.ref_pool[int(self.ref_off[i]):int(self.ref_off[i + 1])]

    def alt(self, i):
        return self.alt_pool[int(self.alt_off[i]):int(self.alt_off[i + 1])]

    def records(self):
        """the edits as the dicts tests/edits_model.py writes: ref_pos, out_off, ref, alt, kind"""
        return [dict(ref_pos=int(e["ref_pos"]), out_off=int(e["out_off"]), ref=self.ref(i), alt=self.alt(i), kind=EDIT_KINDS[int(e["kind"])])
                for i, e in enumerate(self.edits)]


class ResidentContig:
    """A contig's packed pileup resident in HBM (np2_contig_t)."""

    def __init__(self, polisher, handle, pileup):
        self._p = polisher
        self._h = handle
        self.L = pileup.L
        self.n_reads = pileup.n_reads
        self.n_columns = pileup.n_columns()
        self.name = pileup.name

    def free(self):
        if self._h:
            lib().np2_contig_free(self._p._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Polisher:
    """One np2 context == one HIP device + HBM-resident yak tables.

    Mirrors the reference's per-worker state (one Opt clone with its KmerInfo per worker thread,
    src/main.rs:1724): contexts are independent, calls on one context are serialized."""

    def __init__(self, yaks, device=0):
        self._yaks = list(yaks)
        arr = yaks_array(self._yaks)
        h = C.c_void_p()
        rc = lib().np2_ctx_create(C.byref(h), device, arr, len(self._yaks))
        if rc != 0:
            raise Np2Error(rc, "np2_ctx_create failed (see stderr)")
        self._h = h
        self.device = device

    def clone(self):
        """np2_ctx_create_shared: a further context on the same device over the SAME HBM k-mer tables."""
        p = Polisher.__new__(Polisher)
        p._yaks = self._yaks
        p._parent = self
        p.device = self.device
        h = C.c_void_p()
        rc = lib().np2_ctx_create_shared(C.byref(h), self._h)
        if rc != 0:
            raise Np2Error(rc, "np2_ctx_create_shared failed (see stderr)")
        p._h = h
        return p

    def close(self):
        if getattr(self, "_h", None):
            lib().np2_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise Np2Error(rc, lib().np2_last_error(self._h).decode())

    def set_trace(self, on=True):
        lib().np2_ctx_set_trace(self._h, 1 if on else 0)

    def set_timing(self, on=True):
        """Arm every per-stage HIP-event timer (default: only the dense pass is timed)."""
        lib().np2_ctx_set_timing(self._h, 1 if on else 0)

    def upload(self, pileup: Pileup) -> ResidentContig:
        h = C.c_void_p()
        self._check(lib().np2_contig_upload(self._h, pileup.ref.ctypes.data, pileup.L, pileup.reads.ctypes.data,
                                            pileup.n_reads, pileup.nibbles.ctypes.data, pileup.nibbles.shape[0],
                                            C.byref(h)))
        return ResidentContig(self, h, pileup)

    def polish_resident(self, contig: ResidentContig, opts: Opts = None, want_pos=True, defer_output=False):
        """np2_polish_resident.  want_pos=False returns (bases, (first_pos, last_pos)) — all a FASTA record needs.
        defer_output=True leaves the sequence on the device and returns (None, span): fetch it with fetch_begin() /
        fetch_end() so that its host copy overlaps the next contig."""
        o = (opts or Opts()).c()
        ob, op, on = C.c_void_p(), C.c_void_p(), C.c_uint64()
        if defer_output:
            self._check(lib().np2_polish_resident(self._h, contig._h, C.byref(o), None, None, C.byref(on)))
            return None, self.last_span()
        self._check(lib().np2_polish_resident(self._h, contig._h, C.byref(o), C.byref(ob),
                                              C.byref(op) if want_pos else None, C.byref(on)))
        n = on.value
        if want_pos:
            return _owned(ob, n, C.c_uint8), _owned(op, n, C.c_uint32)
        return _owned(ob, n, C.c_uint8), self.last_span()

    def last_span(self):
        a, b = C.c_uint32(), C.c_uint32()
        self._check(lib().np2_last_span(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def fetch_begin(self):
        """np2_result_fetch_begin: start the host copy of the last (deferred) result on the output stream."""
        self._check(lib().np2_result_fetch_begin(self._h))

    def fetch_end(self):
        """np2_result_fetch_end: wait for the copy; zero-copy view of the context's pinned buffer (valid until the
        second-next fetch_begin)."""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(lib().np2_result_fetch_end(self._h, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(n.value, 1),))[: n.value]

    def last_result_device(self):
        """(device address, length) of the last polished sequence in HBM; valid until the next call on this context."""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(lib().np2_last_result_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def polish(self, pileup: Pileup, opts: Opts = None):
        c = self.upload(pileup)
        try:
            return self.polish_resident(c, opts)
        finally:
            c.free()

    def trace(self, pass_idx, name):
        d, n = C.c_void_p(), C.c_uint64()
        if lib().np2_trace_get(self._h, pass_idx, name.encode(), C.byref(d), C.byref(n)) != 0:
            return None
        dt = np.dtype(TRACE_DTYPES[name])
        if n.value == 0:
            return np.zeros(0, dtype=dt)
        buf = (C.c_uint8 * n.value).from_address(d.value)
        return np.frombuffer(bytes(buf), dtype=dt)

    def timings(self):
        names, ms, n = C.c_void_p(), C.c_void_p(), C.c_int()
        lib().np2_last_timings(self._h, C.byref(names), C.byref(ms), C.byref(n))
        out = {}
        if n.value:
            vals = np.ctypeslib.as_array(C.cast(ms, C.POINTER(C.c_float)), shape=(n.value,))
            addr = names.value
            for i in range(n.value):  # NUL-separated names: walk them one C string at a time
                nm = C.string_at(addr)
                addr += len(nm) + 1
                out[nm.decode()] = float(vals[i])
        return out

    def score_strings(self, yak_idx, strings, min_kmer_count=5):
        strings, off, blob = _pack_seqs(strings, to_bytes=False)
        out = np.zeros(len(strings), dtype=np.uint16)
        self._check(lib().np2_score_strings(self._h, yak_idx, blob.ctypes.data, off.ctypes.data, len(strings),
                                            min_kmer_count, out.ctypes.data))
        return out

    def lookup_hashes(self, yak_idx, hashes, min_kmer_count=5):
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        out = np.zeros(h.shape[0], dtype=np.uint16)
        self._check(lib().np2_lookup_hashes(self._h, yak_idx, h.ctypes.data, h.shape[0], min_kmer_count,
                                            out.ctypes.data))
        return out

    def qv_strings(self, yak_idx, seqs, min_count=1, hist=False, bits=False):
        """np2_qv_strings: k-mers and absent k-mers of every sequence of `seqs` (bytes-like each) against table `yak_idx`
        -> QvStats.  count(k-mer) is the stored count if >= min_count, else 0; absent means count == 0."""
        seqs, off, blob = _pack_seqs(seqs)
        n = len(seqs)
        stats = np.zeros((max(n, 1), 2), dtype=np.uint64)
        h = np.zeros(1024, dtype=np.uint64) if hist else None
        nb = [(len(s) + 7) // 8 for s in seqs]
        raw = np.zeros(sum(nb) + 1, dtype=np.uint8) if bits else None
        ms = C.c_float()
        self._check(lib().np2_qv_strings(self._h, yak_idx, blob.ctypes.data, off.ctypes.data, n, min_count, stats.ctypes.data,
                                         h.ctypes.data if hist else None, raw.ctypes.data if bits else None, C.byref(ms)))
        return QvStats(stats[:n], h, _split_bits(raw, nb) if bits else None, ms.value)

    def qv_device(self, yak_idx, dev_ptr, n, min_count=1, hist=False, bits=False):
        """np2_qv_device: the same measurement of ONE sequence of `n` bytes at device address `dev_ptr` on this context's
        device (last_result_device()) -> QvStats with one row."""
        stats = np.zeros((1, 2), dtype=np.uint64)
        h = np.zeros(1024, dtype=np.uint64) if hist else None
        raw = np.zeros((int(n) + 7) // 8 + 1, dtype=np.uint8) if bits else None
        ms = C.c_float()
        self._check(lib().np2_qv_device(self._h, yak_idx, C.c_void_p(dev_ptr) if dev_ptr else None, int(n), min_count,
                                        stats.ctypes.data, h.ctypes.data if hist else None, raw.ctypes.data if bits else None,
                                        C.byref(ms)))
        return QvStats(stats, h, [raw[:(int(n) + 7) // 8]] if bits else None, ms.value)

    def _edits(self, call, min_count, tables):
        o, r = np2_edits_opts_t(int(min_count), int(tables)), np2_edits_t()
        self._check(call(C.byref(o), C.byref(r)))
        try:
            return Edits(r)
        finally:
            lib().np2_edits_free(C.byref(r))

    def edits_buffers(self, ref, bases, pos, min_count=1, tables=-1):
        """np2_edits_buffers: where the output (`bases` with their contig positions `pos`, this project's or the reference
        binary's --out_pos alike) differs from the contig `ref` -> Edits.  tables: bit mask of this context's k-mer tables
        to judge every edit by, -1 all, 0 none.  Np2Error(NP2_E_ARG) for positions that decrease or are not below len(ref)."""
        ref = np.frombuffer(bytes(ref), dtype=np.uint8) if not isinstance(ref, np.ndarray) else np.ascontiguousarray(ref, dtype=np.uint8)
        bases = np.frombuffer(bytes(bases), dtype=np.uint8) if not isinstance(bases, np.ndarray) else np.ascontiguousarray(bases, dtype=np.uint8)
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        if len(bases) != len(pos):
            raise ValueError("bases and pos differ in length")
        L = lib()
        return self._edits(lambda o, r: L.np2_edits_buffers(self._h, ref.ctypes.data if len(ref) else None, len(ref),
                                                            bases.ctypes.data if len(bases) else None,
                                                            pos.ctypes.data if len(pos) else None, len(bases), o, r), min_count, tables)

    def edits_last(self, contig, min_count=1, tables=-1):
        """np2_edits_last: the same for the consensus the last polish_resident of this context left on the device, against
        `contig` (the ResidentContig it polished) as uploaded; nothing is copied up."""
        L = lib()
        return self._edits(lambda o, r: L.np2_edits_last(self._h, contig._h, o, r), min_count, tables)

    def cmp_strings(self, yak_idx, seqs, min_count=2, spectra=False):
        """np2_cmp_strings: k-mer completeness of the set `seqs` (bytes-like each, taken together) against the reads' table
        `yak_idx` -> CmpStats.  A read k-mer is reliable when its stored count is >= max(min_count, 1)."""
        seqs, off, blob = _pack_seqs(seqs)
        n = len(seqs)
        st = np.zeros(4, dtype=np.uint64)
        sp = np.zeros((6, 1024), dtype=np.uint64) if spectra else None
        ao = np.zeros(6, dtype=np.uint64)
        ms = C.c_float()
        self._check(lib().np2_cmp_strings(self._h, yak_idx, blob.ctypes.data, off.ctypes.data, n, min_count, st.ctypes.data,
                                          sp.ctypes.data if spectra else None, ao.ctypes.data, C.byref(ms)))
        return CmpStats(tuple(int(x) for x in st), sp, ao, ms.value)

    def trio_strings(self, pat_idx, mat_idx, seqs, min_count=2, mid_count=5, bits=False):
        """np2_trio_strings: parental markers and consecutive marker pairs of every sequence of `seqs` (bytes-like each)
        against the paternal table `pat_idx` and the maternal table `mat_idx` of the same k -> TrioStats.  A k-mer is a
        parent's marker when that parent's count is >= mid_count and the other's is < min_count."""
        seqs, off, blob = _pack_seqs(seqs)
        n = len(seqs)
        stats = np.zeros((max(n, 1), 7), dtype=np.uint64)
        nb = [(len(s) + 7) // 8 for s in seqs]
        raw = [np.zeros(sum(nb) + 1, dtype=np.uint8) for _ in range(2)] if bits else None
        ms = C.c_float()
        self._check(lib().np2_trio_strings(self._h, pat_idx, mat_idx, blob.ctypes.data, off.ctypes.data, n, min_count, mid_count,
                                           stats.ctypes.data, raw[0].ctypes.data if bits else None,
                                           raw[1].ctypes.data if bits else None, C.byref(ms)))
        per = [_split_bits(r, nb) for r in raw] if bits else [None, None]
        return TrioStats(stats[:n], per[0], per[1], ms.value)

    def trio_device(self, pat_idx, mat_idx, dev_ptr, n, min_count=2, mid_count=5, bits=False):
        """np2_trio_device: the same measurement of ONE sequence of `n` bytes at device address `dev_ptr` on this
        context's device (last_result_device()) -> TrioStats with one row."""
        stats = np.zeros((1, 7), dtype=np.uint64)
        nb = (int(n) + 7) // 8
        raw = [np.zeros(nb + 1, dtype=np.uint8) for _ in range(2)] if bits else None
        ms = C.c_float()
        self._check(lib().np2_trio_device(self._h, pat_idx, mat_idx, C.c_void_p(dev_ptr) if dev_ptr else None, int(n), min_count,
                                          mid_count, stats.ctypes.data, raw[0].ctypes.data if bits else None,
                                          raw[1].ctypes.data if bits else None, C.byref(ms)))
        return TrioStats(stats, [raw[0][:nb]] if bits else None, [raw[1][:nb]] if bits else None, ms.value)

    def bin_stream(self, pat_idx, mat_idx, reads_or_stream, min_count=2, mid_count=5, min_score=2, minor_permille=330, stats=False):
        """np2_bin_stream: the class of every read (b"p", b"m", b"a", b"0") against the paternal table `pat_idx` and the
        maternal table `mat_idx` of the same k -> BinResult.  `reads_or_stream`: a list of reads (bytes-like each, none
        holding a newline) or ONE bytes object holding a packed separator stream (every read followed by a newline)."""
        if isinstance(reads_or_stream, (bytes, bytearray, memoryview)):
            stream = bytes(reads_or_stream)
        else:
            reads = [bytes(r) for r in reads_or_stream]
            if any(b"\n" in r for r in reads):
                raise ValueError("a read holds a newline")
            stream = b"".join(r + b"\n" for r in reads)
        n = stream.count(b"\n")
        blob = np.frombuffer(stream + b"\0", dtype=np.uint8)
        cls = np.zeros(n + 1, dtype=np.uint8)
        st = np.zeros(n + 1, dtype=BIN_DTYPE) if stats else None
        o = np2_bin_opts_t(min_count, mid_count, min_score, minor_permille)
        ms = C.c_float()
        self._check(lib().np2_bin_stream(self._h, pat_idx, mat_idx, blob.ctypes.data if len(stream) else None, len(stream), n, C.byref(o),
                                         cls.ctypes.data, st.ctypes.data if stats else None, C.byref(ms)))
        table = None
        if stats:
            table = np.concatenate([st["n_kmers"][:n, None], st["n_pat"][:n, None], st["n_mat"][:n, None], st["pairs"][:n]], axis=1)
        return BinResult(cls[:n].tobytes(), table, ms.value)


class BatchPolisher:
    """np2_batch_t: up to `n_slots` contigs polished at once with one launch per pipeline step for all of them.

    Mirrors the reference's pool of worker threads (src/main.rs:1717-1843); results per contig are exactly those of
    Polisher.polish_resident."""

    def __init__(self, polisher: Polisher, n_slots):
        self._pol = polisher  # keeps the parent context (and its yak tables) alive
        h = C.c_void_p()
        rc = lib().np2_batch_create(C.byref(h), polisher._h, n_slots)
        if rc != 0:
            raise Np2Error(rc, lib().np2_last_error(polisher._h).decode())
        self._h = h
        self.n_slots = n_slots

    def close(self):
        if getattr(self, "_h", None):
            lib().np2_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_priority(self, high):
        """np2_batch_set_priority: stream priority of this batch (alternate it over the batches of one device)."""
        rc = lib().np2_batch_set_priority(self._h, 1 if high else 0)
        if rc != 0:
            raise Np2Error(rc, "np2_batch_set_priority failed")

    def set_timing(self, on=True):
        lib().np2_batch_set_timing(self._h, 1 if on else 0)

    def last_diff_ms(self):
        ms, n = C.c_float(), C.c_int()
        lib().np2_batch_last_diff_ms(self._h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def last_call_ms_inside(self):
        """(wall ms of the last np2_batch_polish measured inside the call, ms of it after its last flush)"""
        a, t = C.c_double(), C.c_double()
        lib().np2_batch_last_call_ms(self._h, C.byref(a), C.byref(t))
        return a.value, t.value

    def flush_log(self):
        """[(host ms, issue ms, device-wait ms)] per flush of the last polish call."""
        p = C.c_void_p()
        n = lib().np2_batch_flush_log(self._h, C.byref(p))
        if not n:
            return []
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(3 * n,)).copy()
        return [tuple(round(float(x), 3) for x in a[3 * i:3 * i + 3]) for i in range(n)]

    def flush_total_ms(self):
        """host + issue + wait over the flushes of the last polish call (one number: cheap enough for a timed loop)"""
        p = C.c_void_p()
        n = lib().np2_batch_flush_log(self._h, C.byref(p))
        return float(sum((C.c_double * (3 * n)).from_address(p.value))) if n else 0.0

    def stats(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib().np2_batch_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return {"launches": a.value, "commands": b.value, "flushes": c.value}

    def polish(self, contigs, opts: Opts = None, want_pos=False, keep_on_device=False):
        """[(bases, pos-or-span)] per contig, like Polisher.polish_resident(want_pos=...).  keep_on_device=True returns
        [(None, span)]: fetch the sequences of the last wave from the slot contexts (slot_fetch_begin / _end)."""
        n = len(contigs)
        o = (opts or Opts()).c()
        hs = (C.c_void_p * n)(*[c._h for c in contigs])
        key = (n, want_pos, keep_on_device)
        if getattr(self, "_arrs_key", None) != key:  # (the argument arrays of the last call shape are kept)
            self._arrs = ((C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_uint64 * n)(), (C.c_int * n)(), (C.c_uint32 * (2 * n))())
            self._arrs_key = key
        ob, op, on, rcs, span = self._arrs
        import time as _t
        _t0 = _t.perf_counter()
        rc = lib().np2_batch_polish(self._h, hs, n, C.byref(o), None if keep_on_device else ob,
                                    op if (want_pos and not keep_on_device) else None, on, span, rcs)
        self.last_call_ms = (_t.perf_counter() - _t0) * 1e3  # the C call alone (bench.py reports it next to the step time)
        if rc != 0:
            raise Np2Error(rc, lib().np2_batch_last_error(self._h).decode())
        out = []
        for i in range(n):
            if keep_on_device:
                out.append((None, (span[2 * i], span[2 * i + 1])))
                continue
            b = _owned(C.c_void_p(ob[i]), on[i], C.c_uint8)
            if want_pos:
                out.append((b, _owned(C.c_void_p(op[i]), on[i], C.c_uint32)))
            else:
                out.append((b, (span[2 * i], span[2 * i + 1])))
        return out

    def set_sink(self, slot, device_ptr, cap):
        """np2_batch_set_sink: the polished bases of the contig on `slot` are also copied to device address `device_ptr`."""
        rc = lib().np2_batch_set_sink(self._h, slot, C.c_void_p(device_ptr) if device_ptr else None, int(cap))
        if rc != 0:
            raise Np2Error(rc, "np2_batch_set_sink")

    def slot_fetch_begin(self, slot):
        rc = lib().np2_result_fetch_begin(lib().np2_batch_slot_ctx(self._h, slot))
        if rc != 0:
            raise Np2Error(rc, "np2_result_fetch_begin")

    def slot_fetch_end(self, slot):
        p, n = C.c_void_p(), C.c_uint64()
        rc = lib().np2_result_fetch_end(lib().np2_batch_slot_ctx(self._h, slot), C.byref(p), C.byref(n))
        if rc != 0:
            raise Np2Error(rc, "np2_result_fetch_end")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(n.value, 1),))[: n.value]


# ---- shards of one contig (include/np2.h np2_shard_*) -------------------------------------------------------------------
def shard_plan(pileup: Pileup, n_shards, halo=65536):
    """np2_shard_plan: cut a contig into n_shards reference intervals -> [np2_shard_plan_t]."""
    plans = (np2_shard_plan_t * n_shards)()
    rc = lib().np2_shard_plan(pileup.reads.ctypes.data, pileup.n_reads, pileup.L, n_shards, halo, plans)
    if rc != 0:
        raise Np2Error(rc, "np2_shard_plan: contig too short for that many shards?")
    return [plans[i] for i in range(n_shards)]


class Vote:
    """Host copy of one shard's np2_vote_t (numpy arrays), serialisable for the exchange between ranks."""

    FIELDS = (("pair_key", np.uint64), ("pair_cnt", np.uint32), ("read_id", np.uint32), ("first_pos", np.uint32),
              ("ref_w", np.int32), ("flags", np.uint8))

    def __init__(self, **arrays):
        for name, dt in self.FIELDS:
            setattr(self, name, np.ascontiguousarray(arrays.get(name, np.zeros(0, dtype=dt)), dtype=dt))

    @classmethod
    def from_c(cls, v: np2_vote_t, copy=True):
        """copy=False: views of the run's arrays (borrowed until the run's next call: a chromosome's pair list is hundreds
        of MB — packed or decided right away, it need not be copied first)."""
        def arr(ptr, n, dt):
            if not n:
                return np.zeros(0, dtype=dt)
            a = np.frombuffer((C.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt)
            return a.copy() if copy else a
        return cls(pair_key=arr(v.pair_key, v.n_pairs, np.uint64), pair_cnt=arr(v.pair_cnt, v.n_pairs, np.uint32),
                   read_id=arr(v.read_id, v.n_reads, np.uint32), first_pos=arr(v.first_pos, v.n_reads, np.uint32),
                   ref_w=arr(v.ref_w, v.n_reads, np.int32), flags=arr(v.flags, v.n_reads, np.uint8))

    def c(self):
        return np2_vote_t(len(self.pair_key), self.pair_key.ctypes.data, self.pair_cnt.ctypes.data, len(self.read_id),
                          self.read_id.ctypes.data, self.first_pos.ctypes.data, self.ref_w.ctypes.data, self.flags.ctypes.data)

    def pack(self):
        """One uint8 array: [n_pairs, n_reads] + the fields, each padded to 8 bytes (the exchange between ranks)."""
        parts = [np.array([len(self.pair_key), len(self.read_id)], dtype=np.uint64).view(np.uint8)]
        for name, _ in self.FIELDS:
            a = getattr(self, name).view(np.uint8)
            parts.append(a)
            if a.shape[0] & 7:
                parts.append(np.zeros(8 - (a.shape[0] & 7), dtype=np.uint8))
        return np.concatenate(parts)

    @classmethod
    def unpack(cls, raw):
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        n_pairs, n_reads = (int(x) for x in raw[:16].view(np.uint64))
        off, out = 16, {}
        for name, dt in cls.FIELDS:
            n = n_pairs if name.startswith("pair") else n_reads
            nb = n * np.dtype(dt).itemsize
            out[name] = raw[off:off + nb].view(dt)
            off += (nb + 7) & ~7
        return cls(**out)

    def to_bytes(self):
        """Unpadded byte-string form (the one the recorded shard fixtures under tests/golden hold)."""
        hdr = np.array([len(self.pair_key), len(self.read_id)], dtype=np.uint64).tobytes()
        return hdr + b"".join(getattr(self, n).tobytes() for n, _ in self.FIELDS)

    @classmethod
    def from_bytes(cls, raw):
        n_pairs, n_reads = (int(x) for x in np.frombuffer(raw[:16], dtype=np.uint64))
        off, out = 16, {}
        for name, dt in cls.FIELDS:
            n = n_pairs if name.startswith("pair") else n_reads
            nb = n * np.dtype(dt).itemsize
            out[name] = np.frombuffer(raw[off:off + nb], dtype=dt)
            off += nb
        return cls(**out)


def vote_decide(votes, n_reads_total, opts: Opts = None):
    """np2_vote_decide: merge the shards' votes of one phasing pass, Louvain on the merged read graph -> sorted losers
    (contig-wide read ids).  Host only, deterministic: every rank can run it on the same gathered votes."""
    o = (opts or Opts()).c()
    arr = (np2_vote_t * len(votes))(*[v.c() for v in votes])
    out = np.zeros(max(1, n_reads_total), dtype=np.uint32)
    n = C.c_uint32()
    rc = lib().np2_vote_decide(arr, len(votes), n_reads_total, C.byref(o), out.ctypes.data, C.byref(n))
    if rc != 0:
        raise Np2Error(rc, "np2_vote_decide")
    return out[: n.value].copy()


class ShardRun:
    """One shard of a contig on one context: upload (from a host pileup, or an already resident shard built by
    io.shard_from_bam), then vote() / apply() per phasing pass, final()."""

    def __init__(self, polisher: Polisher, pileup, plan: np2_shard_plan_t, opts: Opts = None, verify=1024, resident=None,
                 own_contig=True):
        self._pol = polisher
        self.plan = plan
        self.verify = verify
        self._own = own_contig
        self._c = C.c_void_p()
        if resident is not None:
            self._c = resident  # np2_contig_t* of the shard (ownership taken unless own_contig=False: see upload_shard)
        else:
            polisher._check(lib().np2_shard_upload(polisher._h, pileup.ref.ctypes.data, pileup.L, pileup.reads.ctypes.data,
                                                   pileup.n_reads, pileup.nibbles.ctypes.data, pileup.nibbles.shape[0],
                                                   C.byref(plan), C.byref(self._c)))
        self._o = (opts or Opts()).c()
        self._r = C.c_void_p()
        rc = lib().np2_shard_begin(polisher._h, self._c, C.byref(plan), C.byref(self._o), verify, C.byref(self._r))
        if rc != 0:
            self.close()
            polisher._check(rc)

    def passes_left(self):
        return lib().np2_shard_passes_left(self._r)

    def vote(self, copy=True) -> Vote:
        v = np2_vote_t()
        self._pol._check(lib().np2_shard_vote(self._r, C.byref(v)))
        return Vote.from_c(v, copy)

    def vote_view(self) -> Vote:
        """vote() without the copy: valid until this run's next call (the shard protocol packs or decides it at once)."""
        return self.vote(copy=False)

    def apply(self, losers):
        a = np.ascontiguousarray(losers, dtype=np.uint32)
        self._pol._check(lib().np2_shard_apply(self._r, a.ctypes.data, len(a)))

    def final(self):
        ob, op, on = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._pol._check(lib().np2_shard_final(self._r, C.byref(ob), C.byref(op), C.byref(on)))
        return _owned(ob, on.value, C.c_uint8), _owned(op, on.value, C.c_uint32)

    def final_device(self):
        """The final pass with the polished sub-contig left on the device -> ShardPiece (owned slice: device address +
        length; verification strips on the host)."""
        pc = np2_shard_piece_t()
        self._pol._check(lib().np2_shard_final_device(self._r, C.byref(pc)))
        return ShardPiece(pc)

    def fetch(self, dst_bases, dst_pos=None):
        """Copy the owned slice of the last final_device() into host arrays (slices of a pinned_array for long ones)."""
        self._pol._check(lib().np2_shard_fetch(self._r, dst_bases.ctypes.data, dst_pos.ctypes.data if dst_pos is not None else None))

    def close(self):
        if getattr(self, "_r", None):
            lib().np2_shard_end(self._r)
            self._r = None
        if getattr(self, "_c", None):
            if self._own:
                lib().np2_contig_free(self._pol._h, self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload_shard(polisher: Polisher, pileup: Pileup, plan: np2_shard_plan_t):
    """np2_shard_upload on its own: the resident shard (np2_contig_t*) of `plan`, to be polished any number of times by
    ShardRun(polisher, None, plan, ..., resident=h, own_contig=False); release it with free_shard."""
    h = C.c_void_p()
    polisher._check(lib().np2_shard_upload(polisher._h, pileup.ref.ctypes.data, pileup.L, pileup.reads.ctypes.data,
                                           pileup.n_reads, pileup.nibbles.ctypes.data, pileup.nibbles.shape[0],
                                           C.byref(plan), C.byref(h)))
    return h


def free_shard(polisher: Polisher, h):
    lib().np2_contig_free(polisher._h, h)


class ShardPiece:
    """Host view of np2_shard_piece_t: the owned slice stays on the device (dev_bases / dev_pos, own_len), the two strips
    around the cuts are numpy arrays (contig coordinates) freed with the object."""

    def __init__(self, pc: np2_shard_piece_t):
        self.own_len = int(pc.own_len)
        self.dev_bases, self.dev_pos = pc.dev_bases, pc.dev_pos
        self.first_pos, self.last_pos = int(pc.first_pos), int(pc.last_pos)

        def take(ptr, n, ct, dt):
            if not n or not ptr:
                return np.zeros(0, dtype=dt)
            return _owned(C.c_void_p(ptr), n, ct)
        self.lo_bases, self.lo_pos = take(pc.lo_bases, pc.lo_len, C.c_uint8, np.uint8), take(pc.lo_pos, pc.lo_len, C.c_uint32, np.uint32)
        self.hi_bases, self.hi_pos = take(pc.hi_bases, pc.hi_len, C.c_uint8, np.uint8), take(pc.hi_pos, pc.hi_len, C.c_uint32, np.uint32)

    def strips(self):
        """(lo_bases, lo_pos, hi_bases, hi_pos) as one uint8 array (exchange between ranks) — see unpack_strips."""
        hdr = np.array([self.own_len, self.first_pos, self.last_pos, len(self.lo_bases), len(self.hi_bases)], dtype=np.uint64)
        return np.concatenate([hdr.view(np.uint8), self.lo_pos.view(np.uint8), self.hi_pos.view(np.uint8), self.lo_bases, self.hi_bases])

    @staticmethod
    def unpack_strips(raw):
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        own_len, first, last, nl, nh = (int(x) for x in raw[:40].view(np.uint64))
        o = 40
        lo_pos = raw[o:o + 4 * nl].view(np.uint32); o += 4 * nl
        hi_pos = raw[o:o + 4 * nh].view(np.uint32); o += 4 * nh
        lo_b = raw[o:o + nl]; o += nl
        hi_b = raw[o:o + nh]
        return {"own_len": own_len, "first_pos": first, "last_pos": last, "lo_bases": lo_b, "lo_pos": lo_pos,
                "hi_bases": hi_b, "hi_pos": hi_pos}


def pinned_array(n, dtype=np.uint8):
    """A page-locked host array from the library's result pool (np2_alloc_pinned): large device-to-host copies into
    pageable memory stall on lazy pinning."""
    dt = np.dtype(dtype)
    p = lib().np2_alloc_pinned(max(1, int(n)) * dt.itemsize)
    if not p:  # (no device in this process, e.g. the CPU-only replay tests: plain memory does the same job, slower)
        return np.empty(int(n), dtype=dt)
    ct = {1: C.c_uint8, 4: C.c_uint32, 8: C.c_uint64}[dt.itemsize]
    return _owned(C.c_void_p(p), int(n), ct).view(dt)


def fasta_record(name, bases, pos):
    """display_consensusbase_vec (src/main.rs:607-645): '>{name} start:{first} end:{last}\\n{seq}\\n'."""
    return b">%s start:%d end:%d\n%s\n" % (name.encode() if isinstance(name, str) else name, int(pos[0]), int(pos[-1]),
                                           bytes(bases))


def swiss_order(script):
    """np2_swiss_order: iteration order of the product's SwissTable order model after [(op, key)] (0 insert, 1 remove,
    2 entry)."""
    ops = np.array([o for o, _ in script], dtype=np.uint32)
    keys = np.array([k for _, k in script], dtype=np.uint32)
    out = np.zeros(max(1, len(script)), dtype=np.uint32)
    n = C.c_uint32()
    if lib().np2_swiss_order(ops.ctypes.data, keys.ctypes.data, len(script), out.ctypes.data, C.byref(n)) != 0:
        raise Np2Error(-1, "np2_swiss_order")
    return out[: n.value].tolist()


@contextlib.contextmanager
def alloc_poison(byte):
    """np2_debug_poison for the length of a with block (a test hook): every block the device pools and the pinned pool
    hand out inside it is filled with `byte` (0..255) first; None switches the fill off.  The old setting comes back on
    exit.  A context keeps its buffers, so make it inside the block."""
    old = lib().np2_debug_poison(-1 if byte is None else int(byte) & 255)
    try:
        yield
    finally:
        lib().np2_debug_poison(old)


def alloc_poison_stats():
    """(device bytes, pinned bytes) the poison hook has filled since the process started."""
    d, p = C.c_uint64(), C.c_uint64()
    lib().np2_debug_poison_stats(C.byref(d), C.byref(p))
    return d.value, p.value


def phase_vote(keys, pairs, ref=None):
    """Host-only phasing vote of the product library (np2_phase_vote): keys in creation order, pairs [(a, b, w)],
    ref = {read: weight} or None -> sorted losing reads."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    pa = np.array([p[0] for p in pairs], dtype=np.uint32)
    pb = np.array([p[1] for p in pairs], dtype=np.uint32)
    pw = np.array([p[2] for p in pairs], dtype=np.float32)
    ri = np.array(list(ref.keys()) if ref else [], dtype=np.uint32)
    rw = np.array(list(ref.values()) if ref else [], dtype=np.float32)
    out = np.zeros(max(1, len(keys)), dtype=np.uint32)
    n = C.c_uint32()
    rc = lib().np2_phase_vote(keys.ctypes.data, len(keys), pa.ctypes.data, pb.ctypes.data, pw.ctypes.data, len(pairs),
                              ri.ctypes.data, rw.ctypes.data, len(ri), 1 if ref is not None else 0, out.ctypes.data,
                              C.byref(n))
    if rc != 0:
        raise Np2Error(rc, "np2_phase_vote")
    return out[: n.value].tolist()


def _rep_opts(k, distinct, min_count):
    if min_count is not None and not 0 <= int(min_count) <= 0xFFFFFFFF:
        raise ValueError("min_count: 0 .. 2^32 - 1")
    if not 0 <= int(k) <= 0xFFFFFFFF:
        raise ValueError("k must not be negative")
    return np2_rep_opts_t(int(k), 0 if min_count is None else 1, 0 if min_count is None else int(min_count), float(distinct))


def _rep_check(rc):
    if rc != 0:
        raise Np2Error(rc, (lib().np2_io_last_error() or b"").decode())


def rep_bytes(seq, k=15, distinct=0.9998, min_count=None, device=0):
    """np2_rep_bytes: the repetitive k-mers of a separator stream (sequences' bytes, any non-base byte between them) ->
    (index, count, stats): the canonical indices with count > threshold in ascending order as uint32 arrays, and the
    np2_rep_stats_t fields as a dict.  The threshold comes from `distinct` (meryl's greater-than distinct=f), or is
    `min_count` when that is given (greater-than N).  The rule: include/np2_io.h."""
    L = lib()
    s = np.frombuffer(seq, dtype=np.uint8)
    o, st = _rep_opts(k, distinct, min_count), np2_rep_stats_t()
    pi, pc, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    _rep_check(L.np2_rep_bytes(device, s.ctypes.data if len(s) else None, len(s), C.byref(o), C.byref(pi), C.byref(pc), C.byref(n),
                               C.byref(st)))
    try:
        index = np.asarray(_Raw(pi.value, n.value, "<u4")).copy() if n.value else np.zeros(0, np.uint32)
        count = np.asarray(_Raw(pc.value, n.value, "<u4")).copy() if n.value else np.zeros(0, np.uint32)
    finally:
        L.np2_free(pi)
        L.np2_free(pc)
    return index, count, {f: getattr(st, f) for f, _ in np2_rep_stats_t._fields_}


def rep_files(paths, out_path, k=15, distinct=0.9998, min_count=None, both=False, device=0):
    """np2_rep_files: FASTA files (plain or gzip) -> the text file `out_path`, one "KMER<tab>COUNT" line per listed k-mer
    (with `both`, its reverse complement on the next line) -> the stats dict."""
    L = lib()
    paths = [paths] if isinstance(paths, (str, os.PathLike)) else list(paths)
    arr = (C.c_char_p * max(1, len(paths)))(*[os.fspath(p).encode() for p in paths])
    o, st = _rep_opts(k, distinct, min_count), np2_rep_stats_t()
    _rep_check(L.np2_rep_files(device, arr, len(paths), C.byref(o), None if out_path is None else os.fspath(out_path).encode(),
                               1 if both else 0, C.byref(st)))
    return {f: getattr(st, f) for f, _ in np2_rep_stats_t._fields_}
