"""ctypes binding of liburmapx.so (include/urmapx.h) -- the host-side mirror of the reference seam
State1::SetMethod / SetUFI / Search (map.cpp:11-25) and UFIndex::FromFile (ufindexio.cpp:51-115).

Nothing here computes on the CPU: every call goes to the HIP library, and a missing or unloadable
library is a hard error.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("URMAPX_LIB") or os.path.join(_HERE, "liburmapx.so")  # URMAPX_LIB: A/B builds

MAX_QL = 1024
MAX_PATH_OPS = int(os.environ.get("URMAPX_MAX_PATH_OPS_OVERRIDE", 96))
E_IO, E_FORMAT, E_NOMEM, E_NODEVICE, E_ARG = -1, -2, -3, -4, -5
E_UNSUPPORTED = -6

RESULT_DTYPE = np.dtype([("dbpos", "<u4"), ("seq_index", "<u4"), ("coord", "<u4"), ("score", "<i2"),
                         ("second", "<i2"), ("mapq", "u1"), ("plus", "u1"), ("exit_phase", "u1"),
                         ("status", "u1"), ("hit_count", "<u2"), ("path_nops", "<u2"), ("path_off", "<u4")])
assert RESULT_DTYPE.itemsize == 28

EXPORTS = (
    "urmapx_params_for_method", "urmapx_index_open", "urmapx_index_wrap_host", "urmapx_index_wrap_device",
    "urmapx_index_upload", "urmapx_index_replicate", "urmapx_index_close", "urmapx_index_chain_row_bytes", "urmapx_index_validate", "urmapx_index_word_length", "urmapx_index_max_ix",
    "urmapx_index_slot_count", "urmapx_index_seqdata_size", "urmapx_index_seq_count", "urmapx_index_label",
    "urmapx_index_seq_length", "urmapx_index_seq_offset", "urmapx_ctx_create", "urmapx_ctx_destroy",
    "urmapx_map_se", "urmapx_map_se_device", "urmapx_ctx_sync", "urmapx_ctx_last_kernel_ms",
    "urmapx_seed_probe", "urmapx_seed_probe_device", "urmapx_viterbi_batch", "urmapx_strerror", "urmapx_device_arch",
    "urmapx_make_ufi", "urmapx_make_ufi_opts", "urmapx_build_slots", "urmapx_make_ufi_gpu", "urmapx_build_slots_gpu", "urmapx_sam_se", "urmapx_sam_header_sq", "urmapx_ctx_phase_cycles", "urmapx_ctx_read_cycles", "urmapx_ctx_stage_ms", "urmapx_ctx_phase3", "urmapx_ctx_round_ms", "urmapx_ctx_dp_rounds", "urmapx_ctx_dp_stats", "urmapx_map_pe", "urmapx_sam_pe", "urmapx_map_pe_device", "urmapx_ctx_set_pe_veryfast",
    "urmapx_gunzip_file", "urmapx_fastq_open", "urmapx_fastq_next", "urmapx_fastq_error", "urmapx_fastq_close",
    "urmapx_ctx_gather_microbench", "urmapx_map_files", "urmapx_host_pool_trim", "urmapx_text_create", "urmapx_text_destroy", "urmapx_text_map_se", "urmapx_text_map_pe", "urmapx_pgzip_simd", "urmapx_index_open_device", "urmapx_text_fetch_sam", "urmapx_text_set_deferred", "urmapx_text_wait", "urmapx_text_fetch_pairs", "urmapx_ctx_set_pair_info", "urmapx_ctx_get_pair_info", "urmapx_tab_pe",
    "urmapx_checksum_device", "urmapx_index_checksum", "urmapx_index_layout_checksum",
    "urmapx_bitvec_build", "urmapx_bitvec_open", "urmapx_bitvec_wrap_host", "urmapx_bitvec_save", "urmapx_bitvec_download",
    "urmapx_bitvec_word_length", "urmapx_bitvec_bytes", "urmapx_bitvec_popcount", "urmapx_bitvec_search", "urmapx_bitvec_search_device",
    "urmapx_bitvec_sync", "urmapx_bitvec_last_ms", "urmapx_bitvec_close", "urmapx_make_bitvec", "urmapx_search_bitvec_files",
    "urmapx_index_stats", "urmapx_index_slot_counts", "urmapx_ufi_info",
    "urmapx_bgzf_bound", "urmapx_bgzf_compress_host", "urmapx_bgzf_compress", "urmapx_bgzf_compress_timed", "urmapx_bgzf_code_lengths", "urmapx_bgzf_create",
    "urmapx_bgzf_destroy", "urmapx_bgzf_compress_device", "urmapx_text_set_bgzf",
    "urmapx_text_set_bam", "urmapx_bam_header", "urmapx_bam_se", "urmapx_bam_pe",
    "urmapx_bam_sort", "urmapx_bam_sort_host", "urmapx_bam_sort_free", "urmapx_bam_sort_device_bytes",
    "urmapx_bam_sort_markdup", "urmapx_bam_sort_markdup_host", "urmapx_bam_sort_markdup_device_bytes",
    "urmapx_bam_sort_plan_for", "urmapx_bam_sort_external",
    "urmapx_bam_depth", "urmapx_bam_depth_host", "urmapx_depth_free", "urmapx_bam_depth_device_bytes", "urmapx_bam_depth_resident_bytes",
    "urmapx_map_depth_summary",
    "urmapx_bam_stats", "urmapx_bam_stats_host", "urmapx_stats_free", "urmapx_bam_stats_resident_bytes",
    "urmapx_bam_pileup", "urmapx_bam_pileup_host", "urmapx_pileup_free", "urmapx_bam_pileup_resident_bytes", "urmapx_bam_pileup_device_bytes",
    "urmapx_bam_sort_with", "urmapx_bam_sort_with_host",
    "urmapx_calmd", "urmapx_ref_span", "urmapx_sam_se_tags", "urmapx_sam_pe_tags", "urmapx_bam_se_tags", "urmapx_bam_pe_tags",
    "urmapx_read_group_id", "urmapx_sam_header_rg", "urmapx_bam_header_rg", "urmapx_index_fetch_spans", "urmapx_text_set_tags",
    "urmapx_text_tag_ms", "urmapx_tags_batch",
)

TAG_NM, TAG_MD, TAG_AS, TAG_ALL = 1, 2, 4, 7

BV_MAGIC = 0x42563130
BV_MIN_W, BV_MAX_W = 2, 20
BV_TRUNC_LABELS = 1
VERDICT_NONE, VERDICT_FORWARD, VERDICT_REVERSE = 0, 1, 2


PAIR_INFO_DTYPE = np.dtype([("top_db", "<u4", 2), ("second_db", "<u4", 2), ("top_score", "<i2", 2), ("second_score", "<i2", 2),
                            ("top_plus", "u1", 2), ("second_plus", "u1", 2)])
assert PAIR_INFO_DTYPE.itemsize == 28


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "mismatch_score", "gap_open_score", "gap_ext_score", "min_hsp_score_pct",
        "term_hsp_score_pct_phase3", "xdrop", "max_penalty", "xphase1", "xphase3", "xphase4")] + [
        ("band_radius", C.c_uint32)]


class MapOptions(C.Structure):
    _fields_ = [("first_gpu", C.c_int), ("gpus", C.c_int), ("streams", C.c_int), ("host_threads", C.c_int), ("batch", C.c_uint32),
                ("veryfast", C.c_int), ("minq", C.c_uint), ("cmdline", C.c_char_p), ("sam_shards", C.c_int), ("discard_sam", C.c_int), ("bgzf", C.c_int),
                ("bam", C.c_int), ("bam_sort", C.c_int), ("tags", C.c_uint), ("read_group", C.c_char_p)]


class MapOptionsMarkdup(C.Structure):
    """urmapx_map_options as urmapx_map_files reads it: MapOptions (the struct up to read_group, whose layout tests/test_tags_cpu.py
    pins) with the field appended behind it.  map_files always passes this one."""
    _fields_ = MapOptions._fields_ + [("markdup", C.c_int)]


class MapOptionsSortMem(C.Structure):
    """urmapx_map_options in full: MapOptionsMarkdup with sort_mem appended (the earlier layouts stay pinned by their tests)"""
    _fields_ = MapOptionsMarkdup._fields_ + [("sort_mem", C.c_uint64)]


class MapOptionsDepth(C.Structure):
    """urmapx_map_options in full: MapOptionsSortMem with depth_out and depth_mapq appended.  map_files passes this one."""
    _fields_ = MapOptionsSortMem._fields_ + [("depth_out", C.c_char_p), ("depth_mapq", C.c_uint32)]


class MapOptionsStats(C.Structure):
    """urmapx_map_options in full: MapOptionsDepth with stats_out appended.  map_files passes this one."""
    _fields_ = MapOptionsDepth._fields_ + [("stats_out", C.c_char_p)]


class MapOptionsPileup(C.Structure):
    """urmapx_map_options in full: MapOptionsStats with vcf_out and its four thresholds appended.  map_files passes this one."""
    _fields_ = MapOptionsStats._fields_ + [("vcf_out", C.c_char_p), ("vcf_mapq", C.c_uint32), ("vcf_baseq", C.c_uint32), ("vcf_min_alt", C.c_uint32),
                                           ("vcf_min_pct", C.c_uint32)]


class TagOptions(C.Structure):
    _fields_ = [("tags", C.c_uint), ("rg_id", C.c_char_p), ("ref", C.c_void_p * 2)]


class MapReport(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("mapped_q", C.c_uint64), ("mapped_lowq", C.c_uint64), ("unmapped", C.c_uint64),
                ("unsupported", C.c_uint64), ("seconds", C.c_double), ("parse_s", C.c_double), ("gpu_s", C.c_double),
                ("format_s", C.c_double), ("write_s", C.c_double), ("host_threads", C.c_int), ("lanes", C.c_int),
                ("write_threads", C.c_int), ("text_on_device", C.c_int), ("input_bytes", C.c_uint64), ("medium", C.c_char * 24),
                ("dev_h2d_s", C.c_double), ("dev_parse_s", C.c_double), ("dev_map_s", C.c_double), ("dev_format_s", C.c_double),
                ("dev_d2h_s", C.c_double), ("shards", C.c_int), ("placement", C.c_char * 256), ("shard_scan_s", C.c_double),
                ("dev_map_search_s", C.c_double), ("dev_map_dp_s", C.c_double), ("map_enqueue_s", C.c_double),
                ("alloc_dev_s", C.c_double), ("alloc_pinned_s", C.c_double), ("alloc_dev_calls", C.c_uint32), ("alloc_pinned_calls", C.c_uint32),
                ("sam_text_bytes", C.c_uint64), ("sam_file_bytes", C.c_uint64), ("sort_s", C.c_double),
                ("pairs_examined", C.c_uint64), ("pairs_duplicate", C.c_uint64), ("fragments_examined", C.c_uint64),
                ("fragments_duplicate", C.c_uint64), ("markdup_s", C.c_double)]


class MapReportSort(C.Structure):
    """urmapx_map_report in full: MapReport with sort_partitions appended.  map_files passes this one."""
    _fields_ = MapReport._fields_ + [("sort_partitions", C.c_uint32)]


class MapReportDepth(C.Structure):
    """urmapx_map_report in full: MapReportSort with the depth's seconds and totals appended.  map_files passes this one."""
    _fields_ = MapReportSort._fields_ + [("depth_s", C.c_double), ("depth_runs", C.c_uint64), ("depth_covered", C.c_uint64), ("depth_bases", C.c_uint64)]


class MapReportStats(C.Structure):
    """urmapx_map_report in full: MapReportDepth with the statistics' seconds and totals appended.  map_files passes this one."""
    _fields_ = MapReportDepth._fields_ + [("stats_s", C.c_double), ("stats_reads", C.c_uint64), ("stats_mapped", C.c_uint64),
                                          ("stats_properly_paired", C.c_uint64), ("stats_duplicated", C.c_uint64), ("stats_insert_median", C.c_uint64)]


class MapReportPileup(C.Structure):
    """urmapx_map_report in full: MapReportStats with the pileup's seconds and totals appended.  map_files passes this one."""
    _fields_ = MapReportStats._fields_ + [("pileup_s", C.c_double), ("pileup_sites", C.c_uint64), ("pileup_records", C.c_uint64), ("pileup_alt_alleles", C.c_uint64)]


class BamSortResult(C.Structure):
    _fields_ = [("bgzf", C.c_void_p), ("bai", C.c_void_p), ("bgzf_bytes", C.c_size_t), ("bai_bytes", C.c_size_t),
                ("stream_bytes", C.c_uint64), ("records", C.c_uint64), ("no_coor", C.c_uint64), ("sort_passes", C.c_uint32),
                ("slices", C.c_uint32), ("scan_s", C.c_double), ("alloc_s", C.c_double), ("upload_s", C.c_double), ("sort_s", C.c_double),
                ("gather_s", C.c_double), ("deflate_s", C.c_double), ("copy_s", C.c_double), ("index_s", C.c_double),
                ("external", C.c_uint32), ("partitions", C.c_uint32), ("stage_chunks", C.c_uint64), ("stage_s", C.c_double)]


class BamSortPlan(C.Structure):
    _fields_ = [("external", C.c_int), ("partition_bytes", C.c_uint64), ("partitions", C.c_uint64), ("stage_bytes", C.c_uint64),
                ("device_bytes", C.c_uint64)]


class MarkdupStats(C.Structure):
    _fields_ = [("pairs_examined", C.c_uint64), ("pairs_duplicate", C.c_uint64), ("fragments_examined", C.c_uint64),
                ("fragments_duplicate", C.c_uint64), ("markdup_s", C.c_double)]


class DepthOpts(C.Structure):
    _fields_ = [("min_mapq", C.c_uint32)]


class DepthSummary(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("covered", C.c_uint64), ("bases", C.c_uint64), ("mapq_sum", C.c_uint64)]


class DepthResult(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_bytes", C.c_size_t), ("runs", C.c_uint64), ("refs", C.POINTER(DepthSummary)),
                ("n_ref", C.c_uint32), ("text_slices", C.c_uint32), ("records", C.c_uint64), ("stage_chunks", C.c_uint64),
                ("least_budget", C.c_uint64), ("alloc_s", C.c_double), ("count_s", C.c_double), ("scan_s", C.c_double),
                ("runs_s", C.c_double), ("format_s", C.c_double), ("copy_s", C.c_double)]


class ValidateReport(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("slots", "heads", "positions", "used", "reached", "bad_hash", "bad_pos", "bad_link", "bad_len",
                                          "first_bad_slot")] + [("seconds", C.c_double)]


class StatsResult(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_bytes", C.c_size_t), ("records", C.c_uint64), ("reads", C.c_uint64), ("mapped", C.c_uint64),
                ("properly_paired", C.c_uint64), ("duplicated", C.c_uint64), ("insert_median", C.c_uint64), ("stage_chunks", C.c_uint64),
                ("least_budget", C.c_uint64), ("alloc_s", C.c_double), ("count_s", C.c_double), ("format_s", C.c_double)]


class PileupOpts(C.Structure):
    _fields_ = [("min_mapq", C.c_uint32), ("min_baseq", C.c_uint32), ("min_alt", C.c_uint32), ("min_pct", C.c_uint32)]


class PileupResult(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_bytes", C.c_size_t), ("sites", C.c_uint64), ("alt_alleles", C.c_uint64), ("records", C.c_uint64),
                ("stage_chunks", C.c_uint64), ("least_budget", C.c_uint64), ("alloc_s", C.c_double), ("count_s", C.c_double), ("sites_s", C.c_double),
                ("format_s", C.c_double), ("copy_s", C.c_double)]


class BamSortExtras(C.Structure):
    """urmapx_bam_sort_extras: what urmapx_bam_sort_with takes on the way"""
    _fields_ = [("md", C.POINTER(MarkdupStats)), ("dopts", C.POINTER(DepthOpts)), ("names", C.POINTER(C.c_char_p)), ("lens", C.c_void_p),
                ("depth", C.POINTER(DepthResult)), ("stats", C.POINTER(StatsResult)), ("stats_command", C.c_char_p),
                ("popts", C.POINTER(PileupOpts)), ("seqs", C.POINTER(C.c_char_p)), ("index", C.c_void_p), ("pileup", C.POINTER(PileupResult)),
                ("pileup_command", C.c_char_p)]


STATS_FIELDS = ("word_length", "max_ix", "seqdata_size", "slots", "indexed", "not_indexed", "wildcard", "indexed2", "free", "collision",
                "single_both", "single_plus", "end", "mine", "other", "trunc", "trunc2", "long_mine", "long_other", "total", "bad_rows",
                "first_bad_slot")


class UfiStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in STATS_FIELDS] + [("count_hist", C.c_uint64 * 256), ("trunc_hist", C.c_uint64 * 256),
                                                          ("position_seconds", C.c_double), ("slot_seconds", C.c_double)]


class TextReport(C.Structure):
    _fields_ = [("records", C.c_uint32), ("reason", C.c_uint32), ("sam_bytes", C.c_uint64), ("mapped_q", C.c_uint64),
                ("mapped_lowq", C.c_uint64), ("unmapped", C.c_uint64), ("unsupported", C.c_uint64),
                ("ms_h2d", C.c_float), ("ms_parse", C.c_float), ("ms_map", C.c_float), ("ms_format", C.c_float), ("ms_d2h", C.c_float),
                ("ms_map_search", C.c_float), ("ms_map_dp", C.c_float), ("ms_map_enqueue", C.c_float), ("sam_text_bytes", C.c_uint64)]


TEXT_OK, TEXT_CR, TEXT_RAGGED, TEXT_BAD_RECORD, TEXT_LONG_NAME, TEXT_SAM_CAP, TEXT_TOO_LARGE, TEXT_UNEQUAL, TEXT_INTERNAL, TEXT_DEFERRED = range(10)


class UrmapxError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super().__init__(f"{what}: {strerror(code)} ({code})")


_lib = None


def lib():
    """Load liburmapx.so (built in-tree by __graft_entry__.build()); fails loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP library is the only compute path; there is no fallback)")
    L = C.CDLL(LIB_PATH)
    vp, cp, u32, u64, i32 = C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint64, C.c_int
    L.urmapx_params_for_method.argtypes = [C.c_uint, C.POINTER(Params)]
    L.urmapx_index_open.argtypes = [cp, C.POINTER(vp)]
    L.urmapx_index_wrap_host.argtypes = [u32, u32, u64, vp, vp, u32, u32, vp, vp, cp, C.POINTER(vp)]
    L.urmapx_index_wrap_device.argtypes = [i32, u32, u32, u64, vp, vp, u32, u32, vp, vp, cp, C.POINTER(vp)]
    L.urmapx_index_upload.argtypes = [vp, i32]
    L.urmapx_index_replicate.argtypes = [vp, i32, C.POINTER(vp)]
    L.urmapx_index_close.argtypes = [vp]
    L.urmapx_index_close.restype = None
    for name, rt in (("word_length", u32), ("max_ix", u32), ("slot_count", u64), ("seqdata_size", u32),
                     ("seq_count", u32), ("chain_row_bytes", u64)):
        f = getattr(L, "urmapx_index_" + name)
        f.restype = rt
        f.argtypes = [vp]
    L.urmapx_index_validate.argtypes = [vp, C.POINTER(ValidateReport)]
    L.urmapx_index_stats.argtypes = [vp, C.POINTER(UfiStats)]
    L.urmapx_index_slot_counts.argtypes = [vp, i32, vp, u64]
    L.urmapx_ufi_info.argtypes = [cp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
    L.urmapx_checksum_device.argtypes = [i32, vp, u64, C.POINTER(u64)]
    L.urmapx_index_checksum.argtypes = [vp, C.POINTER(u64)]
    L.urmapx_index_layout_checksum.argtypes = [vp, C.POINTER(u64)]
    L.urmapx_index_label.restype = cp
    L.urmapx_index_label.argtypes = [vp, u32]
    L.urmapx_index_seq_length.restype = u32
    L.urmapx_index_seq_length.argtypes = [vp, u32]
    L.urmapx_index_seq_offset.restype = u32
    L.urmapx_index_seq_offset.argtypes = [vp, u32]
    L.urmapx_ctx_create.argtypes = [vp, i32, C.POINTER(Params), C.POINTER(vp)]
    L.urmapx_ctx_destroy.argtypes = [vp]
    L.urmapx_ctx_destroy.restype = None
    L.urmapx_map_se.argtypes = [vp, vp, vp, u32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.urmapx_map_pe.argtypes = [vp, vp, vp, u32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.urmapx_sam_pe.restype = C.c_size_t
    L.urmapx_sam_pe.argtypes = [vp, vp, vp, vp, cp, vp, vp, u32, cp, vp, vp, u32, vp, C.c_size_t]
    L.urmapx_map_se_device.argtypes = [vp, vp, vp, u32, u64, u32, vp, vp, vp]
    L.urmapx_map_pe_device.argtypes = [vp, vp, vp, u32, u64, u32, vp, vp, vp]
    L.urmapx_ctx_set_pe_veryfast.argtypes = [vp, i32]
    L.urmapx_ctx_sync.argtypes = [vp]
    L.urmapx_ctx_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float * 2)]
    L.urmapx_ctx_phase_cycles.argtypes = [vp, C.POINTER(C.c_uint64 * 12)]
    L.urmapx_ctx_read_cycles.argtypes = [vp, vp, u32]
    L.urmapx_seed_probe_device.argtypes = [vp, vp, vp, u32, u64, u32, C.POINTER(C.c_float)]
    L.urmapx_ctx_stage_ms.argtypes = [vp, C.POINTER(C.c_float * 7)]
    L.urmapx_ctx_phase3.argtypes = [vp, C.POINTER(C.c_float * 3), C.POINTER(C.c_uint32 * 2)]
    L.urmapx_ctx_round_ms.argtypes = [vp, C.POINTER(C.c_float * 16), C.POINTER(C.c_int)]
    L.urmapx_ctx_dp_stats.argtypes = [vp, C.POINTER(C.c_uint32 * 8)]
    L.urmapx_seed_probe.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    L.urmapx_viterbi_batch.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.urmapx_make_ufi.argtypes = [cp, cp, u32, u32, u64]
    L.urmapx_build_slots.argtypes = [vp, u32, u32, u32, u64, vp, C.POINTER(u32)]
    L.urmapx_make_ufi_gpu.argtypes = [i32, cp, cp, u32, u32, u64]
    L.urmapx_build_slots_gpu.argtypes = [i32, vp, vp, u32, u32, u32, u64, vp, C.POINTER(u32)]
    L.urmapx_sam_se.restype = C.c_size_t
    L.urmapx_sam_se.argtypes = [vp, vp, vp, cp, vp, vp, u32, vp, C.c_size_t]
    L.urmapx_sam_header_sq.restype = C.c_size_t
    L.urmapx_sam_header_sq.argtypes = [vp, vp, C.c_size_t]
    L.urmapx_strerror.restype = cp
    L.urmapx_strerror.argtypes = [i32]
    L.urmapx_device_arch.restype = cp
    L.urmapx_device_arch.argtypes = [vp]
    L.urmapx_ctx_gather_microbench.argtypes = [vp, u64, C.POINTER(C.c_double)]
    L.urmapx_ctx_set_pair_info.argtypes = [vp, i32]
    L.urmapx_ctx_get_pair_info.argtypes = [vp, vp, u32]
    L.urmapx_tab_pe.restype = C.c_size_t
    L.urmapx_tab_pe.argtypes = [vp, vp, vp, vp, cp, u32, u32, i32, vp, C.c_size_t]
    L.urmapx_map_files.argtypes = [vp, C.POINTER(MapOptionsPileup), cp, cp, cp, cp, C.POINTER(MapReportPileup), cp, C.c_size_t]
    L.urmapx_map_depth_summary.argtypes = []
    L.urmapx_map_depth_summary.restype = C.c_char_p
    L.urmapx_host_pool_trim.argtypes = []
    L.urmapx_host_pool_trim.restype = None
    L.urmapx_text_create.argtypes = [vp, C.POINTER(vp)]
    L.urmapx_text_destroy.argtypes = [vp]
    L.urmapx_text_destroy.restype = None
    L.urmapx_text_map_se.argtypes = [vp, vp, C.c_size_t, C.c_uint, vp, C.c_size_t, C.POINTER(TextReport)]
    L.urmapx_text_map_pe.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint, vp, C.c_size_t, C.POINTER(TextReport)]
    L.urmapx_text_fetch_sam.argtypes = [vp, vp, C.c_size_t, C.POINTER(TextReport)]
    L.urmapx_text_set_deferred.argtypes = [vp, C.c_int]
    L.urmapx_text_wait.argtypes = [vp, C.POINTER(TextReport)]
    L.urmapx_fastq_open.argtypes = [cp, C.POINTER(vp)]
    L.urmapx_fastq_next.restype = C.c_int64
    L.urmapx_fastq_next.argtypes = [vp, u32] + [C.POINTER(vp)] * 5
    L.urmapx_fastq_error.restype = cp
    L.urmapx_fastq_error.argtypes = [vp]
    L.urmapx_fastq_close.restype = None
    L.urmapx_fastq_close.argtypes = [vp]
    L.urmapx_bitvec_build.argtypes = [i32, vp, vp, u32, vp, vp, u32, u32, C.POINTER(vp), C.POINTER(u64 * 2)]
    L.urmapx_bitvec_open.argtypes = [cp, i32, C.POINTER(vp)]
    L.urmapx_bitvec_wrap_host.argtypes = [i32, u32, vp, C.POINTER(vp)]
    L.urmapx_bitvec_save.argtypes = [vp, cp]
    L.urmapx_bitvec_download.argtypes = [vp, vp, u64]
    L.urmapx_bitvec_word_length.restype = u32
    L.urmapx_bitvec_word_length.argtypes = [vp]
    L.urmapx_bitvec_bytes.restype = u64
    L.urmapx_bitvec_bytes.argtypes = [vp]
    L.urmapx_bitvec_popcount.argtypes = [vp, C.POINTER(u64)]
    L.urmapx_bitvec_search.argtypes = [vp, vp, vp, u32, vp]
    L.urmapx_bitvec_search_device.argtypes = [vp, vp, vp, u32, vp]
    L.urmapx_bitvec_sync.argtypes = [vp]
    L.urmapx_bitvec_last_ms.argtypes = [vp, C.POINTER(C.c_float * 3)]
    L.urmapx_bitvec_close.argtypes = [vp]
    L.urmapx_bitvec_close.restype = None
    L.urmapx_make_bitvec.argtypes = [i32, cp, cp, u32, cp, C.POINTER(u64 * 2)]
    L.urmapx_search_bitvec_files.argtypes = [vp, cp, cp, cp, cp, C.c_uint, C.POINTER(u64 * 2), cp, C.c_size_t]
    _lib = L
    return L


def strerror(code):
    return lib().urmapx_strerror(code).decode()


def _check(rc, what, allow=()):
    if rc != 0 and rc not in allow:
        raise UrmapxError(rc, what)
    return rc


def params_for_method(method=6) -> Params:
    """State1::SetMethod (state1.cpp:147-183): 6 = default, 7 = -veryfast."""
    p = Params()
    _check(lib().urmapx_params_for_method(method, C.byref(p)), "urmapx_params_for_method")
    return p


def make_ufi(fasta, ufi, slots, word_length=24, max_ix=32):
    """urmap -make_ufi FASTA -output UFI -slots N (ufindexio.cpp:117-179)."""
    _check(lib().urmapx_make_ufi(os.fsencode(fasta), os.fsencode(ufi), word_length, max_ix, slots), "urmapx_make_ufi")


def build_slots(seqdata: np.ndarray, slots, word_length=24, max_ix=32) -> np.ndarray:
    """UFIndex::MakeIndex on a concatenated upper-case sequence store -> 5*slots byte slot table."""
    seqdata = np.ascontiguousarray(seqdata, dtype=np.uint8)
    blob = np.empty(5 * slots + 8, dtype=np.uint8)
    blob[5 * slots:] = 0
    trunc = C.c_uint32(0)
    _check(lib().urmapx_build_slots(seqdata.ctypes.data, len(seqdata), word_length, max_ix, slots, blob.ctypes.data,
                                    C.byref(trunc)), "urmapx_build_slots")
    return blob


def make_ufi_gpu(device, fasta, ufi, slots, word_length=24, max_ix=32):
    """-make_ufi with the counting passes, head slots and overflow list made on the GPU; byte-identical output."""
    _check(lib().urmapx_make_ufi_gpu(device, os.fsencode(fasta), os.fsencode(ufi), word_length, max_ix, slots), "urmapx_make_ufi_gpu")


def build_slots_gpu(device, slots, seqdata: np.ndarray | None = None, d_seq_ptr=None, size=None, word_length=24, max_ix=32) -> np.ndarray:
    """UFIndex::MakeIndex -> 5*slots byte slot table; the sequence store comes from a host array or is resident on
    `device` already (d_seq_ptr, size)."""
    blob = np.empty(5 * slots + 8, dtype=np.uint8)
    blob[5 * slots:] = 0
    trunc = C.c_uint32(0)
    if seqdata is not None:
        seqdata = np.ascontiguousarray(seqdata, dtype=np.uint8)
        size = len(seqdata)
    _check(lib().urmapx_build_slots_gpu(device, seqdata.ctypes.data if seqdata is not None else None, d_seq_ptr, size, word_length,
                                        max_ix, slots, blob.ctypes.data, C.byref(trunc)), "urmapx_build_slots_gpu")
    return blob


def checksum_device(device, d_ptr, nbytes):
    """urmapx_checksum_device: the checksum of `nbytes` device-resident bytes at the 8-byte-aligned address d_ptr"""
    out = C.c_uint64(0)
    _check(lib().urmapx_checksum_device(device, d_ptr, nbytes, C.byref(out)), "urmapx_checksum_device")
    return int(out.value)


class Index:
    """UFIndex (read side): parsed .ufi + its copy in HBM."""

    def __init__(self, handle, keep=()):
        self.h = C.c_void_p(handle)
        self._keep = keep

    @classmethod
    def open(cls, path):
        h = C.c_void_p()
        _check(lib().urmapx_index_open(os.fsencode(path), C.byref(h)), f"urmapx_index_open({path})")
        return cls(h.value)

    @classmethod
    def open_device(cls, path, device=0):
        """UFIndex::FromFile straight into the HBM of `device` (no host copy of the arrays is kept): what the command line loads with."""
        h = C.c_void_p()
        _check(lib().urmapx_index_open_device(os.fsencode(path), int(device), C.byref(h)), f"urmapx_index_open_device({path})")
        return cls(h.value)

    @classmethod
    def wrap_host(cls, word_length, max_ix, slot_count, blob, seqdata, seq_lengths, offsets, labels):
        sl = np.ascontiguousarray(seq_lengths, dtype=np.uint32)
        of = np.ascontiguousarray(offsets, dtype=np.uint32)
        lab = b"".join(l.encode() + b"\0" for l in labels)
        h = C.c_void_p()
        _check(lib().urmapx_index_wrap_host(word_length, max_ix, slot_count, blob.ctypes.data, seqdata.ctypes.data,
                                            len(seqdata), len(labels), sl.ctypes.data, of.ctypes.data, lab,
                                            C.byref(h)), "urmapx_index_wrap_host")
        return cls(h.value, keep=(blob, seqdata, sl, of, lab))

    @classmethod
    def wrap_device(cls, device, word_length, max_ix, slot_count, d_blob_ptr, d_seq_ptr, seqdata_size, seq_lengths,
                    offsets, labels, keep=()):
        """Adopt arrays already resident in HBM (raw device pointers, e.g. torch tensor .data_ptr())."""
        sl = np.ascontiguousarray(seq_lengths, dtype=np.uint32)
        of = np.ascontiguousarray(offsets, dtype=np.uint32)
        lab = b"".join(l.encode() + b"\0" for l in labels)
        h = C.c_void_p()
        _check(lib().urmapx_index_wrap_device(device, word_length, max_ix, slot_count, d_blob_ptr, d_seq_ptr,
                                              seqdata_size, len(labels), sl.ctypes.data, of.ctypes.data, lab,
                                              C.byref(h)), "urmapx_index_wrap_device")
        return cls(h.value, keep=tuple(keep) + (sl, of, lab))

    def upload(self, device=0):
        _check(lib().urmapx_index_upload(self.h, device), "urmapx_index_upload")
        return self

    def replicate(self, device):
        """Another replica of this index in the HBM of `device` (one per GPU; reads are sharded across them)."""
        h = C.c_void_p()
        _check(lib().urmapx_index_replicate(self.h, device, C.byref(h)), "urmapx_index_replicate")
        return Index(h.value, keep=(self,))

    def chain_row_bytes(self): return int(lib().urmapx_index_chain_row_bytes(self.h))

    def validate(self):
        """UFIndex::Validate (ufindex.cpp:611-658) as one device pass over the resident table -> (ok, report dict)."""
        r = ValidateReport()
        rc = lib().urmapx_index_validate(self.h, C.byref(r))
        if rc not in (0, E_FORMAT):
            raise UrmapxError(rc, "urmapx_index_validate")
        return rc == 0, {n: getattr(r, n) for n, _ in ValidateReport._fields_}

    def stats(self):
        """-ufi_stats (UFIndex::LogStats, ufistats.cpp) as two device passes over the resident table -> dict of every counter, the two
        256-bin histograms (count_hist, trunc_hist) and the passes' seconds.  A damaged row raises UrmapxError(E_FORMAT)."""
        r = UfiStats()
        _check(lib().urmapx_index_stats(self.h, C.byref(r)), "urmapx_index_stats")
        d = {n: int(getattr(r, n)) for n in STATS_FIELDS}
        d["count_hist"] = [int(x) for x in r.count_hist]
        d["trunc_hist"] = [int(x) for x in r.trunc_hist]
        d["position_seconds"], d["slot_seconds"] = r.position_seconds, r.slot_seconds
        return d

    def slot_counts(self, minus=False):
        """CountSlots (the bytes -ufi_counts writes) or, minus=True, CountSlots_Minus of the resident table: uint8 per slot"""
        out = np.empty(self.slot_count, dtype=np.uint8)
        _check(lib().urmapx_index_slot_counts(self.h, 1 if minus else 0, out.ctypes.data, out.size), "urmapx_index_slot_counts")
        return out

    def checksum(self):
        """(slot table, sequence store): urmapx_index_checksum over the resident arrays -- which table and which genome this is"""
        out = (C.c_uint64 * 2)()
        _check(lib().urmapx_index_checksum(self.h, out), "urmapx_index_checksum")
        return int(out[0]), int(out[1])

    def layout_checksum(self):
        """(slot16, chain rows): urmapx_index_layout_checksum -- the layouts derived from the table at upload (0: not built)"""
        out = (C.c_uint64 * 2)()
        _check(lib().urmapx_index_layout_checksum(self.h, out), "urmapx_index_layout_checksum")
        return int(out[0]), int(out[1])

    @property
    def word_length(self): return lib().urmapx_index_word_length(self.h)
    @property
    def max_ix(self): return lib().urmapx_index_max_ix(self.h)
    @property
    def slot_count(self): return lib().urmapx_index_slot_count(self.h)
    @property
    def seqdata_size(self): return lib().urmapx_index_seqdata_size(self.h)

    def directory(self):
        n = lib().urmapx_index_seq_count(self.h)
        return [(lib().urmapx_index_label(self.h, i).decode(), lib().urmapx_index_seq_length(self.h, i),
                 lib().urmapx_index_seq_offset(self.h, i)) for i in range(n)]

    def sam_header_sq(self) -> bytes:
        buf = C.create_string_buffer(1 << 20)
        n = lib().urmapx_sam_header_sq(self.h, buf, len(buf))
        return buf.raw[:n]

    def sam_se(self, results: np.ndarray, ops: np.ndarray, labels, bases: np.ndarray, offs: np.ndarray,
               quals: np.ndarray) -> bytes:
        """SAM records (State1::Output1 -> SetSAM) of a mapped batch, in input order.  Host-side text only."""
        results = np.ascontiguousarray(results)
        ops = np.ascontiguousarray(ops, dtype=np.uint16)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        out = []
        buf = C.create_string_buffer(1 << 16)
        ops_ptr = ops.ctypes.data if len(ops) else None
        for i in range(len(results)):
            o, e = int(offs[i]), int(offs[i + 1])
            n = lib().urmapx_sam_se(self.h, results[i:i + 1].ctypes.data, ops_ptr, labels[i].encode(),
                                    bases[o:e].ctypes.data, quals[o:e].ctypes.data, e - o, buf, len(buf))
            if n == 0:
                raise UrmapxError(-5, "urmapx_sam_se: record does not fit")
            out.append(buf.raw[:n])
        return b"".join(out)

    def bam_header(self, cmdline=None) -> bytes:
        """The uncompressed header block of a BAM file over this index (urmapx_bam_header): magic, the SAM header text, the references."""
        L = lib()
        L.urmapx_bam_header.restype = C.c_size_t
        L.urmapx_bam_header.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
        cl = cmdline.encode() if isinstance(cmdline, str) else cmdline
        n = L.urmapx_bam_header(self.h, cl, None, 0)
        buf = C.create_string_buffer(max(1, n))
        assert L.urmapx_bam_header(self.h, cl, buf, n) == n
        return buf.raw[:n]

    def _bam_call(self, fn_name, *args):
        fn = getattr(lib(), fn_name)
        fn.restype = C.c_size_t
        cap = 1 << 16
        while True:
            buf = C.create_string_buffer(cap)
            n = fn(*args, buf, C.c_size_t(cap))
            if n == C.c_size_t(-1).value:
                raise UrmapxError(-2, f"{fn_name}: a QNAME over 254 bytes does not fit a BAM record")
            if n:
                return buf.raw[:n]
            cap *= 4
            if cap > 1 << 28:
                raise UrmapxError(-5, f"{fn_name}: record does not fit")

    def bam_se(self, results: np.ndarray, ops: np.ndarray, labels, bases: np.ndarray, offs: np.ndarray,
               quals: np.ndarray) -> bytes:
        """BAM records (urmapx_bam_se) of a mapped batch, in input order: what sam_se prints, in the binary layout.  Host side only.
        UrmapxError naming the read for a QNAME over 254 bytes."""
        results = np.ascontiguousarray(results)
        ops = np.ascontiguousarray(ops, dtype=np.uint16)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        out = []
        ops_ptr = C.c_void_p(ops.ctypes.data if len(ops) else None)
        for i in range(len(results)):
            o, e = int(offs[i]), int(offs[i + 1])
            try:
                out.append(self._bam_call("urmapx_bam_se", self.h, C.c_void_p(results[i:i + 1].ctypes.data), ops_ptr, labels[i].encode("latin-1"),
                                          C.c_void_p(bases[o:e].ctypes.data), C.c_void_p(quals[o:e].ctypes.data), C.c_uint32(e - o)))
            except UrmapxError as x:
                raise UrmapxError(x.code, f"{x}: read {labels[i][:60]}...") if x.code == -2 else x
        return b"".join(out)

    def bam_pe(self, results: np.ndarray, ops: np.ndarray, labels, bases: np.ndarray, offs: np.ndarray,
               quals: np.ndarray) -> bytes:
        """BAM records of mapped PAIRS (reads 2i, 2i+1 = mates of pair i; urmapx_bam_pe): what sam_pe prints, in the binary layout."""
        results = np.ascontiguousarray(results)
        ops = np.ascontiguousarray(ops, dtype=np.uint16)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        out = []
        ops_ptr = C.c_void_p(ops.ctypes.data if len(ops) else None)
        for i in range(0, len(results), 2):
            o1, e1, e2 = int(offs[i]), int(offs[i + 1]), int(offs[i + 2])
            try:
                out.append(self._bam_call("urmapx_bam_pe", self.h, C.c_void_p(results[i:i + 1].ctypes.data), C.c_void_p(results[i + 1:i + 2].ctypes.data),
                                          ops_ptr, labels[i].encode("latin-1"), C.c_void_p(bases[o1:e1].ctypes.data), C.c_void_p(quals[o1:e1].ctypes.data),
                                          C.c_uint32(e1 - o1), labels[i + 1].encode("latin-1"), C.c_void_p(bases[e1:e2].ctypes.data),
                                          C.c_void_p(quals[e1:e2].ctypes.data), C.c_uint32(e2 - e1)))
            except UrmapxError as x:
                raise UrmapxError(x.code, f"{x}: pair {labels[i][:60]}...") if x.code == -2 else x
        return b"".join(out)

    def _tag_opts(self, tags, rg_id, refs):
        """urmapx_tag_options; refs: per mate bytes of the reference window or None (read from the host arrays).  -> (struct, keep-alive)"""
        keep = [np.frombuffer(r, dtype=np.uint8) if r is not None and len(r) else None for r in refs]
        to = TagOptions(int(tags), rg_id.encode("latin-1") if isinstance(rg_id, str) else rg_id,
                        (C.c_void_p * 2)(*[(k.ctypes.data if k is not None else None) for k in (keep + [None])[:2]]))
        return to, keep

    def records_tags(self, results, ops, labels, bases, offs, quals, tags=0, rg_id=None, bam=False, paired=False, windows=None) -> bytes:
        """SAM text or BAM records of a mapped batch with the optional fields NM MD AS RG (urmapx_sam_se_tags / _pe_tags / urmapx_bam_se_tags /
        _pe_tags).  tags = TAG_* bits, rg_id = the read group's ID or None.  windows: None (the reference bases come from this index's host
        arrays) or one bytes object per record (None for an unmapped one): the store bytes under it, as urmapx_index_fetch_spans gives them."""
        results = np.ascontiguousarray(results)
        ops = np.ascontiguousarray(ops, dtype=np.uint16)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        ops_ptr = C.c_void_p(ops.ctypes.data if len(ops) else None)
        name = ("urmapx_bam_" if bam else "urmapx_sam_") + ("pe_tags" if paired else "se_tags")
        out = []
        step = 2 if paired else 1
        enc = lambda l: l.encode("latin-1")
        for i in range(0, len(results), step):
            refs = [windows[i + k] for k in range(step)] if windows is not None else [None] * step
            to, keep = self._tag_opts(tags, rg_id, refs)
            o, e = int(offs[i]), int(offs[i + 1])
            args = [self.h, C.c_void_p(results[i:i + 1].ctypes.data)]
            if paired:
                e2 = int(offs[i + 2])
                args += [C.c_void_p(results[i + 1:i + 2].ctypes.data), ops_ptr, enc(labels[i]), C.c_void_p(bases[o:e].ctypes.data),
                         C.c_void_p(quals[o:e].ctypes.data), C.c_uint32(e - o), enc(labels[i + 1]), C.c_void_p(bases[e:e2].ctypes.data),
                         C.c_void_p(quals[e:e2].ctypes.data), C.c_uint32(e2 - e)]
            else:
                args += [ops_ptr, enc(labels[i]), C.c_void_p(bases[o:e].ctypes.data), C.c_void_p(quals[o:e].ctypes.data), C.c_uint32(e - o)]
            out.append(self._bam_call(name, *args, C.byref(to)))
            del keep
        return b"".join(out)

    def header_rg(self, cmdline=None, read_group=None, sorted=False, bam=False) -> bytes:
        """The SAM header text or (bam) the BAM header block with read_group (an @RG line, tabs real) in front of the @PG line
        (urmapx_sam_header_rg / urmapx_bam_header_rg); sorted: the @HD line of -sort first."""
        fn = getattr(lib(), "urmapx_bam_header_rg" if bam else "urmapx_sam_header_rg")
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]
        cl = cmdline.encode() if isinstance(cmdline, str) else cmdline
        rg = read_group.encode("latin-1") if isinstance(read_group, str) else read_group
        n = fn(self.h, cl, rg, int(bool(sorted)), None, 0)
        buf = C.create_string_buffer(max(1, n))
        assert fn(self.h, cl, rg, int(bool(sorted)), buf, n) == n
        return buf.raw[:n]

    def fetch_spans(self, starts, lens):
        """The store bytes under spans (start, length) (urmapx_index_fetch_spans): from the host arrays, else one gather on the device
        and one copy.  -> list of bytes"""
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        out = np.zeros(max(1, int(ln.sum())), dtype=np.uint8)
        L = lib()
        L.urmapx_index_fetch_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        _check(L.urmapx_index_fetch_spans(self.h, st.ctypes.data, ln.ctypes.data, len(st), out.ctypes.data), "urmapx_index_fetch_spans")
        cuts = np.concatenate([[0], np.cumsum(ln.astype(np.int64))])
        return [out[int(cuts[i]):int(cuts[i + 1])].tobytes() for i in range(len(st))]

    def tab_pe(self, res, info, labels, offs, sam_on=True):
        """-tabbedout lines (State2::OutputTab2) for pairs interleaved as in map_pe; labels = per read."""
        L = lib()
        out = []
        buf = C.create_string_buffer(4096)
        res = np.ascontiguousarray(res)
        info = np.ascontiguousarray(info)
        for i in range(len(info)):
            l1 = int(offs[2 * i + 1] - offs[2 * i]); l2 = int(offs[2 * i + 2] - offs[2 * i + 1])
            k = L.urmapx_tab_pe(self.h, res[2 * i:].ctypes.data, res[2 * i + 1:].ctypes.data, info[i:].ctypes.data,
                                labels[2 * i].encode("latin-1"), l1, l2, int(sam_on), buf, len(buf))
            out.append(buf.raw[:k])
        return b"".join(out)

    def sam_pe(self, results: np.ndarray, ops: np.ndarray, labels, bases: np.ndarray, offs: np.ndarray,
               quals: np.ndarray) -> bytes:
        """SAM records of mapped PAIRS (reads 2i, 2i+1 = mates of pair i): State2::SetSAM2 + SetSAM."""
        results = np.ascontiguousarray(results)
        ops = np.ascontiguousarray(ops, dtype=np.uint16)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        out = []
        buf = C.create_string_buffer(1 << 16)
        ops_ptr = ops.ctypes.data if len(ops) else None
        for i in range(0, len(results), 2):
            o1, e1, e2 = int(offs[i]), int(offs[i + 1]), int(offs[i + 2])
            n = lib().urmapx_sam_pe(self.h, results[i:i + 1].ctypes.data, results[i + 1:i + 2].ctypes.data, ops_ptr,
                                    labels[i].encode(), bases[o1:e1].ctypes.data, quals[o1:e1].ctypes.data, e1 - o1,
                                    labels[i + 1].encode(), bases[e1:e2].ctypes.data, quals[e1:e2].ctypes.data, e2 - e1,
                                    buf, len(buf))
            if n == 0:
                raise UrmapxError(-5, "urmapx_sam_pe: record does not fit")
            out.append(buf.raw[:n])
        return b"".join(out)

    def close(self):
        if self.h:
            lib().urmapx_index_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ufi_info(path):
    """-ufi_info: the header of a .ufi file (host only; the index is not loaded) -> dict"""
    w, m, sd, sc = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    _check(lib().urmapx_ufi_info(os.fsencode(path), C.byref(w), C.byref(m), C.byref(sd), C.byref(sc)), "urmapx_ufi_info")
    return {"word_length": w.value, "max_ix": m.value, "seqdata_size": sd.value, "slots": sc.value}


def gunzip_file(gz_path, out_path, threads=0):
    """the .gz reader of urmapx_map_files alone (pgzip.h) -> (bytes written, by the parallel road, through zlib)"""
    L = lib()
    L.urmapx_gunzip_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64 * 3)]
    st = (C.c_uint64 * 3)()
    _check(L.urmapx_gunzip_file(os.fsencode(gz_path), os.fsencode(out_path), threads, C.byref(st)), f"urmapx_gunzip_file({gz_path})")
    return int(st[0]), int(st[1]), int(st[2])


def map_files(index: "Index", fastq1, fastq2=None, samout=None, tabout=None, first_gpu=0, gpus=1, streams=2, host_threads=0,
              batch=0, veryfast=False, minq=10, cmdline=None, allow_unsupported=False, sam_shards=0, discard_sam=False, bgzf=False, bam=False,
              bam_sort=False, tags=0, read_group=None, markdup=False, sort_mem=0, depth_out=None, depth_mapq=0,
              stats_out=None, vcf_out=None, vcf_mapq=0, vcf_baseq=13, vcf_min_alt=3, vcf_min_pct=10):
    """urmap -map / -map2 file to file (cmd_map / cmd_map2) on an index that has its host arrays or is resident on
    first_gpu.  bgzf: samout is a BGZF file (-bgzf).  bam: samout is a BAM file (-bamout).  bam_sort (with bam):
    its records in coordinate order, with the index samout + ".bai" beside it (-sort).  tags: TAG_* bits (-tags), read_group: an @RG line
    with real tabs (-rg): the optional fields of the records.  markdup (with bam_sort): flag 0x400 on duplicate records (-markdup),
    the counters in the report.  sort_mem (with bam_sort): the device bytes the sort may take (-sortmem); records that do not fit them
    stream through the device, and the report's sort_partitions says in how many partitions.  depth_out (with bam_sort): a bedGraph
    file of the per-base depth of the records as written (-depth), depth_mapq: its least MAPQ (-depth_mapq); the report then holds
    depth_s, depth_runs, depth_covered, depth_bases and, as depth_summary, the table per reference.  stats_out (with bam_sort): a text
    file of the alignment statistics of the records as written (-stats); the report then holds stats_s and a few totals.  vcf_out (with
    bam_sort): a sites-only VCF file of the columns where the records as written differ from the index's sequences (-vcfout; include/urmapx.h
    "Pileup"), vcf_mapq, vcf_baseq, vcf_min_alt, vcf_min_pct: its thresholds; the report then holds pileup_s, pileup_sites, pileup_records
    and pileup_alt_alleles.  -> dict of State1::HitStats' counters and stage times."""
    o = MapOptionsPileup(first_gpu, gpus, streams, host_threads, batch, int(veryfast), minq, cmdline.encode() if cmdline else None,
                   int(sam_shards), int(discard_sam), int(bgzf), int(bam), int(bam_sort), int(tags),
                   (read_group.encode("latin-1") if isinstance(read_group, str) else read_group), int(markdup), int(sort_mem),
                   os.fsencode(depth_out) if depth_out else None, int(depth_mapq), os.fsencode(stats_out) if stats_out is not None else None,
                   os.fsencode(vcf_out) if vcf_out is not None else None, int(vcf_mapq), int(vcf_baseq), int(vcf_min_alt), int(vcf_min_pct))
    rep = MapReportPileup()
    err = C.create_string_buffer(1024)
    enc = lambda p: os.fsencode(p) if p else None
    rc = lib().urmapx_map_files(index.h, C.byref(o), enc(fastq1), enc(fastq2), enc(samout), enc(tabout), C.byref(rep), err, len(err))
    if rc != 0 and not (rc == E_UNSUPPORTED and allow_unsupported):
        raise UrmapxError(rc, "urmapx_map_files: " + err.value.decode("latin-1"))
    out = {k: getattr(rep, k) for k, _ in MapReportPileup._fields_}
    if depth_out:
        out["depth_summary"] = lib().urmapx_map_depth_summary().decode("latin-1")
    return out


def calmd(ref: bytes, cigar, seq: bytes):
    """NM and MD of one alignment (urmapx_calmd; host only): ref = the reference window, cigar = [(length, 'M' | 'I' | 'D')], seq = SEQ as
    printed.  -> (NM, MD text); ValueError if the runs leave the window or the read."""
    L = lib()
    L.urmapx_calmd.restype = C.c_size_t
    L.urmapx_calmd.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
    runs = np.array([(int(n) << 4) | "MID".index(op) for n, op in cigar], dtype=np.uint32)
    nm = C.c_uint32(0)
    n = L.urmapx_calmd(ref, len(ref), runs.ctypes.data, len(runs), seq, len(seq), C.byref(nm), None, 0)
    if n == C.c_size_t(-1).value:
        raise ValueError("urmapx_calmd: the CIGAR leaves the reference window or the read")
    buf = C.create_string_buffer(max(1, n))
    assert L.urmapx_calmd(ref, len(ref), runs.ctypes.data, len(runs), seq, len(seq), C.byref(nm), buf, n) == n
    return int(nm.value), buf.raw[:n].decode()


def ref_span(result: np.ndarray, ops: np.ndarray, read_len):
    """reference bases under the emitted CIGAR of one result (urmapx_ref_span); 0: unmapped"""
    L = lib()
    L.urmapx_ref_span.restype = C.c_uint32
    L.urmapx_ref_span.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    ops = np.ascontiguousarray(ops, dtype=np.uint16)
    r = np.ascontiguousarray(result)
    return int(L.urmapx_ref_span(r.ctypes.data, ops.ctypes.data if len(ops) else None, int(read_len)))


def read_group_id(line):
    """-rg LINE as the command line takes it (urmapx_read_group_id): -> (the line with real tabs, its ID); ValueError with the refusal"""
    L = lib()
    L.urmapx_read_group_id.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    raw = line.encode("latin-1") if isinstance(line, str) else line
    out, ident, err = C.create_string_buffer(len(raw) + 8), C.create_string_buffer(len(raw) + 8), C.create_string_buffer(1024)
    if L.urmapx_read_group_id(raw, out, len(out), ident, len(ident), err, len(err)) != 0:
        raise ValueError(err.value.decode("latin-1"))
    return out.value.decode("latin-1"), ident.value.decode("latin-1")


def _depth_refs(n_ref, names, lens):
    """the names and lengths of n_ref references as the depth calls take them -> (char ** array, uint32 array)"""
    names = [n.encode("latin-1") if isinstance(n, str) else bytes(n) for n in names]
    if len(names) != int(n_ref) or len(lens) != int(n_ref):
        raise ValueError("n_ref names and lengths are needed")
    return (C.c_char_p * max(1, len(names)))(*names), np.ascontiguousarray(lens, dtype=np.uint32)


def _depth_out(res, report):
    """(text, runs, summaries[, report]) of a filled DepthResult; summaries: one dict of reads, covered, bases, mapq_sum per reference"""
    text = C.string_at(res.text, res.text_bytes) if res.text_bytes else b""
    refs = [{k: int(getattr(res.refs[r], k)) for k, _ in DepthSummary._fields_} for r in range(res.n_ref)]
    out = (text, int(res.runs), refs)
    return out + ({k: getattr(res, k) for k, _ in DepthResult._fields_ if k not in ("text", "refs")},) if report else out


def _bam_depth(fn_name, head, records, n_ref, names, lens, min_mapq, report, starts):
    src = np.frombuffer(bytes(records), dtype=np.uint8)
    L = lib()
    fn = getattr(L, fn_name)
    fn.argtypes = ([C.c_int] * len(head) + [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.POINTER(DepthOpts), C.POINTER(DepthResult)])
    L.urmapx_depth_free.argtypes = [C.POINTER(DepthResult)]
    L.urmapx_depth_free.restype = None
    nm, ln = _depth_refs(n_ref, names, lens)
    st = np.ascontiguousarray(starts if starts is not None else [], dtype=np.uint64)
    res, opts = DepthResult(), DepthOpts(int(min_mapq))
    _check(fn(*head, src.ctypes.data if len(src) else None, len(src), int(n_ref), nm, ln.ctypes.data if len(ln) else None,
              st.ctypes.data if len(st) else None, len(st), C.byref(opts), C.byref(res)), fn_name)
    try:
        return _depth_out(res, report)
    finally:
        L.urmapx_depth_free(C.byref(res))


def bam_depth(records: bytes, n_ref, names, lens, device=0, min_mapq=0, report=False, starts=None):
    """BAM alignment records back to back, in any order, and the references' names and lengths -> (the bedGraph text of the per-base
    depth, its number of lines, one dict of reads / covered / bases / mapq_sum per reference), computed on the device
    (urmapx_bam_depth; depth.hip; the rule is in include/urmapx.h "Depth").  min_mapq: records below it do not count.  report: a
    fourth item, the call's counters and step times."""
    return _bam_depth("urmapx_bam_depth", (int(device),), records, n_ref, names, lens, min_mapq, report, starts)


def bam_depth_host(records: bytes, n_ref, names, lens, min_mapq=0, report=False, starts=None):
    """the same contract on the host, no device (urmapx_bam_depth_host; depth_host.cpp)"""
    return _bam_depth("urmapx_bam_depth_host", (), records, n_ref, names, lens, min_mapq, report, starts)


def bam_depth_device_bytes(total_columns, n_ref, n_records):
    """device bytes urmapx_bam_depth takes (host arithmetic)"""
    L = lib()
    L.urmapx_bam_depth_device_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64]
    L.urmapx_bam_depth_device_bytes.restype = C.c_uint64
    return int(L.urmapx_bam_depth_device_bytes(int(total_columns), int(n_ref), int(n_records)))


def bam_depth_resident_bytes(total_columns, n_ref):
    """device bytes the depth adds to the planned sort (host arithmetic)"""
    L = lib()
    L.urmapx_bam_depth_resident_bytes.argtypes = [C.c_uint64, C.c_uint32]
    L.urmapx_bam_depth_resident_bytes.restype = C.c_uint64
    return int(L.urmapx_bam_depth_resident_bytes(int(total_columns), int(n_ref)))


def _bam_stats(fn_name, head, records, n_ref, names, lens, command, report, starts):
    src = np.frombuffer(bytes(records), dtype=np.uint8)
    L = lib()
    fn = getattr(L, fn_name)
    fn.argtypes = ([C.c_int] * len(head) + [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_char_p, C.POINTER(StatsResult)])
    L.urmapx_stats_free.argtypes = [C.POINTER(StatsResult)]
    L.urmapx_stats_free.restype = None
    nm, ln = _depth_refs(n_ref, names, lens)
    st = np.ascontiguousarray(starts if starts is not None else [], dtype=np.uint64)
    res = StatsResult()
    cmd = command.encode("latin-1") if isinstance(command, str) else command
    _check(fn(*head, src.ctypes.data if len(src) else None, len(src), int(n_ref), nm, ln.ctypes.data if len(ln) else None,
              st.ctypes.data if len(st) else None, len(st), cmd, C.byref(res)), fn_name)
    try:
        text = C.string_at(res.text, res.text_bytes) if res.text_bytes else b""
        return (text, {k: getattr(res, k) for k, _ in StatsResult._fields_ if k != "text"}) if report else text
    finally:
        L.urmapx_stats_free(C.byref(res))


def bam_stats(records: bytes, n_ref, names, lens, device=0, command=None, report=False, starts=None):
    """BAM alignment records back to back, in any order, and the references' names and lengths -> the text of their alignment
    statistics (include/urmapx.h "Stats"), counted on the device (urmapx_bam_stats; stats.hip).  command: the text of the second
    line.  report: (text, the call's totals and step times)."""
    return _bam_stats("urmapx_bam_stats", (int(device),), records, n_ref, names, lens, command, report, starts)


def bam_stats_host(records: bytes, n_ref, names, lens, command=None, report=False, starts=None):
    """the same contract on the host, no device (urmapx_bam_stats_host; stats_host.cpp)"""
    return _bam_stats("urmapx_bam_stats_host", (), records, n_ref, names, lens, command, report, starts)


def bam_stats_resident_bytes(n_ref):
    """device bytes the statistics add to the planned sort (host arithmetic)"""
    L = lib()
    L.urmapx_bam_stats_resident_bytes.argtypes = [C.c_uint32]
    L.urmapx_bam_stats_resident_bytes.restype = C.c_uint64
    return int(L.urmapx_bam_stats_resident_bytes(int(n_ref)))


def _pileup_opts(opts):
    """None (the library's defaults), a dict of min_mapq / min_baseq / min_alt / min_pct (those left out: 0, 13, 3, 10) or the four numbers"""
    if opts is None:
        return None
    if isinstance(opts, dict):
        opts = (opts.get("min_mapq", 0), opts.get("min_baseq", 13), opts.get("min_alt", 3), opts.get("min_pct", 10))
    return PileupOpts(*[int(v) for v in opts])


def _pileup_seqs(n_ref, seqs):
    """one bytes object per reference -> char ** array (the caller keeps it alive over the call)"""
    seqs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    if len(seqs) != int(n_ref):
        raise ValueError("a sequence per reference is needed")
    return (C.c_char_p * max(1, len(seqs)))(*seqs)


def _bam_pileup(fn_name, head, records, n_ref, names, lens, seqs, opts, command, report, starts):
    src = np.frombuffer(bytes(records), dtype=np.uint8)
    L = lib()
    fn = getattr(L, fn_name)
    fn.argtypes = ([C.c_int] * len(head) + [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(C.c_char_p), C.c_void_p, C.c_size_t,
                                            C.POINTER(PileupOpts), C.c_char_p, C.POINTER(PileupResult)])
    L.urmapx_pileup_free.argtypes = [C.POINTER(PileupResult)]
    L.urmapx_pileup_free.restype = None
    nm, ln = _depth_refs(n_ref, names, lens)
    sq = _pileup_seqs(n_ref, seqs)
    st = np.ascontiguousarray(starts if starts is not None else [], dtype=np.uint64)
    res, po = PileupResult(), _pileup_opts(opts)
    cmd = command.encode("latin-1") if isinstance(command, str) else command
    _check(fn(*head, src.ctypes.data if len(src) else None, len(src), int(n_ref), nm, ln.ctypes.data if len(ln) else None, sq,
              st.ctypes.data if len(st) else None, len(st), C.byref(po) if po is not None else None, cmd, C.byref(res)), fn_name)
    try:
        text = C.string_at(res.text, res.text_bytes) if res.text_bytes else b""
        return (text, {k: getattr(res, k) for k, _ in PileupResult._fields_ if k != "text"}) if report else text
    finally:
        L.urmapx_pileup_free(C.byref(res))


def bam_pileup(records: bytes, n_ref, names, lens, seqs, opts=None, device=0, command=None, report=False, starts=None):
    """BAM alignment records back to back, in any order, the references' names and lengths and their bases (one bytes object of ASCII
    letters per reference) -> the sites-only VCF text of the columns where the reads show a base other than the reference's
    (include/urmapx.h "Pileup"), piled up on the device (urmapx_bam_pileup; pileup.hip).  opts: None for the defaults, or a dict of
    min_mapq, min_baseq, min_alt, min_pct.  command: the text of the ##urmapCommand line.  report: (text, the call's totals and times)."""
    return _bam_pileup("urmapx_bam_pileup", (int(device),), records, n_ref, names, lens, seqs, opts, command, report, starts)


def bam_pileup_host(records: bytes, n_ref, names, lens, seqs, opts=None, command=None, report=False, starts=None):
    """the same contract on the host, no device (urmapx_bam_pileup_host; pileup_host.cpp)"""
    return _bam_pileup("urmapx_bam_pileup_host", (), records, n_ref, names, lens, seqs, opts, command, report, starts)


def bam_pileup_resident_bytes(total_columns, n_ref, seq_resident=False):
    """device bytes the pileup adds to the planned sort (host arithmetic); seq_resident: the bases are an index's resident store"""
    L = lib()
    L.urmapx_bam_pileup_resident_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_int]
    L.urmapx_bam_pileup_resident_bytes.restype = C.c_uint64
    return int(L.urmapx_bam_pileup_resident_bytes(int(total_columns), int(n_ref), int(seq_resident)))


def bam_pileup_device_bytes(total_columns, n_ref, n_records):
    """device bytes urmapx_bam_pileup takes (host arithmetic)"""
    L = lib()
    L.urmapx_bam_pileup_device_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64]
    L.urmapx_bam_pileup_device_bytes.restype = C.c_uint64
    return int(L.urmapx_bam_pileup_device_bytes(int(total_columns), int(n_ref), int(n_records)))


def _bam_sort_with(fn_name, head, records, n_ref, in_front, report, starts, markdup, depth, depth_mapq, stats, pileup):
    """the planned sort with the depth, the statistics and the pileup, each or none, taken on the way (urmapx_bam_sort_with,
    urmapx_bam_sort_with_host) -> (members, bai[, depth result][, stats text][, VCF text][, report]); the depth result is (text, runs,
    summaries), and the report holds the results' fields as depth_*, stats_* and pileup_*.  depth, stats: (names, lens).  pileup:
    (names, lens, seqs, opts); seqs may be an Index, whose sequence store then gives the bases"""
    src = np.frombuffer(bytes(records), dtype=np.uint8)
    L = lib()
    fn = getattr(L, fn_name)
    fn.argtypes = ([C.c_int, C.c_uint64][:len(head)] + [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(BamSortExtras),
                                                       C.POINTER(BamSortResult)])
    for free, kind in (("urmapx_bam_sort_free", BamSortResult), ("urmapx_depth_free", DepthResult), ("urmapx_stats_free", StatsResult),
                       ("urmapx_pileup_free", PileupResult)):
        getattr(L, free).argtypes = [C.POINTER(kind)]
        getattr(L, free).restype = None
    nm, ln = _depth_refs(n_ref, *(pileup if pileup is not None else depth if depth is not None else stats)[:2])
    sq = index = po = None
    if pileup is not None:
        index = pileup[2].h if isinstance(pileup[2], Index) else None
        sq = None if index is not None else _pileup_seqs(n_ref, pileup[2])
        po = _pileup_opts(pileup[3])
    st = np.ascontiguousarray(starts if starts is not None else [], dtype=np.uint64)
    res, md, dres, sres, pres, opts = BamSortResult(), MarkdupStats(), DepthResult(), StatsResult(), PileupResult(), DepthOpts(int(depth_mapq))
    ex = BamSortExtras(C.pointer(md) if markdup else None, C.pointer(opts), nm, ln.ctypes.data if len(ln) else None,
                       C.pointer(dres) if depth is not None else None, C.pointer(sres) if stats is not None else None, None,
                       C.pointer(po) if po is not None else None, sq, index, C.pointer(pres) if pileup is not None else None, None)
    rc = fn(*head, src.ctypes.data if len(src) else None, len(src), int(n_ref), int(in_front), st.ctypes.data if len(st) else None, len(st),
            C.byref(ex), C.byref(res))
    if rc != 0:
        least = int(pres.least_budget or sres.least_budget or dres.least_budget)
        e = UrmapxError(rc, fn_name + (": %d bytes are needed at the least" % least if least else ""))
        e.least_budget = least
        raise e
    try:
        out = (C.string_at(res.bgzf, res.bgzf_bytes) if res.bgzf_bytes else b"", C.string_at(res.bai, res.bai_bytes))
        rep = {k: getattr(res, k) for k, _ in BamSortResult._fields_ if k not in ("bgzf", "bai")}
        if markdup:
            rep.update({k: getattr(md, k) for k, _ in MarkdupStats._fields_})
        if depth is not None:
            out += (_depth_out(dres, False),)
            rep.update({"depth_" + k: getattr(dres, k) for k, _ in DepthResult._fields_ if k not in ("text", "refs")})
        if stats is not None:
            out += (C.string_at(sres.text, sres.text_bytes) if sres.text_bytes else b"",)
            rep.update({"stats_" + k: getattr(sres, k) for k, _ in StatsResult._fields_ if k != "text"})
        if pileup is not None:
            out += (C.string_at(pres.text, pres.text_bytes) if pres.text_bytes else b"",)
            rep.update({"pileup_" + k: getattr(pres, k) for k, _ in PileupResult._fields_ if k != "text"})
    finally:
        L.urmapx_bam_sort_free(C.byref(res))
        L.urmapx_depth_free(C.byref(dres))
        L.urmapx_stats_free(C.byref(sres))
        L.urmapx_pileup_free(C.byref(pres))
    return out + (rep,) if report else out


def _bam_sort(fn_name, head, records, n_ref, in_front, report, starts=None, markdup=False, budget=None):
    src = np.frombuffer(bytes(records), dtype=np.uint8)
    res = BamSortResult()
    md = MarkdupStats()
    L = lib()
    if budget is not None:  # the planned call: one entry with or without marking (md NULL), the budget behind the device
        fn_name, head = "urmapx_bam_sort_external", head + (int(budget),)
    elif markdup:
        fn_name = fn_name.replace("urmapx_bam_sort", "urmapx_bam_sort_markdup")
    fn = getattr(L, fn_name)
    fn.argtypes = ([C.c_int] * (len(head) - (budget is not None)) + [C.c_uint64] * (budget is not None) +
                   [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t] +
                   ([C.POINTER(MarkdupStats)] if markdup or budget is not None else []) + [C.POINTER(BamSortResult)])
    L.urmapx_bam_sort_free.argtypes = [C.POINTER(BamSortResult)]
    L.urmapx_bam_sort_free.restype = None
    st = np.ascontiguousarray(starts if starts is not None else [], dtype=np.uint64)
    tail = (C.byref(md), C.byref(res)) if markdup else (None, C.byref(res)) if budget is not None else (C.byref(res),)
    _check(fn(*head, src.ctypes.data if len(src) else None, len(src), int(n_ref), int(in_front), st.ctypes.data if len(st) else None, len(st),
              *tail), fn_name)
    try:
        out = (C.string_at(res.bgzf, res.bgzf_bytes) if res.bgzf_bytes else b"", C.string_at(res.bai, res.bai_bytes))
        rep = {k: getattr(res, k) for k, _ in BamSortResult._fields_ if k not in ("bgzf", "bai")}
        if markdup:
            rep.update({k: getattr(md, k) for k, _ in MarkdupStats._fields_})
    finally:
        L.urmapx_bam_sort_free(C.byref(res))
    return out + (rep,) if report else out


def bam_sort_plan(n_bytes, n_records, budget, markdup=False):
    """the road urmapx_bam_sort_external takes for `budget` device bytes (urmapx_bam_sort_plan_for; host arithmetic, no device) -> dict of
    external, partition_bytes, partitions, stage_bytes, device_bytes.  UrmapxError (E_NOMEM) where not even one slice fits: its `plan`
    attribute is the dict, device_bytes the least budget that does."""
    L = lib()
    L.urmapx_bam_sort_plan_for.argtypes = [C.c_size_t, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(BamSortPlan)]
    p = BamSortPlan()
    rc = L.urmapx_bam_sort_plan_for(int(n_bytes), int(n_records), int(markdup), int(budget), C.byref(p))
    plan = {k: int(getattr(p, k)) for k, _ in BamSortPlan._fields_}
    if rc != 0:
        e = UrmapxError(rc, "urmapx_bam_sort_plan_for: %d bytes are needed at the least" % plan["device_bytes"])
        e.plan = plan
        raise e
    return plan


def bam_sort(records: bytes, n_ref, device=0, bytes_in_front=0, report=False, starts=None, markdup=False, budget=None, depth=None, depth_mapq=0,
             stats=None, pileup=None):
    """BAM alignment records back to back -> (the records in coordinate order as BGZF members, the bytes of their .bai index), sorted on
    the device (urmapx_bam_sort; bam_sort.hip).  bytes_in_front: what the file holds in front of the first member, for the index's
    virtual offsets.  report: a third item, the call's counters and step times.  starts: offsets at which records are known to begin (the
    chain is then walked from all of them at once).  markdup: flag 0x400 of the records says whether they are duplicates
    (urmapx_bam_sort_markdup; markdup.hip), and the report holds the counters and markdup_s.  budget: device bytes the sort may take
    (0: what is free): the call is urmapx_bam_sort_external, which streams the records through the device where they do not fit the
    budget; the report's external, partitions, stage_chunks and stage_s say what it did.  depth=(names, lens) of the n_ref references:
    the call is urmapx_bam_sort_with (budget None: 0), the per-base depth of the records as written -- under markdup without the
    duplicates -- is taken while they are on the device, and a third item (text, runs, summaries) comes back, as from bam_depth;
    depth_mapq: its least MAPQ.  stats=(names, lens): urmapx_bam_sort_with too, the alignment statistics of the records as
    written are counted where the depth is taken, and their text comes back as one more item behind the depth's (as from bam_stats).
    pileup=(names, lens, seqs, opts): urmapx_bam_sort_with too, the SNV candidate sites of the records as written are piled up
    there too, and their VCF text comes back as the last item in front of the report (as from bam_pileup); seqs: a bytes object per
    reference, or an Index, whose sequence store then gives the bases."""
    if depth is not None or stats is not None or pileup is not None:
        return _bam_sort_with("urmapx_bam_sort_with", (int(device), int(budget or 0)), records, n_ref, bytes_in_front, report, starts, markdup, depth,
                              depth_mapq, stats, pileup)
    return _bam_sort("urmapx_bam_sort", (int(device),), records, n_ref, bytes_in_front, report, starts, markdup, budget)


def bam_sort_host(records: bytes, n_ref, bytes_in_front=0, report=False, starts=None, markdup=False, depth=None, depth_mapq=0, stats=None, pileup=None):
    """the same contract on the host, no device (urmapx_bam_sort_host, urmapx_bam_sort_markdup_host): std::stable_sort and zlib inside
    the BGZF framing.  depth, stats, pileup: as for bam_sort (urmapx_bam_sort_with_host)"""
    if depth is not None or stats is not None or pileup is not None:
        return _bam_sort_with("urmapx_bam_sort_with_host", (), records, n_ref, bytes_in_front, report, starts, markdup, depth, depth_mapq, stats, pileup)
    return _bam_sort("urmapx_bam_sort_host", (), records, n_ref, bytes_in_front, report, starts, markdup)


BGZF_PIECE = 65280
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_bound(n):
    """the most n bytes of text can become as BGZF, end-of-file member included"""
    L = lib()
    L.urmapx_bgzf_bound.restype = C.c_size_t
    L.urmapx_bgzf_bound.argtypes = [C.c_size_t]
    return int(L.urmapx_bgzf_bound(int(n)))


def _bgzf(fn_name, head, data, eof, cap, tail=()):
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = bgzf_bound(len(src)) if cap is None else int(cap)
    out = np.empty(max(1, cap), dtype=np.uint8)
    used = C.c_size_t()
    fn = getattr(lib(), fn_name)
    fn.argtypes = [C.c_int] * len(head) + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_int] + [C.c_void_p] * len(tail)
    _check(fn(*head, src.ctypes.data if len(src) else None, len(src), out.ctypes.data, cap, C.byref(used), int(bool(eof)), *tail), fn_name)
    return out[: used.value].tobytes()


def bgzf_compress_host(data, eof=True, cap=None):
    """bytes -> BGZF (zlib inside the framing, on the host, no device)"""
    return _bgzf("urmapx_bgzf_compress_host", (), data, eof, cap)


def bgzf_compress(data, device=0, eof=True, cap=None):
    """bytes -> BGZF, deflated on the device (bgzf_gpu.hip)"""
    return _bgzf("urmapx_bgzf_compress", (int(device),), data, eof, cap)


def bgzf_compress_timed(data, device=0, eof=True):
    """-> (BGZF bytes, ms of the compress launches alone, by events)"""
    ms = C.c_float()
    out = _bgzf("urmapx_bgzf_compress_timed", (int(device),), data, eof, None, (C.cast(C.byref(ms), C.c_void_p),))
    return out, float(ms.value)


def bgzf_code_lengths(counts, maxbits, force2=False, device=0):
    """symbol counts -> code lengths of at most maxbits bits, by the device compressor's own stage (huff_lengths of bgzf_gpu.hip)"""
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    out = np.zeros(max(1, len(cnt)), dtype=np.uint8)
    fn = lib().urmapx_bgzf_code_lengths
    fn.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    _check(fn(int(device), cnt.ctypes.data if len(cnt) else None, len(cnt), int(maxbits), int(bool(force2)), out.ctypes.data), "urmapx_bgzf_code_lengths")
    return out[: len(cnt)]


def _seq_arrays(seqs):
    """list of byte strings / uint8 arrays, or (bases, offs) already concatenated -> (uint8 bases, uint64 offs)"""
    if isinstance(seqs, tuple) and len(seqs) == 2 and isinstance(seqs[1], np.ndarray):
        return np.ascontiguousarray(seqs[0], dtype=np.uint8), np.ascontiguousarray(seqs[1], dtype=np.uint64)
    arrs = [np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else x.astype(np.uint8) for x in seqs]
    offs = np.zeros(len(arrs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(a) for a in arrs])
    bases = np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)
    return np.ascontiguousarray(bases, dtype=np.uint8), offs


class BitVec:
    """The k-mer bit vector of -make_bitvec / -search_bitvec (4^W bits in the HBM of one device)."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)

    @classmethod
    def build(cls, device, seqs, excl=(), word_length=16):
        """Set the words of `seqs` (both strands), then clear those of `excl`.  Each: a list of byte strings or (bases, offs).
        -> (BitVec, (words included, words excluded))"""
        b, o = _seq_arrays(seqs)
        eb, eo = _seq_arrays(excl)
        h, cnt = C.c_void_p(), (C.c_uint64 * 2)()
        _check(lib().urmapx_bitvec_build(int(device), b.ctypes.data, o.ctypes.data, len(o) - 1, eb.ctypes.data, eo.ctypes.data, len(eo) - 1,
                                         int(word_length), C.byref(h), C.byref(cnt)), "urmapx_bitvec_build")
        return cls(h.value), (int(cnt[0]), int(cnt[1]))

    @classmethod
    def open(cls, path, device=0):
        h = C.c_void_p()
        _check(lib().urmapx_bitvec_open(os.fsencode(path), int(device), C.byref(h)), f"urmapx_bitvec_open({path})")
        return cls(h.value)

    @classmethod
    def wrap_host(cls, word_length, bits: np.ndarray, device=0):
        """Copy 4^W/8 bytes of bits (the .bv layout) to `device`."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        if len(bits) < (1 << (2 * word_length)) // 8:
            raise ValueError("bits: fewer than 4^W/8 bytes")
        h = C.c_void_p()
        _check(lib().urmapx_bitvec_wrap_host(int(device), int(word_length), bits.ctypes.data, C.byref(h)), "urmapx_bitvec_wrap_host")
        return cls(h.value)

    @property
    def word_length(self): return int(lib().urmapx_bitvec_word_length(self.h))

    @property
    def nbytes(self): return int(lib().urmapx_bitvec_bytes(self.h))

    def save(self, path):
        _check(lib().urmapx_bitvec_save(self.h, os.fsencode(path)), f"urmapx_bitvec_save({path})")

    def download(self) -> np.ndarray:
        out = np.empty(self.nbytes, dtype=np.uint8)
        _check(lib().urmapx_bitvec_download(self.h, out.ctypes.data, len(out)), "urmapx_bitvec_download")
        return out

    def popcount(self):
        out = C.c_uint64(0)
        _check(lib().urmapx_bitvec_popcount(self.h, C.byref(out)), "urmapx_bitvec_popcount")
        return int(out.value)

    def search(self, bases: np.ndarray, offs: np.ndarray) -> np.ndarray:
        """-> uint8 verdict per read: 0 not found, 1 forward, 2 reverse"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        out = np.zeros(len(offs) - 1, dtype=np.uint8)
        _check(lib().urmapx_bitvec_search(self.h, bases.ctypes.data, offs.ctypes.data, len(out), out.ctypes.data), "urmapx_bitvec_search")
        return out

    def search_device(self, d_bases_ptr, d_offs_ptr, n, d_verdicts_ptr):
        """asynchronous on the bit vector's stream; sync() waits"""
        _check(lib().urmapx_bitvec_search_device(self.h, d_bases_ptr, d_offs_ptr, n, d_verdicts_ptr), "urmapx_bitvec_search_device")

    def sync(self):
        _check(lib().urmapx_bitvec_sync(self.h), "urmapx_bitvec_sync")

    def last_ms(self):
        """device ms of the last build's include and exclude launches and of the last completed search launch"""
        ms = (C.c_float * 3)()
        _check(lib().urmapx_bitvec_last_ms(self.h, C.byref(ms)), "urmapx_bitvec_last_ms")
        return [float(x) for x in ms]

    def search_files(self, fastq1, out1, fastq2=None, out2=None, trunc_labels=False):
        """-search_bitvec (fastq2 None) / -search_bitvec2 file to file -> (reads or pairs found, read)"""
        cnt = (C.c_uint64 * 2)()
        err = C.create_string_buffer(1024)
        enc = lambda p: os.fsencode(p) if p else None
        rc = lib().urmapx_search_bitvec_files(self.h, enc(fastq1), enc(fastq2), enc(out1), enc(out2), BV_TRUNC_LABELS if trunc_labels else 0,
                                              C.byref(cnt), err, len(err))
        if rc != 0:
            raise UrmapxError(rc, "urmapx_search_bitvec_files: " + err.value.decode("latin-1"))
        return int(cnt[0]), int(cnt[1])

    def close(self):
        if self.h:
            lib().urmapx_bitvec_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_bitvec(device, ref_fa, excl_fa, word_length, bv_path):
    """urmap -make_bitvec ref_fa -input2 excl_fa -wordlength W -output bv_path -> (words included, words excluded)"""
    cnt = (C.c_uint64 * 2)()
    _check(lib().urmapx_make_bitvec(int(device), os.fsencode(ref_fa), os.fsencode(excl_fa), int(word_length), os.fsencode(bv_path), C.byref(cnt)),
           "urmapx_make_bitvec")
    return int(cnt[0]), int(cnt[1])


def decode_path(ops: np.ndarray) -> str:
    """Run-length path arena entries -> the reference's M/D/I path string."""
    return "".join("MDI"[int(o) & 3] * (int(o) >> 2) for o in ops)


class Mapper:
    """One mapping context (the State1 of one OMP thread in map.cpp:11-25), batch form."""

    def __init__(self, index: Index, device=0, method=6, params: Params | None = None):
        self.index = index
        self.device = device
        self.params = params if params is not None else params_for_method(method)
        h = C.c_void_p()
        self._text = None
        self.h = None
        _check(lib().urmapx_ctx_create(index.h, device, C.byref(self.params), C.byref(h)), "urmapx_ctx_create")
        self.h = h

    @property
    def arch(self):
        return lib().urmapx_device_arch(self.h).decode()

    def map_se(self, bases: np.ndarray, offs: np.ndarray, allow_unsupported=False):
        """-> (results structured array, path op arena).  Raises UrmapxError(E_UNSUPPORTED) if any read
        fell outside the device domain unless allow_unsupported (then check results['status'])."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        res = np.zeros(n, dtype=RESULT_DTYPE)
        cap = max(1, n * MAX_PATH_OPS)
        ops = np.zeros(cap, dtype=np.uint16)
        used = C.c_size_t(0)
        rc = lib().urmapx_map_se(self.h, bases.ctypes.data, offs.ctypes.data, n, res.ctypes.data, ops.ctypes.data, cap,
                                 C.byref(used))
        _check(rc, "urmapx_map_se", allow=(E_UNSUPPORTED,) if allow_unsupported else ())
        return res, ops[: used.value].copy()

    def set_pe_veryfast(self, on=True):
        _check(lib().urmapx_ctx_set_pe_veryfast(self.h, int(on)), "urmapx_ctx_set_pe_veryfast")

    def map_pe(self, bases: np.ndarray, offs: np.ndarray, allow_unsupported=False):
        """Pairs interleaved: reads 2i, 2i+1 are R1, R2 of pair i.  -> (results[2*npairs], path op arena)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        assert n % 2 == 0
        res = np.zeros(n, dtype=RESULT_DTYPE)
        cap = max(1, n * MAX_PATH_OPS)
        ops = np.zeros(cap, dtype=np.uint16)
        used = C.c_size_t(0)
        rc = lib().urmapx_map_pe(self.h, bases.ctypes.data, offs.ctypes.data, n // 2, res.ctypes.data, ops.ctypes.data,
                                 cap, C.byref(used))
        _check(rc, "urmapx_map_pe", allow=(E_UNSUPPORTED,) if allow_unsupported else ())
        return res, ops[: used.value].copy()

    def map_se_device(self, d_bases_ptr, d_offs_ptr, n, total_bases, max_read_len, d_results_ptr, d_path_ops_ptr,
                      d_path_used_ptr):
        _check(lib().urmapx_map_se_device(self.h, d_bases_ptr, d_offs_ptr, n, total_bases, max_read_len,
                                          d_results_ptr, d_path_ops_ptr, d_path_used_ptr), "urmapx_map_se_device")

    def map_pe_device(self, d_bases_ptr, d_offs_ptr, npairs, total_bases, max_read_len, d_results_ptr, d_path_ops_ptr,
                      d_path_used_ptr):
        _check(lib().urmapx_map_pe_device(self.h, d_bases_ptr, d_offs_ptr, npairs, total_bases, max_read_len,
                                          d_results_ptr, d_path_ops_ptr, d_path_used_ptr), "urmapx_map_pe_device")

    def sync(self):
        _check(lib().urmapx_ctx_sync(self.h), "urmapx_ctx_sync")

    def last_kernel_ms(self):
        ms = (C.c_float * 2)()
        _check(lib().urmapx_ctx_last_kernel_ms(self.h, C.byref(ms)), "urmapx_ctx_last_kernel_ms")
        return float(ms[0]), float(ms[1])

    def stage_ms(self):
        """ms of the launches of the last single-end device call: search, its DP launches (summed), its finalize launches
        (summed), the same three for the second pass, the general kernel over what both left flagged."""
        ms = (C.c_float * 7)()
        _check(lib().urmapx_ctx_stage_ms(self.h, C.byref(ms)), "urmapx_ctx_stage_ms")
        return [float(x) for x in ms]

    def seed_probe_device(self, d_bases_ptr, d_offs_ptr, n, total_bases, max_read_len):
        """the probe launch alone over reads resident in HBM -> its ms on the context's stream"""
        ms = C.c_float(0)
        _check(lib().urmapx_seed_probe_device(self.h, d_bases_ptr, d_offs_ptr, n, total_bases, max_read_len, C.byref(ms)), "urmapx_seed_probe_device")
        return float(ms.value)

    def phase3(self):
        """The search stage of the last single-end device call when phase 3 is parked (round 5): ms of the first search launch, of
        phase 3's DP launch and of the launch over the reads parked at phase 3; DpJobs made for phase 3, reads parked there."""
        ms = (C.c_float * 3)()
        st = (C.c_uint32 * 2)()
        _check(lib().urmapx_ctx_phase3(self.h, C.byref(ms), C.byref(st)), "urmapx_ctx_phase3")
        return [float(x) for x in ms], [int(x) for x in st]

    def round_ms(self):
        """ms of the first pass's phase-6 launches one by one: [(dp, finalize) per round]"""
        ms = (C.c_float * 16)()
        n = C.c_int(0)
        _check(lib().urmapx_ctx_round_ms(self.h, C.byref(ms), C.byref(n)), "urmapx_ctx_round_ms")
        return [(float(ms[2 * r]), float(ms[2 * r + 1])) for r in range(n.value)]

    def dp_rounds(self):
        """the rounds of phase 6 in the last single-end call as text: 'HSPs [0,2), [2,16), [16,...) of a read'"""
        lo = (C.c_uint32 * 8)()
        n = C.c_int(0)
        L = lib()
        L.urmapx_ctx_dp_rounds.argtypes = [C.c_void_p, C.POINTER(C.c_uint32 * 8), C.POINTER(C.c_int)]
        _check(L.urmapx_ctx_dp_rounds(self.h, C.byref(lo), C.byref(n)), "urmapx_ctx_dp_rounds")
        parts = [f"[{lo[r]},{lo[r + 1]})" if r + 1 < n.value else f"[{lo[r]},...)" for r in range(n.value)]
        return "HSPs " + ", ".join(parts) + " of a read"

    def dp_stats(self):
        """per pass: (HSPs handed to the DP launches, reads parked, DPs the ordered replay looked at, jobs gated before their DP)"""
        out = (C.c_uint32 * 8)()
        _check(lib().urmapx_ctx_dp_stats(self.h, C.byref(out)), "urmapx_ctx_dp_stats")
        return [int(x) for x in out]

    def set_pair_info(self, on=True):
        _check(lib().urmapx_ctx_set_pair_info(self.h, int(on)), "urmapx_ctx_set_pair_info")

    def pair_info(self, npairs):
        """urmapx_pair_info records of the last paired-end call (needs set_pair_info(True) before it)."""
        out = np.zeros(npairs, dtype=PAIR_INFO_DTYPE)
        _check(lib().urmapx_ctx_get_pair_info(self.h, out.ctypes.data, npairs), "urmapx_ctx_get_pair_info")
        return out

    def gather_microbench(self, n_loads=1 << 28):
        """Random 5-byte slot reads per second over the resident slot table (measurement aid)."""
        r = C.c_double(0.0)
        _check(lib().urmapx_ctx_gather_microbench(self.h, n_loads, C.byref(r)), "urmapx_ctx_gather_microbench")
        return r.value

    def phase_cycles(self):
        out = (C.c_uint64 * 12)()
        _check(lib().urmapx_ctx_phase_cycles(self.h, C.byref(out)), "urmapx_ctx_phase_cycles")
        return [int(x) for x in out]

    def read_cycles(self, n):
        """Shader cycles each of the first n reads of the last single-end call took (URMAPX_PHASE_STATS=1)."""
        out = np.zeros(n, dtype=np.uint32)
        _check(lib().urmapx_ctx_read_cycles(self.h, out.ctypes.data, n), "urmapx_ctx_read_cycles")
        return out.astype(np.int64) * 16

    def seed_probe(self, bases: np.ndarray, offs: np.ndarray):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        total = int(offs[-1])
        slots = np.zeros(2 * total, dtype=np.uint64)
        tallies = np.zeros(2 * total, dtype=np.uint8)
        positions = np.zeros(2 * total, dtype=np.uint32)
        _check(lib().urmapx_seed_probe(self.h, bases.ctypes.data, offs.ctypes.data, n, slots.ctypes.data,
                                       tallies.ctypes.data, positions.ctypes.data), "urmapx_seed_probe")
        return slots, tallies, positions

    def viterbi_batch(self, pairs, flags):
        """pairs: list of (A bytes, B bytes); flags: list of ints (bit0 Left, bit1 Right)."""
        n = len(pairs)
        a = np.frombuffer(b"".join(p[0] for p in pairs), dtype=np.uint8)
        b = np.frombuffer(b"".join(p[1] for p in pairs), dtype=np.uint8)
        ao = np.zeros(n + 1, dtype=np.uint32)
        bo = np.zeros(n + 1, dtype=np.uint32)
        ao[1:] = np.cumsum([len(p[0]) for p in pairs])
        bo[1:] = np.cumsum([len(p[1]) for p in pairs])
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        scores = np.zeros(n, dtype=np.float32)
        status = np.zeros(n, dtype=np.uint8)
        ops = np.zeros(n * MAX_PATH_OPS, dtype=np.uint16)
        nops = np.zeros(n, dtype=np.uint16)
        a_ = np.ascontiguousarray(a) if len(a) else np.zeros(1, np.uint8)
        b_ = np.ascontiguousarray(b) if len(b) else np.zeros(1, np.uint8)
        _check(lib().urmapx_viterbi_batch(self.h, a_.ctypes.data, ao.ctypes.data, b_.ctypes.data, bo.ctypes.data,
                                          fl.ctypes.data, n, scores.ctypes.data, status.ctypes.data, ops.ctypes.data,
                                          nops.ctypes.data), "urmapx_viterbi_batch")
        paths = [decode_path(ops[i * MAX_PATH_OPS: i * MAX_PATH_OPS + int(nops[i])]) for i in range(n)]
        return scores, status, paths

    def set_bgzf(self, on=True):
        """The text stage of this mapper delivers each chunk's SAM text as BGZF members (urmapx_text_set_bgzf): report['sam_bytes'] is
        the compressed size, report['sam_text_bytes'] the text's."""
        if self._text is None:
            t = C.c_void_p()
            _check(lib().urmapx_text_create(self.h, C.byref(t)), "urmapx_text_create")
            self._text = t
        L = lib()
        L.urmapx_text_set_bgzf.argtypes = [C.c_void_p, C.c_int]
        _check(L.urmapx_text_set_bgzf(self._text, int(bool(on))), "urmapx_text_set_bgzf")

    def set_bam(self, on=True):
        """The text stage of this mapper delivers each chunk's BAM alignment records instead of SAM text (urmapx_text_set_bam): raw
        records, or BGZF members of them after set_bgzf; report['sam_text_bytes'] is the uncompressed record bytes either way."""
        if self._text is None:
            t = C.c_void_p()
            _check(lib().urmapx_text_create(self.h, C.byref(t)), "urmapx_text_create")
            self._text = t
        L = lib()
        L.urmapx_text_set_bam.argtypes = [C.c_void_p, C.c_int]
        _check(L.urmapx_text_set_bam(self._text, int(bool(on))), "urmapx_text_set_bam")

    def set_tags(self, tags=0, rg_id=None):
        """The text stage of this mapper writes the optional fields NM MD AS (tags = TAG_* bits) and RG:Z:rg_id behind every record
        (urmapx_text_set_tags; tags_gpu.hip), SAM text and BAM records alike.  0 and None: records end at QUAL again."""
        if self._text is None:
            t = C.c_void_p()
            _check(lib().urmapx_text_create(self.h, C.byref(t)), "urmapx_text_create")
            self._text = t
        L = lib()
        L.urmapx_text_set_tags.argtypes = [C.c_void_p, C.c_uint, C.c_char_p]
        _check(L.urmapx_text_set_tags(self._text, int(tags), rg_id.encode("latin-1") if isinstance(rg_id, str) else rg_id), "urmapx_text_set_tags")

    def tag_ms(self):
        """device ms of the two tag passes of the last chunk (urmapx_text_tag_ms): (the counting pass, the writing pass)"""
        ms = (C.c_float * 2)()
        if self._text is None:
            return 0.0, 0.0
        _check(lib().urmapx_text_tag_ms(self._text, C.byref(ms)), "urmapx_text_tag_ms")
        return float(ms[0]), float(ms[1])

    def tags_batch(self, bases: np.ndarray, offs: np.ndarray, results: np.ndarray, ops: np.ndarray, tags=TAG_ALL):
        """The tag passes alone on host arrays (urmapx_tags_batch; the device functions the text stage runs).
        -> (NM per record, tagged flag per record, [MD text per record])"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        results = np.ascontiguousarray(results)
        ops = np.ascontiguousarray(ops, dtype=np.uint16)
        n = len(offs) - 1
        nm = np.zeros(max(1, n), dtype=np.uint32)
        tagged = np.zeros(max(1, n), dtype=np.uint8)
        md_offs = np.zeros(n + 1, dtype=np.uint64)
        cap = 2 * int(offs[-1]) + 64 * n + 1024
        for r in results:  # a deletion's letters come on top of the read's columns
            if r["dbpos"] != 0xFFFFFFFF and r["path_nops"]:
                p = ops[int(r["path_off"]): int(r["path_off"]) + int(r["path_nops"])]
                cap += 2 * int((p[(p & 3) == 2] >> 2).sum())
        md = np.zeros(cap, dtype=np.uint8)
        used = C.c_size_t(0)
        L = lib()
        L.urmapx_tags_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
        _check(L.urmapx_tags_batch(self.h, bases.ctypes.data, offs.ctypes.data, n, results.ctypes.data, ops.ctypes.data if len(ops) else None,
                                   len(ops), int(tags), nm.ctypes.data, tagged.ctypes.data, md.ctypes.data, cap, md_offs.ctypes.data,
                                   C.byref(used)), "urmapx_tags_batch")
        texts = [md[int(md_offs[i]): int(md_offs[i + 1])].tobytes().decode() for i in range(n)]
        return nm[:n].copy(), tagged[:n].copy(), texts

    def map_text_se(self, fastq: bytes, minq=10, sam_cap=None):
        """A chunk of FASTQ text (cut after a record's last newline) -> (the SAM text of its records | None, report dict).
        None with report['reason'] != TEXT_OK: the device parser does not take the chunk as it is (see urmapx.h)."""
        if self._text is None:
            t = C.c_void_p()
            _check(lib().urmapx_text_create(self.h, C.byref(t)), "urmapx_text_create")
            self._text = t
        src = np.frombuffer(fastq, dtype=np.uint8)
        cap = sam_cap if sam_cap is not None else 2 * len(src) + 4096 * 64
        out = np.empty(max(1, cap), dtype=np.uint8)
        rep = TextReport()
        _check(lib().urmapx_text_map_se(self._text, src.ctypes.data if len(src) else None, len(src), minq, out.ctypes.data, cap, C.byref(rep)),
               "urmapx_text_map_se")
        d = {k: int(getattr(rep, k)) for k, _ in TextReport._fields_}
        if rep.reason != TEXT_OK:
            return None, d
        return out[: rep.sam_bytes].tobytes(), d

    def map_text_pe(self, fastq1: bytes, fastq2: bytes, minq=10, sam_cap=None):
        """Chunks of the two mate files with the same number of records -> (SAM text of the pairs | None, report dict)."""
        if self._text is None:
            t = C.c_void_p()
            _check(lib().urmapx_text_create(self.h, C.byref(t)), "urmapx_text_create")
            self._text = t
        a, b = np.frombuffer(fastq1, dtype=np.uint8), np.frombuffer(fastq2, dtype=np.uint8)
        cap = sam_cap if sam_cap is not None else 2 * (len(a) + len(b)) + 4096 * 64
        out = np.empty(max(1, cap), dtype=np.uint8)
        rep = TextReport()
        _check(lib().urmapx_text_map_pe(self._text, a.ctypes.data if len(a) else out.ctypes.data, len(a), b.ctypes.data if len(b) else out.ctypes.data,
                                        len(b), minq, out.ctypes.data, cap, C.byref(rep)), "urmapx_text_map_pe")
        d = {k: int(getattr(rep, k)) for k, _ in TextReport._fields_}
        if rep.reason != TEXT_OK:
            return None, d
        return out[: rep.sam_bytes].tobytes(), d

    def map_text_se_stream(self, chunks, minq=10, sam_caps=None):
        """Chunks of one FASTQ file through the context with the copy back deferred (urmapx_text_set_deferred): chunk i + 1 is handed
        over before chunk i's text is waited for, as a lane of urmapx_map_files does.  -> [(SAM text | None, report dict)] per chunk.
        sam_caps[i] (optional): the buffer offered for chunk i; too small -> urmapx_text_fetch_sam into a larger one, deferred too."""
        if self._text is None:
            t = C.c_void_p()
            _check(lib().urmapx_text_create(self.h, C.byref(t)), "urmapx_text_create")
            self._text = t
        _check(lib().urmapx_text_set_deferred(self._text, 1), "urmapx_text_set_deferred")
        res, prev = [], None

        def finish(item):
            out, d0 = item
            if d0["reason"] != TEXT_DEFERRED:
                return (b"" if d0["reason"] == TEXT_OK else None), d0
            rep = TextReport()
            _check(lib().urmapx_text_wait(self._text, C.byref(rep)), "urmapx_text_wait")
            d = {k: (int(getattr(rep, k)) if not k.startswith("ms_") else float(getattr(rep, k))) for k, _ in TextReport._fields_}
            return (out[: rep.sam_bytes].tobytes() if rep.reason == TEXT_OK else None), d

        try:
            for i, fastq in enumerate(chunks):
                src = np.frombuffer(fastq, dtype=np.uint8)
                cap = sam_caps[i] if sam_caps is not None and sam_caps[i] is not None else 2 * len(src) + 4096 * 64
                out = np.empty(max(1, cap), dtype=np.uint8)
                rep = TextReport()
                _check(lib().urmapx_text_map_se(self._text, src.ctypes.data if len(src) else None, len(src), minq, out.ctypes.data, cap, C.byref(rep)),
                       "urmapx_text_map_se")
                if rep.reason == TEXT_SAM_CAP:
                    out = np.empty(int(rep.sam_bytes) + 64, dtype=np.uint8)
                    _check(lib().urmapx_text_fetch_sam(self._text, out.ctypes.data, len(out), C.byref(rep)), "urmapx_text_fetch_sam")
                d = {k: (int(getattr(rep, k)) if not k.startswith("ms_") else float(getattr(rep, k))) for k, _ in TextReport._fields_}
                if prev is not None:
                    item, prev = prev, None
                    res.append(finish(item))
                prev = (out, d)
            if prev is not None:
                item, prev = prev, None
                res.append(finish(item))
        finally:
            #  after an exception a chunk may still be on its way: it is waited for before the mode is switched back, and nothing
            # is raised from here -- the exception that ended the loop is the one the caller sees
            rep = TextReport()
            while lib().urmapx_text_wait(self._text, C.byref(rep)) == 0:
                pass
            lib().urmapx_text_set_deferred(self._text, 0)
        return res

    def fetch_text_sam(self, sam_cap):
        """After map_text_se returned TEXT_SAM_CAP: the text of that chunk (the search is not run again)."""
        out = np.empty(max(1, sam_cap), dtype=np.uint8)
        rep = TextReport()
        _check(lib().urmapx_text_fetch_sam(self._text, out.ctypes.data, sam_cap, C.byref(rep)), "urmapx_text_fetch_sam")
        d = {k: int(getattr(rep, k)) for k, _ in TextReport._fields_}
        return (out[: rep.sam_bytes].tobytes() if rep.reason == TEXT_OK else None), d

    def close(self):
        if self._text is not None:
            lib().urmapx_text_destroy(self._text)
            self._text = None
        if self.h:
            lib().urmapx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def interleave_pairs(a, b):
    """(labels, bases, offs, quals) of R1 and of R2 -> one interleaved set (R1_0, R2_0, R1_1, ...)."""
    la, ba, oa, qa = a
    lb, bb, ob, qb = b
    assert len(la) == len(lb)
    labels, seqs, quals = [], [], []
    for i in range(len(la)):
        labels += [la[i], lb[i]]
        seqs += [ba[int(oa[i]):int(oa[i + 1])], bb[int(ob[i]):int(ob[i + 1])]]
        quals += [qa[int(oa[i]):int(oa[i + 1])], qb[int(ob[i]):int(ob[i + 1])]]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return labels, np.concatenate(seqs), offs, np.concatenate(quals)


class FastqReader:
    """ctypes view of urmapx_fastq_* (the product's FASTQSeqSource): iterate batches of records."""

    def __init__(self, path):
        self._h = C.c_void_p()
        rc = lib().urmapx_fastq_open(os.fsencode(path), C.byref(self._h))
        if rc:
            raise UrmapxError(rc, f"urmapx_fastq_open({path})")

    def next(self, max_reads):
        """-> (labels list[str], bases uint8, offs uint64, quals uint8) or None at end of file."""
        L = lib()
        pb, pq, po, pl, plo = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = L.urmapx_fastq_next(self._h, max_reads, C.byref(pb), C.byref(pq), C.byref(po), C.byref(pl), C.byref(plo))
        if n < 0:
            raise ValueError(L.urmapx_fastq_error(self._h).decode())
        if n == 0:
            return None
        offs = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        nb = int(offs[-1])
        if nb:
            bases = np.ctypeslib.as_array(C.cast(pb, C.POINTER(C.c_uint8)), shape=(nb,)).copy()
            quals = np.ctypeslib.as_array(C.cast(pq, C.POINTER(C.c_uint8)), shape=(nb,)).copy()
        else:
            bases = np.zeros(0, dtype=np.uint8)
            quals = np.zeros(0, dtype=np.uint8)
        lo = np.ctypeslib.as_array(C.cast(plo, C.POINTER(C.c_uint64)), shape=(n,))
        labels = [C.string_at(pl.value + int(o)).decode("latin-1") for o in lo]
        return labels, bases, offs, quals

    def close(self):
        if self._h:
            lib().urmapx_fastq_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_fastq_arrays(path, batch=1 << 16):
    """FASTQ -> (labels, bases uint8, offs uint64, quals uint8) through the product's reader."""
    rd = FastqReader(path)
    labels, bl, ql, lens = [], [], [], []
    while True:
        b = rd.next(batch)
        if b is None:
            break
        labels += b[0]
        bl.append(b[1])
        ql.append(b[3])
        lens.append(np.diff(b[2]))
    rd.close()
    offs = np.zeros(len(labels) + 1, dtype=np.uint64)
    if lens:
        offs[1:] = np.cumsum(np.concatenate(lens))
    bases = np.concatenate(bl) if bl else np.zeros(0, dtype=np.uint8)
    qual = np.concatenate(ql) if ql else np.zeros(0, dtype=np.uint8)
    return labels, bases, offs, qual
